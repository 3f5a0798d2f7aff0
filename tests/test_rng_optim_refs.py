"""The two independent references the GPU tests lean on, checked where no GPU is needed.

* ``_philox.philox4x32_10`` against the Random123 known-answer vectors (``kat_vectors`` of the
  Random123 distribution, the three ``philox4x32 10`` lines), so the device streams are compared with
  Philox4x32-10 as published, not with a transcription of the kernel.
* ``hfrep.train.optim.KerasOptimizer`` on the CPU in fp64 -- the twin that every CPU engine and every
  GPU-vs-CPU trainer test rests on -- against the Keras 2.7 rules written out in ``_keras_optim_ref``.
"""
import numpy as np
import pytest
import torch

import _keras_optim_ref as K
import _philox as P

KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = P.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]
    # the same three, as one vectorised call
    got = P.philox4x32_10(np.array([c for c, _, _ in KAT], dtype=np.uint64), np.array([k for _, k, _ in KAT], dtype=np.uint64))
    assert got.shape == (3, 4) and [tuple(int(x) for x in row) for row in got] == [w for _, _, w in KAT]


def test_philox_stream_layout():
    """``stream_blocks`` puts the tag in word 0, the 64-bit counter in words 2 and 3 (with the carry) and
    the 64-bit seed in the key; the helpers slice quads the way a fill of ``n`` values does."""
    seed, ctr = 0x7234567889ABCDEF, 2 ** 32 - 2
    blocks = P.stream_blocks(seed, ctr, 4, P.TAG_FILL)
    key = np.array([0x89ABCDEF, 0x72345678], dtype=np.uint64)
    for i, (lo, hi) in enumerate([(0xFFFFFFFE, 0), (0xFFFFFFFF, 0), (0, 1), (1, 1)]):
        want = P.philox4x32_10(np.array([P.TAG_FILL, 0, lo, hi], dtype=np.uint64), key)
        assert np.array_equal(blocks[i], want)
    assert P.stream_blocks(seed, ctr, 0, P.TAG_FILL).shape == (0, 4)
    assert not np.array_equal(P.stream_blocks(seed, ctr, 4, P.TAG_SAMPLE), blocks)
    u = P.uniform_ref(seed, ctr, 13)
    assert u.shape == (13,) and np.array_equal(u, P.uniform_ref(seed, ctr, 16)[:13])
    assert np.array_equal(u[4:8], ((blocks[1] >> 8).astype(np.float64) + 1) / 2 ** 24)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and u.min() > 0 and u.max() <= 1
    assert P.uniform_ref(seed, ctr, 0).shape == (0,)
    z = P.normal_ref(seed, ctr, 6)
    u8 = P.uniform_ref(seed, ctr, 8)
    assert np.allclose(z[4] ** 2 + z[5] ** 2, -2 * np.log(u8[4]), rtol=1e-14)
    assert np.isclose(np.arctan2(z[5], z[4]) % (2 * np.pi), 2 * np.pi * u8[5], rtol=1e-12)
    idx = P.window_index_ref(seed, ctr, 5, 7)
    r = P.stream_blocks(seed, ctr, 5, P.TAG_SAMPLE)
    assert [int(i) for i in idx] == [((int(a) << 32) | int(b)) % 7 for a, b in r[:, :2]]


# ------------------------------------------------------------------------------------------ optimizers
# the workload's hyper-parameters: the WGAN(-GP) critics' RMSprop(5e-5) with the 0.01 weight clip, the
# GAN's Adam(2e-4, 0.5), the autoencoder's Nadam()
HYPER = {
    "rmsprop": dict(lr=5e-5, clip=0.01, kw={}, scale=0.01),
    "adam": dict(lr=2e-4, clip=0.0, kw=dict(beta_1=0.5), scale=1.0),
    "nadam": dict(lr=1e-3, clip=0.0, kw={}, scale=1.0),
}
STEPS, N = 300, 257


def _rel(got, want):
    """max |got - want| relative to the largest magnitude of ``want``: the fp64 roundings of 300 steps
    land on the parameter's own scale (a random walk of ~1e-16 steps), so an element that happens to sit
    near zero is measured against the buffer, not against itself."""
    want = np.asarray(want, dtype=np.float64)
    got = got.detach().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.dtype == np.float64
    return float(np.abs(got - want).max() / max(np.abs(want).max(), np.finfo(np.float64).tiny))


def _check(opt, ref, flats, names, ps, what):
    for f, name, p in zip(flats, names, ps):
        assert _rel(f, p) <= 1e-12, f"{what}: parameters {name}"
        for s, rs in zip(opt._slots(f), ref.slots[name]):
            assert _rel(s, rs) <= 1e-12, f"{what}: slot of {name}"
    assert opt.iterations.item() == ref.iterations, what
    if ref.kind == "nadam":
        assert _rel(opt.m_cache.double(), [ref.m_cache]) <= 1e-12, f"{what}: momentum cache"


@pytest.mark.parametrize("mode", ["gscale", "shared", "group"])
@pytest.mark.parametrize("kind", ["rmsprop", "adam", "nadam"])
def test_cpu_optimizer_follows_keras_rules(kind, mode):
    """300 steps of the CPU fp64 ``KerasOptimizer`` against the written Keras 2.7 rules, to 1e-12 of the
    buffer's scale: with the data-parallel ``gscale``, with one optimizer object applied in turn to two
    buffers (the counter ticks on every ``apply``), and through ``apply_group`` (one tick for both)."""
    from hfrep.train.optim import KerasOptimizer

    h = HYPER[kind]
    rng = np.random.RandomState(20 + ["rmsprop", "adam", "nadam"].index(kind))
    names = ["a"] if mode == "gscale" else ["a", "b"]
    gscale = 0.25 if mode == "gscale" else 1.0
    ps = [rng.randn(N) * h["scale"] for _ in names]
    flats = [torch.tensor(p, dtype=torch.float64) for p in ps]
    opt = KerasOptimizer(kind, h["lr"], **h["kw"])
    ref = K.RefOptimizer(kind, h["lr"], b1=h["kw"].get("beta_1", 0.9))
    for step in range(1, STEPS + 1):
        gs = [rng.randn(N) * (4.0 if mode == "gscale" else 1.0) for _ in names]
        if mode == "group":
            for f, g in zip(flats, gs):
                f.grad = torch.tensor(g, dtype=torch.float64)
            opt.apply_group(flats, clip=h["clip"], gscale=gscale)
            ps = ref.apply_group(list(zip(names, ps, gs)), clip=h["clip"], gscale=gscale)
        else:
            for i, g in enumerate(gs):
                opt.apply(flats[i], torch.tensor(g, dtype=torch.float64), clip=h["clip"], gscale=gscale)
                ps[i] = ref.apply(names[i], ps[i], g, clip=h["clip"], gscale=gscale)
        if step in (1, 2, 10, 100, STEPS):
            _check(opt, ref, flats, names, ps, f"{kind}/{mode} step {step}")
    assert ref.iterations == (STEPS if mode != "shared" else 2 * STEPS)
    if h["clip"] > 0:
        assert all(f.abs().max().item() <= h["clip"] for f in flats)
        assert any((f.abs() == h["clip"]).any().item() for f in flats), "the clip never bound: the case checks nothing"
