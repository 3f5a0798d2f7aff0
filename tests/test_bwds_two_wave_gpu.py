"""The split-recurrent fp32 BPTT on two waves per SIMD (lstmf_bwds2_kernel, set_lstmf_bwd_impl 4) against the
four-wave split BPTT (lstmf_bwds_kernel, value 3): the eight-wave kernel gives the 7 real dh_rec tiles and the 25
real cell groups to more waves and runs the same arithmetic per tile and per cell, so dZ is bitwise equal -- with a
materialised dH, with the head adjoint generated in the kernel (HEAD) and without any dH (a null seed).  Launches
that keep the h adjoints aH run the four-wave kernel under value 4 too (the eight-wave form measured no clear gain
there, profiles/bwds_two_wave/README.md); their cases hold whatever value 4 selects to the same bits, dZ and aH.
Three launches of value 4 are bitwise equal (this family's races have shown up as run-to-run drift).  (The op
rejects head factors without the row factor, so HEAD always comes with both; the null-seed case is the one that
runs a HEAD-less kernel without a dH tensor.)"""
import pytest
import torch

from hfrep.ops import reference as R

pytestmark = pytest.mark.gpu

H, K = 100, 32
TOL32 = dict(rtol=2e-4, atol=2e-5)  # the suite's fp32-kernel-against-fp64 tolerance (tests/test_kernels_gpu.py)
VARIANTS = ["plain", "head", "ah", "head_ah", "null"]


def _ops():
    from hfrep.ops import _native

    return _native.native()


def _inputs(B, T, act, cuda, seed=93):
    from hfrep.ops import functional as Fn

    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, K, generator=g) * 0.5
    W = torch.randn(K, 4 * H, generator=g) * (1.0 / K ** 0.5)
    b = torch.randn(4 * H, generator=g) * 0.1
    U = torch.randn(H, 4 * H, generator=g) * (1.0 / H ** 0.5)
    dH = torch.randn(B, T, H, generator=g)
    d = torch.randn(B, 1, generator=g)
    w = torch.randn(T * H, 1, generator=g)
    cpu = dict(x=x, W=W, b=b, U=U, dH=dH, d=d, w=w)
    dev = {k: v.to(cuda) for k, v in cpu.items()}
    hs, tape = Fn.lstm_layer_fwd(dev["x"], dev["W"], dev["b"], dev["U"], act, True)
    dev["hs"], dev["tape"] = hs, tape
    return cpu, dev


def _run(variant, dev, act):
    """(dZ, aH or None) of one BPTT launch under the current switch."""
    from hfrep.ops import functional as Fn

    B, T = dev["dH"].shape[:2]
    seed = Fn.OuterAdjoint(dev["d"], dev["w"], (B, T, H)) if variant.startswith("head") else dev["dH"]
    if variant == "null":
        return _ops().lstmf_bwd(None, dev["tape"].t, dev["U"], int(act), B, T), None
    if variant.endswith("ah"):
        dZ, _, ah = Fn.lstm_layer_bwd_keep(seed, dev["tape"], dev["U"], act)
        return dZ, ah
    return Fn.lstm_layer_bwd(seed, dev["tape"], dev["U"], act), None


def _assert_same(new, ref, what):
    """Bitwise, the likely owners first: units 96..99 (the last cell group, the fourth one of the wave without a
    tile), then each row half of the first row block, then everything."""
    n = new.view(new.shape[0], new.shape[1], -1, H)  # dZ: (B, T, 4, H); aH: (B, T, 1, H)
    r = ref.view(ref.shape[0], ref.shape[1], -1, H)
    assert torch.equal(n[..., 96:], r[..., 96:]), f"{what}: units 96..99"
    assert torch.equal(n[:16], r[:16]), f"{what}: row half 0 of the first row block"
    assert torch.equal(n[16:32], r[16:32]), f"{what}: row half 1 of the first row block"
    assert torch.equal(new, ref), what


def test_switch_returns_previous_and_default(cuda):
    ops = _ops()
    first = ops.set_lstmf_bwd_impl(3)
    try:
        assert first == 4  # the library default: the eight-wave kernel where no h adjoints are kept
        assert ops.set_lstmf_bwd_impl(4) == 3
        assert ops.lstmf_ahd_supported()
        assert ops.set_lstmf_bwd_impl(2) == 4
        assert not ops.lstmf_ahd_supported()
        assert ops.set_lstmf_bwd_impl(3) == 2
    finally:
        ops.set_lstmf_bwd_impl(first)


CASES = [(act, B, T) for act in (0, 1, 2) for B, T in ((1, 1), (16, 1), (17, 2), (33, 2), (70, 24))] + [(2, 8237, 2)]


@pytest.mark.parametrize("act,B,T", CASES)
def test_eight_wave_split_bptt_bitwise(cuda, act, B, T):
    _, dev = _inputs(B, T, act, cuda)
    ops = _ops()
    prev = ops.set_lstmf_bwd_impl(3)
    try:
        ref = {v: _run(v, dev, act) for v in VARIANTS}
        ops.set_lstmf_bwd_impl(4)
        new = {v: [_run(v, dev, act) for _ in range(3)] for v in VARIANTS}
    finally:
        ops.set_lstmf_bwd_impl(prev)
    for v in VARIANTS:
        assert torch.isfinite(ref[v][0]).all()
        for i, (dZ, ah) in enumerate(new[v]):
            _assert_same(dZ, ref[v][0], f"dZ {v} launch {i}")
            if ah is not None:
                _assert_same(ah, ref[v][1], f"aH {v} launch {i}")


def test_eight_wave_dz_through_its_consumers(cuda):
    """impl 4's dZ through the weight gradients (lstmf_wgrad) and the input gradient (lstmf_dgrad): bitwise the
    results from impl 3's dZ."""
    from hfrep.ops import functional as Fn

    act, B, T = 2, 70, 24
    _, dev = _inputs(B, T, act, cuda)
    ops = _ops()
    prev = ops.set_lstmf_bwd_impl(3)
    out = {}
    try:
        for impl in (3, 4):
            ops.set_lstmf_bwd_impl(impl)
            dZ = Fn.lstm_layer_bwd(dev["dH"], dev["tape"], dev["U"], act)
            gW, gU, gb = (torch.zeros(K, 4 * H, device=cuda), torch.zeros(H, 4 * H, device=cuda),
                          torch.zeros(4 * H, device=cuda))
            Fn.lstm_wgrad_(dev["x"], dev["hs"], dZ, gW, gU, gb)
            out[impl] = (gW, gU, gb, Fn.linear_dgrad(dZ, dev["W"]))
    finally:
        ops.set_lstmf_bwd_impl(prev)
    for a, c, name in zip(out[4], out[3], ("gW", "gU", "gb", "dX")):
        assert torch.isfinite(c).all() and c.abs().max() > 0
        assert torch.equal(a, c), name


def test_eight_wave_head_ah_vs_fp64(cuda):
    """HEAD + aH under impl 4 against fp64 at the workload's T, and HEAD alone (the eight-wave kernel): dZ within
    the split BPTT's bound (twice the exact fp32 kernel's error plus fp32 noise, tests/test_kernels_gpu.py
    test_lstmf_split_bptt_vs_exact; the exact kernel takes the materialised head adjoint), aH within the suite's
    fp32 tolerance."""
    from hfrep.ops import functional as Fn

    act, B, T = 2, 70, 24
    cpu, dev = _inputs(B, T, act, cuda)
    zx = cpu["x"].double() @ cpu["W"].double() + cpu["b"].double()
    _, rg, rc = R.lstm_seq_fwd(zx, cpu["U"].double(), act)
    seed = (cpu["d"].double() * cpu["w"].double().reshape(1, -1)).reshape(B, T, H)
    rdz, rah = R.lstm_seq_bwd_ahd(seed, rg, rc, cpu["U"].double(), act)
    ops = _ops()
    prev = ops.set_lstmf_bwd_impl(2)
    try:
        exact = Fn.lstm_layer_bwd(Fn.OuterAdjoint(dev["d"], dev["w"], (B, T, H)), dev["tape"], dev["U"], act)
        ops.set_lstmf_bwd_impl(4)
        dZ, ah = _run("head_ah", dev, act)
        dZh, _ = _run("head", dev, act)
    finally:
        ops.set_lstmf_bwd_impl(prev)
    e2 = (exact.double().cpu() - rdz).abs().max().item()
    e4 = (dZ.double().cpu() - rdz).abs().max().item()
    ea, sa = (ah.double().cpu() - rah).abs().max().item(), rah.abs().max().item()
    print(f"max abs err dZ exact {e2:.3e} eight-wave split {e4:.3e}; aH {ea:.3e} (scale {sa:.3e})")
    assert torch.isfinite(dZ).all() and torch.isfinite(ah).all()
    assert e4 <= 2 * e2 + 2e-6, (e2, e4)
    eh = (dZh.double().cpu() - rdz).abs().max().item()
    assert torch.isfinite(dZh).all() and eh <= 2 * e2 + 2e-6, (e2, eh)
    assert ea <= TOL32["atol"] * max(1.0, sa) + TOL32["rtol"] * sa, (ea, sa)
