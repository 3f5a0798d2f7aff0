"""GAN_eval's KS, ACF, Lp and naive-Bayes divergence metrics on an MI355X (csrc/evalm.hip; run with -m gpu).

* every native op against its float64 oracle (ops/reference.py, run on the CPU on the same float32 values):
  ``ks_stat`` equal to 1e-12 (an integer count difference over n), ``acf_mean`` and ``lp_cols`` abs <= 1e-12
  (``lp_cols`` at the larger shapes added here: n 2^-53 of the largest sum, see the test),
  ``nb_divergences`` rel <= 1e-10: float64 against float64 with another summation order;
* the KS chunk edges (16 384 keys per sorted chunk): one full chunk, one element over, three chunks, and
  2^20 + 5 rows, with 64-level values so that equal keys sit in different chunks and merge tiles;
* ``GANEval(device=cuda)`` against ``GANEval()`` for the six metrics.  The host path sees the same float32
  values: KS (the same integer statistic, the same p-value formula), the ACF and the divergences do their
  arithmetic in float64 on both sides, rel 1e-9; ``lp_dist``'s host path subtracts and sums in float32
  (numpy's pairwise sum of n = 16 800 terms: about log2(n) 2^-24 = 8e-7), rel 1e-5;
* one upload per array, one ``nb_divergences`` launch for the three NB metrics; bitwise repeatability;
  the debug poison (an output or slab element no kernel wrote would be NaN); the argument checks.
"""
import functools

import numpy as np
import pytest
import torch
from sklearn.naive_bayes import GaussianNB

from hfrep.eval import gan_eval
from hfrep.eval.gan_eval import GANEval
from hfrep.ops import _native
from hfrep.ops import functional as Fn
from hfrep.ops import reference as R

pytestmark = pytest.mark.gpu

SHAPES3 = [(37, 24, 5), (9, 12, 3), (300, 48, 35), (20, 168, 36)]
NB_SHAPES = [(37, 24, 5), (300, 48, 35), (20, 168, 36), (6, 168, 64)]  # the last: tables too large for the LDS
# 16 384 keys per sorted chunk, 4 096 per merge tile: one chunk (no merge pass), one key over (a run of 1), three
# chunks (an odd run out, then runs of 32 768 + 7 232), and 2^20 + 5 rows (65 chunks, seven passes, past wdist's n)
KS_CASES = [(12000, 5, False), (16391, 3, True), (16384, 3, True), (16385, 3, True), (40000, 3, True),
            ((1 << 20) + 5, 2, True)]
LP_SHAPES = [(37 * 24, 5), (300 * 48, 35), (1001, 300)]  # the last: more than one column tile
_id = lambda s: "x".join(str(int(v)) for v in s)  # noqa: E731


def _sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


@functools.lru_cache(maxsize=None)
def _pair(shape, levels=False):
    """real uniform, fake sigmoid-of-normal, float32 (64 levels: about n / 64 ties per value); read only."""
    rs = np.random.RandomState(sum(shape) + 7)
    real, fake = rs.rand(*shape).astype(np.float32), _sigmoid(rs.randn(*shape)).astype(np.float32)
    if levels:
        real, fake = (np.floor(np.clip(a, 0.0, 0.999999) * 64.0).astype(np.float32) / 64.0 for a in (real, fake))
    real.setflags(write=False)
    fake.setflags(write=False)
    return real, fake


@functools.lru_cache(maxsize=None)
def _fitted(T, F):
    ds = np.random.RandomState(100 + T + F).rand(64, T, F).astype(np.float32)
    gnb = GaussianNB().fit(np.transpose(ds, (0, 2, 1)).reshape(-1, T), np.repeat(np.arange(F), 64))
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
                 for a in (gnb.theta_, gnb.var_, np.log(gnb.class_prior_)))


def _t(a, dev=None):
    return torch.tensor(a).to(dev or "cpu")  # a copy: the shared inputs are read-only arrays


@functools.lru_cache(maxsize=None)
def _oracle(op, shape, levels=False):
    real, fake = _pair(shape, levels)
    if op == "ks":
        return R.ks_stat(_t(fake), Fn.wdist_ref(_t(real))).numpy()
    if op == "acf":
        return R.acf_mean(_t(real), 17).numpy()
    if op == "lp":
        return R.lp_cols(_t(real), _t(fake)).numpy()
    return R.nb_divergences(_t(real), _t(fake), *_fitted(shape[1], shape[2])).numpy()


def _native_op(op, shape, dev, levels=False):
    real, fake = _pair(shape, levels)
    if op == "ks":
        out = Fn.ks_stat(_t(fake, dev), Fn.wdist_ref(_t(real, dev)))
    elif op == "acf":
        out = Fn.acf_mean(_t(real, dev), 17)
    elif op == "lp":
        out = Fn.lp_cols(_t(real, dev), _t(fake, dev))
    else:
        out = Fn.nb_divergences(_t(real, dev), _t(fake, dev), *(p.to(dev) for p in _fitted(shape[1], shape[2])))
    assert out.dtype == torch.float64 and out.is_cuda
    return out


@pytest.mark.parametrize("case", KS_CASES, ids=_id)
def test_ks_stat_matches_oracle(cuda, case):
    n, F, levels = case
    got, want = _native_op("ks", (n, F), cuda, levels).cpu().numpy(), _oracle("ks", (n, F), levels)
    print(f"ks_stat {n}x{F} levels={levels}: got {got}, worst difference {np.abs(got - want).max():.3e}")
    assert got.shape == (F,) and np.isfinite(got).all() and (want > 0.01).all()
    assert np.abs(got - want).max() <= 1e-12, (got, want)


def test_ks_stat_non_finite(cuda):
    """+-inf are ordinary values, zeros of either sign one value; a NaN on either side makes its column NaN."""
    real, fake = (a.copy() for a in _pair((16391, 4)))
    real[3, 0] = fake[5, 0] = fake[16390, 0] = np.inf
    real[7, 0] = -np.inf
    real[:10, 1], fake[:7, 1] = -0.0, 0.0
    real[11, 2] = np.nan
    fake[16390, 3] = np.nan  # the second chunk's last element
    want = R.ks_stat(_t(fake), Fn.wdist_ref(_t(real))).numpy()
    got = Fn.ks_stat(_t(fake, cuda), Fn.wdist_ref(_t(real, cuda))).cpu().numpy()
    assert np.isnan(got[2]) and np.isnan(got[3]) and np.isnan(want[2:]).all()
    assert np.abs(got[:2] - want[:2]).max() <= 1e-12, (got, want)


@pytest.mark.parametrize("shape", SHAPES3, ids=_id)
def test_acf_mean_matches_oracle(cuda, shape):
    got, want = _native_op("acf", shape, cuda).cpu().numpy(), _oracle("acf", shape)
    assert got.shape == (shape[2], 18) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[:, shape[1]:]).all() and np.isfinite(got[:, : min(shape[1], 18)]).all()
    err = np.nanmax(np.abs(got - want))
    print(f"acf_mean {shape}: worst absolute difference {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("shape", LP_SHAPES, ids=_id)
def test_lp_cols_matches_oracle(cuda, shape):
    got, want = _native_op("lp", shape, cuda).cpu().numpy(), _oracle("lp", shape)
    assert got.shape == (3, shape[1]) and np.isfinite(got).all()
    err = np.abs(got - want).max(axis=1)
    # abs 1e-12 at (888, 5), where the sums stay below 512 (a few ulp); at the larger shapes added here one ulp
    # of a sum is already 9e-13, so the bound is the worst case of a float64 sum of n terms taken in another
    # order, n 2^-53 relative to the largest sum (a dropped or doubled element is off by ~0.1)
    gate = 1e-12 if shape == LP_SHAPES[0] else shape[0] * 2.0 ** -53 * want.max()
    print(f"lp_cols {shape}: worst absolute differences (sum |d|, sum d^2, max |d|) {err}, sums up to "
          f"{want.max():.4g}, gate {gate:.3g}")
    assert err.max() <= gate


@pytest.mark.parametrize("shape", NB_SHAPES, ids=_id)
def test_nb_divergences_matches_oracle(cuda, shape):
    got, want = _native_op("nb", shape, cuda).cpu().numpy(), _oracle("nb", shape)
    assert got.shape == (4,) and np.isfinite(want).all() and (want > 0).all()
    err = np.abs(got / want - 1.0).max()
    print(f"nb_divergences {shape}: {got / (shape[0] * shape[2])}, worst relative difference {err:.3e}")
    assert err <= 1e-10, (got, want)


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _evals(shape, cuda):
    real, fake = (a.copy() for a in _pair(shape))
    ds = np.random.RandomState(5).rand(64, shape[1], shape[2]).astype(np.float32)
    names = [f"f{i}" for i in range(shape[2])]
    return GANEval(real, fake, ds, names, ["m"]), GANEval(real, fake, ds, names, ["m"], device=cuda)


def test_gan_eval_device_matches_host(cuda):
    cpu, dev = _evals((700, 24, 32), cuda)
    a, b = cpu.ks_test(p_val_only=False), dev.ks_test(p_val_only=False)
    assert b.shape == (2,) and abs(a[0] - b[0]) <= 1e-12 and _rel(b[1], a[1]) <= 1e-9, (a, b)
    a, b = cpu.ks_test(group=False), dev.ks_test(group=False)
    assert b.shape == (32, 2) and np.abs(a.values[:, 0] - b.values[:, 0]).max() <= 1e-12
    assert _rel(b.values[:, 1], a.values[:, 1]) <= 1e-9
    assert _rel(dev.ks_test(), cpu.ks_test()) <= 1e-9
    a, b = cpu.ACF(group=False), dev.ACF(group=False)
    assert len(b) == 32 and np.isfinite(b).all() and np.abs(np.array(a) - np.array(b)).max() <= 1e-12
    assert abs(cpu.ACF() - dev.ACF()) <= 1e-12
    for ord_ in (1, 2, np.inf):
        a, b = cpu.lp_dist(ord=ord_, group=False), dev.lp_dist(ord=ord_, group=False)
        assert len(b) == 32 and _rel(b, a) <= 1e-5, (ord_, a, b)
        assert _rel(dev.lp_dist(ord=ord_), cpu.lp_dist(ord=ord_)) <= 1e-5
    assert dev.lp_dist(ord=3) == cpu.lp_dist(ord=3)  # any other order: the host formula
    for name in ("kl_div", "js_div"):
        a, b = getattr(cpu, name)(div_only=False), getattr(dev, name)(div_only=False)
        assert len(b) == 2 and np.isfinite(a).all() and _rel(b, a) <= 1e-9, (name, a, b)
        assert _rel(getattr(dev, name)(), getattr(cpu, name)()) <= 1e-9
    assert _rel(dev.Inception_score(), cpu.Inception_score()) <= 1e-9


def test_small_samples_take_the_exact_host_route(cuda, monkeypatch):
    cpu, dev = _evals((37, 24, 5), cuda)  # 888 rows <= 10 000: scipy's exact mode
    monkeypatch.setattr(Fn, "ks_stat", lambda *a: pytest.fail("ks_stat launched for a small sample"))
    assert np.array_equal(cpu.ks_test(p_val_only=False), dev.ks_test(p_val_only=False))
    assert cpu.ks_test(group=False).equals(dev.ks_test(group=False))


def test_one_upload_per_array_and_one_nb_launch(cuda, monkeypatch):
    _, dev = _evals((700, 24, 32), cuda)
    uploads, launches = [], []
    up, nb = gan_eval._upload, Fn.nb_divergences
    monkeypatch.setattr(gan_eval, "_upload", lambda a, d: (uploads.append(id(a)), up(a, d))[1])
    monkeypatch.setattr(Fn, "nb_divergences", lambda *a: (launches.append(1), nb(*a))[1])
    dev.kl_div(), dev.js_div(), dev.Inception_score(), dev.kl_div(div_only=False), dev.js_div(div_only=False)
    assert len(launches) == 1
    dev.ks_test(), dev.ACF(), dev.lp_dist(), dev.lp_dist(ord=1), dev.wasserstein(), dev.FID(), dev.linear_MMD()
    assert sorted(uploads) == sorted([id(dev.real), id(dev.fake)]), uploads
    other = _pair((700, 24, 32))[1].copy()  # an override is another array: its own upload and NB pass
    dev.kl_div(fake=other), dev.js_div(fake=other)
    assert len(launches) == 2 and len(uploads) == 3


def _all_ops(cuda):
    return [_native_op("ks", (40000, 3), cuda, True), _native_op("acf", (300, 48, 35), cuda),
            _native_op("lp", (300 * 48, 35), cuda), _native_op("nb", (300, 48, 35), cuda),
            _native_op("nb", (6, 168, 64), cuda)]


def test_two_runs_are_bitwise_identical(cuda):
    for a, b in zip(_all_ops(cuda), _all_ops(cuda)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_results_are_finite_under_the_debug_poison(cuda):
    ops = _native.native()
    prev = ops.set_debug_poison(True)
    try:
        outs = _all_ops(cuda) + [_native_op("ks", (16385, 3), cuda, True), _native_op("lp", (1001, 300), cuda)]
        for o in outs:
            assert bool(torch.isfinite(o).all()), o
    finally:
        ops.set_debug_poison(prev)


def test_argument_checks(cuda):
    ops = _native.native()
    z = lambda *s, **k: torch.zeros(*s, device=cuda, **k)  # noqa: E731
    n = (1 << 24) + 1
    with pytest.raises(RuntimeError, match="2\\^24"):
        ops.ks_stat(z(n, 1), z(1, n))
    with pytest.raises(RuntimeError, match="ref_sorted"):
        ops.ks_stat(z(100, 3), z(100, 3))
    with pytest.raises(RuntimeError):
        ops.ks_stat(z(3, 100).t(), z(3, 100))
    with pytest.raises(RuntimeError, match="LDS"):
        ops.acf_mean(z(2, 400, 100), 17)
    with pytest.raises(RuntimeError):
        ops.acf_mean(z(2, 24, 5), -1)
    with pytest.raises(RuntimeError, match="T <= 168"):
        ops.nb_divergences(z(2, 169, 5), z(2, 169, 5), z(5, 169, dtype=torch.float64), z(5, 169, dtype=torch.float64),
                           z(5, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="F <= 64"):
        ops.nb_divergences(z(2, 24, 65), z(2, 24, 65), z(65, 24, dtype=torch.float64), z(65, 24, dtype=torch.float64),
                           z(65, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="float64"):
        ops.nb_divergences(z(2, 24, 5), z(2, 24, 5), z(5, 24), z(5, 24), z(5))
    with pytest.raises(RuntimeError):
        ops.nb_divergences(z(2, 24, 5), z(2, 24, 5), z(5, 23, dtype=torch.float64), z(5, 23, dtype=torch.float64),
                           z(5, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.lp_cols(z(10, 3), z(10, 4))
    with pytest.raises(Exception):  # a CPU tensor has no kernel of these ops
        ops.lp_cols(torch.zeros(10, 3), torch.zeros(10, 3))
    assert not Fn.nb_divergences_supported(169, 5) and not Fn.acf_mean_supported(400, 100, 17)
