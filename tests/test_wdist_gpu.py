"""Device W-dist (csrc/wdist.hip) and its tracker on an MI355X (run with -m gpu).

The op against float64 scipy on the same fp32 / bf16-rounded values at the sizes where the kernels change
behaviour (below one wave, one full chunk of 16 384, one element into the second chunk, several chunks),
with continuous values and with 8-level samples whose equal values sit in different chunks; bitwise
repeatability; non-finite inputs; the argument checks; the ``GANEval`` device path; the tracker against
the CPU metric on ``GANTrainer.generate``; graph capture of ``update``; a run under ``graph=True``.
Every case runs with the debug poison on: an output, workspace or slab element that no kernel wrote is NaN.

Gate of the op: the kernel forms every |x - ref| and every sum in float64 from exactly the values scipy
sees, so the two differ by summation order only: <= n 2^-53 < 1.5e-11 relative for n <= 2^17; 1e-10.
"""
import numpy as np
import pytest
import torch
from scipy.stats import wasserstein_distance

from hfrep.data.windows import synthetic_windows
from hfrep.eval.gan_eval import GANEval
from hfrep.ops import _native
from hfrep.ops import functional as Fn
from hfrep.train.gan_trainer import GANConfig, GANTrainer
from hfrep.train.runner import RunOptions, run
from hfrep.train.wdist_tracker import WDistTracker

pytestmark = pytest.mark.gpu
GATE = 1e-10
SHAPES = [(1, 3), (2, 1), (63, 5), (64, 32), (65, 35), (16384, 4), (16385, 4), (48000, 35), (70001, 3)]
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}


@pytest.fixture(autouse=True)
def poison(cuda):
    ops = _native.native()
    prev = ops.set_debug_poison(True)
    try:
        yield
    finally:
        ops.set_debug_poison(prev)


def _quantise(a):
    """8 levels k / 8 (exact in bf16): every value ties with about an eighth of the sample."""
    return torch.floor(torch.clamp((a + 2.0) / 4.0, 0.0, 0.999) * 8.0) / 8.0


def _sample(n, F, dtype, quantised, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, F, generator=g)
    y = torch.randn(n, F, generator=g) * 1.25 + 0.1
    if quantised:
        x, y = _quantise(x), _quantise(y)
    return x.to(dtype), y


def _scipy(x, y, cols=None):
    """float64 scipy on the values the kernel sees: per-feature W1 and the mean."""
    xv, yv = x.float().cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
    cols = range(xv.shape[1]) if cols is None else cols
    w = np.array([wasserstein_distance(yv[:, i], xv[:, i]) for i in cols])
    return w, float(np.mean(w))


def _sorted_ref(y, dev):
    return torch.sort(y.to(dev).t().contiguous(), dim=1).values.contiguous()


def _rel(got, want):
    return abs(got - want) / max(abs(want), 1e-300) if want != 0 else abs(got)


@pytest.mark.parametrize("quantised", [False, True], ids=["continuous", "levels8"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_op_matches_scipy(cuda, shape, dtype, quantised):
    n, F = shape
    x, y = _sample(n, F, DTYPES[dtype], quantised, seed=n + F)
    out = Fn.wdist(x.to(cuda), _sorted_ref(y, cuda))
    assert out.dtype == torch.float64 and tuple(out.shape) == (F + 1,)
    got = out.cpu().numpy()
    w, mean = _scipy(x, y)
    worst = max([_rel(got[i], w[i]) for i in range(F)] + [_rel(got[F], mean)])
    print(f"wdist {n}x{F} {dtype} quantised={quantised}: worst relative difference {worst:.3e}")
    assert np.isfinite(got).all() and worst <= GATE, (worst, got, w)


def test_two_calls_are_bitwise_identical(cuda):
    x, y = _sample(48000, 35, torch.float32, False, seed=9)
    xd, ref = x.to(cuda), _sorted_ref(y, cuda)
    a = Fn.wdist(xd, ref)
    b = Fn.wdist(xd, ref)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_non_finite_columns_stay_in_their_columns(cuda, dtype):
    n, F = 16385, 4
    x, y = _sample(n, F, DTYPES[dtype], False, seed=21)
    x[5, 1] = x[9000, 1] = x[n - 1, 1] = float("inf")  # +inf in both chunks, beside the first chunk's pads
    x[16384, 2] = float("nan")                         # the second chunk's only element
    buf = torch.full(((n + 64) * F,), float("nan"), dtype=DTYPES[dtype], device=cuda)
    xd = buf[17 * F:(17 + n) * F].view(n, F)           # a read before or past x finds NaN
    xd.copy_(x)
    got = Fn.wdist(xd, _sorted_ref(y, cuda)).cpu().numpy()
    w, _ = _scipy(x, y, cols=[0, 3])
    for i, want in zip([0, 3], w):
        assert np.isfinite(got[i]) and _rel(got[i], want) <= GATE, (i, got[i], want)
    assert got[1] == np.inf and np.isnan(got[2]) and not np.isfinite(got[F])


def test_argument_checks(cuda):
    ops = _native.native()
    n = (1 << 20) + 1
    with pytest.raises(RuntimeError, match="2\\^20"):
        ops.wdist_sorted(torch.zeros(n, 1, device=cuda), torch.zeros(1, n, device=cuda))
    x = torch.zeros(100, 3, device=cuda)
    with pytest.raises(RuntimeError, match="ref_sorted"):
        ops.wdist_sorted(x, torch.zeros(100, 3, device=cuda))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.wdist_sorted(torch.zeros(3, 100, device=cuda).t(), torch.zeros(3, 100, device=cuda))
    with pytest.raises(RuntimeError):
        ops.wdist_sorted(x.double(), torch.zeros(3, 100, device=cuda))
    with pytest.raises(RuntimeError):
        ops.wdist_sorted(x, torch.zeros(3, 100, device=cuda, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        ops.wdist_sorted(torch.zeros(0, 3, device=cuda), torch.zeros(3, 0, device=cuda))
    with pytest.raises(Exception):  # a CPU tensor has no kernel of this op
        ops.wdist_sorted(x.cpu(), torch.zeros(3, 100))


def test_gan_eval_device_path(cuda):
    real = synthetic_windows(400, 24, 32, seed=1)
    fake = (synthetic_windows(400, 24, 32, seed=2) * 0.9 + 0.05).astype(np.float32)
    names = [f"f{i}" for i in range(32)]
    cpu = GANEval(real, fake, real, names, ["m"])
    dev = GANEval(real, fake, real, names, ["m"], device=cuda)
    a, b = cpu.wasserstein(), dev.wasserstein()
    assert isinstance(b, float) and _rel(b, a) <= 1e-6, (a, b)
    pa, pb = cpu.wasserstein(group=False), dev.wasserstein(group=False)
    assert len(pb) == 32 and max(_rel(q, p) for p, q in zip(pa, pb)) <= 1e-6


def _trainer(cuda, arch, dtype):
    ds = synthetic_windows(64, 24, 32, seed=3)
    cfg = GANConfig(arch=arch, loss="wgan_gp", window=24, features=32, batch_size=16, dtype=dtype, seed=11)
    return GANTrainer(cfg, ds, device=cuda)


def _hold():
    return synthetic_windows(64, 24, 32, seed=1011)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("arch", ["mlp", "lstm"])
def test_tracker_matches_the_cpu_metric_and_leaves_training_alone(cuda, arch, dtype):
    hold = _hold()
    tr = _trainer(cuda, arch, dtype)
    tk = WDistTracker(tr, hold)
    gate = 1e-5 if dtype == "float32" else 2e-2
    seen = []
    for it in range(1, 5):
        tr.train_step()
        tk.update(it)
        got = tk.values()
        fake = tr.generate(64, seed=tr.cfg.seed + 7)
        want = GANEval(hold, fake, hold, [f"f{i}" for i in range(32)], ["m"]).wasserstein()
        print(f"tracker {arch} {dtype} iteration {it}: {got['w_dist']:.9g} vs CPU {want:.9g}")
        assert _rel(got["w_dist"], want) <= gate, (it, got, want)
        seen.append(got["w_dist"])
        assert got["w_best"] == min(seen) and got["w_best_iteration"] == 1 + int(np.argmin(seen))
    plain = _trainer(cuda, arch, dtype)
    for _ in range(4):
        plain.train_step()
    torch.cuda.synchronize()
    assert torch.equal(tr.generator.flat, plain.generator.flat) and torch.equal(tr.critic.flat, plain.critic.flat)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_update_is_graph_capturable(cuda, dtype):
    """No host synchronise, no host read: ``update`` captures on one stream, and a replay evaluates the
    weights the generator holds THEN."""
    tr = _trainer(cuda, "lstm", dtype)
    tk = WDistTracker(tr, _hold())
    fresh = {k: v.clone() for k, v in tk.state_dict().items()}
    tk.update(1)
    tk.update(2)
    before = tk.values()["w_dist"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tk.update(7)
    with torch.no_grad():
        tr.generator.flat.mul_(1.25)
    tk.load_state_dict(fresh)
    g.replay()
    torch.cuda.synchronize()
    replayed, best = tk.values(), tk.best_flat.clone()
    tk.load_state_dict(fresh)
    tk.update(7)
    eager = tk.values()
    assert replayed == eager and replayed["w_best_iteration"] == 7 and replayed["w_dist"] != before
    assert torch.equal(best, tk.best_flat) and torch.equal(best, tr.generator.flat.detach())


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_run_under_graph_replay_logs_the_eager_values(cuda, dtype):
    hold = _hold()
    recs = {}
    for graph in (False, True):
        tr = _trainer(cuda, "lstm", dtype)
        recs[graph] = run(tr, RunOptions(epochs=6, log_every=1, echo=False, graph=graph, wdist_every=2, wdist_real=hold))
    for a, b in zip(recs[False], recs[True]):
        assert a["iteration"] == b["iteration"]
        for k in ("w_dist", "w_best", "w_best_iteration"):
            assert a[k] == b[k], (k, a, b)  # (None before the first evaluation)
    assert np.isfinite(recs[True][-1]["w_dist"]) and recs[True][-1]["w_best_iteration"] in (2, 4, 6)
