"""Direct causal conv1d kernels (csrc/conv1d.hip) on an MI355X: every op against fp64 on the CPU, row by
row, and against the im2col route; the launcher's other paths, accumulation, bitwise repeats, debug poison, the
("conv", "wgan_gp") trainer on both routes and under graph replay, a declined shape, and peak memory against
the im2col route.

fp64 references come from ``R.conv1d_causal`` and its autograd gradients on inputs rounded to the compute
dtype.  Bounds: ``test_kernels_gpu._close`` (``TOL``) on the whole tensor, the same bound on every (b, t)
row with the row's own scale (floored at the mean row scale: a leak into a few rows cannot hide under a
global maximum), and at most twice the im2col route's own error against fp64."""
import numpy as np
import pytest
import torch

from _blocks import BF16_GLOBAL, VANISHED, assert_blocks_close, block_errors, cpu_twin, wasserstein_half_scales
from hfrep.ops import functional as Fn
from hfrep.ops import reference as R

pytestmark = pytest.mark.gpu

TOL = {torch.float32: dict(rtol=2e-4, atol=2e-5), torch.bfloat16: dict(rtol=5e-2, atol=3e-2)}  # test_kernels_gpu.TOL

# (B, T, C_in, C_out, k, dil)
SHAPES = [(3, 5, 32, 100, 3, 2),      # halo 4 of T = 5: masked taps almost everywhere, sample boundaries inside a tile
          (1, 1, 32, 100, 3, 1),      # T = 1: only the last tap exists
          (2, 7, 32, 100, 4, 3),      # halo 9 > T: some taps never contribute
          (4, 24, 36, 100, 1, 1),     # k = 1: a Dense layer
          (37, 24, 32, 100, 3, 1),    # 888 rows: a partial last row tile
          (5, 48, 100, 100, 3, 2),    # the second layer
          (2, 168, 36, 100, 3, 2),    # the production window
          (700, 24, 32, 100, 3, 2)]   # 16 800 rows: several workgroups, the weight gradient's slab reduce
BIG = SHAPES[-1]
DTS = [torch.float32, torch.bfloat16]


def _bound(s, dt):
    t = TOL[dt]
    return t["atol"] * max(1.0, s) + t["rtol"] * s


def _err(got, ref):
    return (got.double().cpu() - ref).abs().max().item()


def _close(got, ref, dt, scale=None, what=""):
    s = scale if scale is not None else max(ref.abs().max().item(), 1e-3)
    err = _err(got, ref)
    print(f"{what}: max err {err:.3e} (scale {s:.3e}, bound {_bound(s, dt):.3e})")
    assert err <= _bound(s, dt), f"{what}: max err {err:.3e} (scale {s:.3e})"


def _rows_close(got, ref, dt, what=""):
    """Every (b, t) row against the ``_close`` bound at the row's own scale, floored at the mean row scale."""
    got = got.double().cpu()
    s = ref.abs().amax(-1)
    s = torch.maximum(s, s.mean().clamp_min(1e-3))
    t = TOL[dt]
    bound = t["atol"] * s.clamp_min(1.0) + t["rtol"] * s
    err = (got - ref).abs().amax(-1)
    worst = (err / bound).max().item()
    print(f"{what}: worst row error {worst:.3e} of its bound")
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} rows outside their bound, first (b, t) = {bad[0].tolist()}, " \
                             f"err {err[tuple(bad[0])]:.3e} bound {bound[tuple(bad[0])]:.3e}"


def _inputs(shape, dt, seed=0):
    """Random inputs as test_linear's; the last (k-1) dil steps of every sample of x and the first of dz are
    scaled by 8: own-sample terms are in the reference, a read from the neighbouring sample is not."""
    B, T, Cin, Cout, k, dil = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, Cin, generator=g) * 0.5
    W = torch.randn(k, Cin, Cout, generator=g) * (1.0 / (k * Cin) ** 0.5)
    b = torch.randn(Cout, generator=g) * 0.1
    dz = torch.randn(B, T, Cout, generator=g) * 0.1
    h = min((k - 1) * dil, T)
    if h:
        x[:, T - h:] *= 8
        dz[:, :h] *= 8
    return x.to(dt), W, b, dz.to(dt)


_REF = {}


def _reference(shape, dt):
    """fp64 (y with bias and LeakyReLU, dx, gW, gb) of the inputs of ``_inputs``; computed once per case."""
    key = (shape, dt)
    if key not in _REF:
        x, W, b, dz = _inputs(shape, dt)
        dil = shape[5]
        xr, Wr, br = (t.double().requires_grad_(True) for t in (x, W, b))
        z = R.conv1d_causal(xr, Wr, br, None, dil)
        dx, gW, gb = torch.autograd.grad(z, (xr, Wr, br), dz.double())
        # scale of the weight gradient's sum: |x|^T |dz| per tap (test_wgrad's)
        Wa = torch.ones_like(W, dtype=torch.float64, requires_grad=True)
        sW, = torch.autograd.grad(R.conv1d_causal(x.double().abs(), Wa, None, None, dil), Wa, dz.double().abs())
        _REF[key] = (R.apply_act(z.detach(), 3), dx, gW, gb, sW.max().item(), dz.double().abs().sum((0, 1)).max().item())
    return _REF[key]


def _ops():
    from hfrep.ops import _native

    return _native.native()


def _run(shape, dt, cuda, gW0=None, gb0=None):
    """(y, dx, gW, gb) on the GPU, on whichever route the environment selects: ``Fn.conv1d_fwd`` / ``conv1d_dgrad``,
    and for the weight gradient the direct op itself on the direct route (``Fn.conv1d_wgrad_`` keeps bf16 on
    im2col + GEMM there, which the trainer tests cover)."""
    x, W, b, dz = _inputs(shape, dt)
    B, T, Cin, Cout, k, dil = shape
    xg, Wg, bg, dzg = x.to(cuda), W.to(cuda), b.to(cuda), dz.to(cuda)
    y = Fn.conv1d_fwd(xg, Wg, bg, 3, dil)
    dx = Fn.conv1d_dgrad(dzg, Wg, dil)
    gW = (torch.zeros(k, Cin, Cout) if gW0 is None else gW0.clone()).to(cuda)
    gb = (torch.zeros(Cout) if gb0 is None else gb0.clone()).to(cuda)
    if Fn.conv1d_direct(xg, Wg, dil):  # the op itself: Fn.conv1d_wgrad_ keeps bf16 on the unfolded route
        _ops().conv1d_causal_wgrad_(xg, dzg, gW, gb, dil)
    else:
        Fn.conv1d_wgrad_(xg, dzg, gW, gb, dil)
    torch.cuda.synchronize()
    return y, dx, gW, gb


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_conv1d_ops_vs_fp64(cuda, shape, dt, monkeypatch):
    B, T, Cin, Cout, k, dil = shape
    monkeypatch.delenv("HFREP_CONV_DIRECT", raising=False)
    x, W, b, dz = _inputs(shape, dt)
    assert Fn.conv1d_direct(x.to(cuda), W.to(cuda), dil), "the direct kernels must take this shape"
    ry, rdx, rgW, rgb, sW, sb = _reference(shape, dt)
    y, dx, gW, gb = _run(shape, dt, cuda)
    assert y.dtype == dt and dx.dtype == dt and y.shape == (B, T, Cout) and dx.shape == (B, T, Cin)
    tag = f"{shape} {dt}"
    _close(y, ry, dt, what=f"{tag} y")
    _rows_close(y, ry, dt, what=f"{tag} y")
    _close(dx, rdx, dt, what=f"{tag} dx")
    _rows_close(dx, rdx, dt, what=f"{tag} dx")
    _close(gW, rgW, dt, scale=sW, what=f"{tag} gW")
    _close(gb, rgb, dt, scale=sb, what=f"{tag} gb")
    if k == 1:  # a Dense layer: the same numbers as linear, to the bound
        lin = Fn.linear(x.to(cuda), W[0].to(cuda), b.to(cuda), 3)
        _close(y, lin.double().cpu(), dt, what=f"{tag} y vs linear")
    # at most twice the im2col route's error against fp64, floored at the _close bound
    monkeypatch.setenv("HFREP_CONV_DIRECT", "0")
    assert not Fn.conv1d_direct(x.to(cuda), W.to(cuda), dil)
    y0, dx0, gW0, gb0 = _run(shape, dt, cuda)
    for name, got, old, ref, s in (("y", y, y0, ry, None), ("dx", dx, dx0, rdx, None), ("gW", gW, gW0, rgW, sW),
                                   ("gb", gb, gb0, rgb, sb)):
        s = s if s is not None else max(ref.abs().max().item(), 1e-3)
        e, e0 = _err(got, ref), _err(old, ref)
        print(f"{tag} {name}: direct {e:.3e}, im2col {e0:.3e}")
        assert e <= max(2.0 * e0, _bound(s, dt)), f"{tag} {name}: direct {e:.3e} vs im2col {e0:.3e}"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(2, 9, 100, 100, 4, 2),      # fp32: four taps of 100 x 100 exceed LDS, two launches
                                   (1, 120, 100, 100, 3, 30),   # fp32: a halo of 60 rows beside 120 KB of weights: staged per tap
                                   (3, 40, 128, 128, 2, 5)])    # the widest channels: full 32-column tiles
def test_conv1d_other_kernel_paths(cuda, shape, dt, monkeypatch):
    """Shapes at which the forward / input-gradient launcher takes its other paths."""
    monkeypatch.delenv("HFREP_CONV_DIRECT", raising=False)
    B, T, Cin, Cout, k, dil = shape
    x, W, b, dz = _inputs(shape, dt)
    assert Fn.conv1d_direct(x.to(cuda), W.to(cuda), dil)
    ry, rdx, rgW, rgb, sW, sb = _reference(shape, dt)
    y, dx, gW, gb = _run(shape, dt, cuda)
    tag = f"{shape} {dt}"
    _close(y, ry, dt, what=f"{tag} y")
    _rows_close(y, ry, dt, what=f"{tag} y")
    _close(dx, rdx, dt, what=f"{tag} dx")
    _rows_close(dx, rdx, dt, what=f"{tag} dx")
    _close(gW, rgW, dt, scale=sW, what=f"{tag} gW")
    _close(gb, rgb, dt, scale=sb, what=f"{tag} gb")


@pytest.mark.parametrize("dt", DTS)
def test_conv1d_no_bias_linear_act(cuda, dt):
    """bias = None and act = linear (the tangent forward's call), gb = None (the tangent reverse's)."""
    shape = SHAPES[0]
    B, T, Cin, Cout, k, dil = shape
    x, W, b, dz = _inputs(shape, dt)
    y = Fn.conv1d_fwd(x.to(cuda), W.to(cuda), None, 0, dil)
    ref = R.conv1d_causal(x.double(), W.double(), None, None, dil)
    _close(y, ref, dt, what="no bias y")
    _rows_close(y, ref, dt, what="no bias y")
    gW = torch.zeros(k, Cin, Cout, device=cuda)
    _ops().conv1d_causal_wgrad_(x.to(cuda), dz.to(cuda), gW, None, dil)
    _, _, rgW, _, sW, _ = _reference(shape, dt)
    _close(gW, rgW, dt, scale=sW, what="no bias gW")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[5]])
def test_conv1d_wgrad_accumulates(cuda, shape, dt):
    B, T, Cin, Cout, k, dil = shape
    g = torch.Generator().manual_seed(3)
    gW0, gb0 = torch.randn(k, Cin, Cout, generator=g), torch.randn(Cout, generator=g)
    _, _, rgW, rgb, sW, sb = _reference(shape, dt)
    _, _, gW, gb = _run(shape, dt, cuda, gW0, gb0)
    _close(gW, gW0.double() + rgW, dt, scale=sW, what="accumulated gW")
    _close(gb, gb0.double() + rgb, dt, scale=sb, what="accumulated gb")


@pytest.mark.parametrize("dt", DTS)
def test_conv1d_bitwise_repeat_and_side_stream(cuda, dt):
    a = _run(BIG, dt, cuda)
    b = _run(BIG, dt, cuda)
    for name, u, v in zip(("y", "dx", "gW", "gb"), a, b):
        assert torch.equal(u, v), f"{name} differs between two runs"
    x, W, _, dz = _inputs(BIG, dt)
    B, T, Cin, Cout, k, dil = BIG
    xg, dzg = x.to(cuda), dz.to(cuda)
    gW, gb = torch.zeros(k, Cin, Cout, device=cuda), torch.zeros(Cout, device=cuda)
    side = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _ops().conv1d_causal_wgrad_(xg, dzg, gW, gb, dil)
    side.synchronize()
    assert torch.equal(gW, a[2]) and torch.equal(gb, a[3]), "the weight gradient depends on the stream"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]])
def test_conv1d_poison(cuda, shape, dt):
    """Outputs and workspaces allocated full of NaN: every element the ops return is written."""
    clean = _run(shape, dt, cuda)
    ops = _ops()
    prev = ops.set_debug_poison(True)
    try:
        got = _run(shape, dt, cuda)
    finally:
        ops.set_debug_poison(prev)
    for name, u, v in zip(("y", "dx", "gW", "gb"), got, clean):
        assert bool(torch.isfinite(u).all()), f"{name} has unwritten elements"
        assert torch.equal(u, v), f"{name} differs under poison"


def _trainer(cuda, dtype, B=37, T=24, F=32, seed_ds=0):
    from hfrep.train.gan_trainer import GANConfig, GANTrainer

    ds = np.random.RandomState(seed_ds).rand(64, T, F).astype(np.float32)
    return GANTrainer(GANConfig(arch="conv", loss="wgan_gp", window=T, features=F, batch_size=B, dtype=dtype), ds,
                      device=cuda)


def _assert_route(tr, x, direct):
    """Which route a conv layer's saved context shows: no ``cols`` and no tensor of k C_in columns on the direct one."""
    layer = tr.critic.layers[0]
    with torch.no_grad():
        _, ctx = layer.efwd(x, save=True)
    wide = [n for n, t in ctx.items() if torch.is_tensor(t) and t.shape[-1] == layer.k * layer.cin]
    assert ("cols" in ctx) == (not direct) and bool(wide) == (not direct), (sorted(ctx), wide)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("direct", [True, False])
def test_conv_trainer_gradients_both_routes(cuda, dtype, direct, monkeypatch):
    """The critic GP gradient and the generator gradient of ("conv", "wgan_gp") at B = 37, block by block against
    the fp64 CPU twin, with the bounds of test_trainer_gradients_gpu_vs_cpu / test_trainer_gradients_bf16_conv."""
    key, B, T, F = ("conv", "wgan_gp"), 37, 24, 32
    monkeypatch.setenv("HFREP_CONV_DIRECT", "1" if direct else "0")
    tg = _trainer(cuda, dtype)
    dt = tg.dtype
    tc = cpu_twin(tg, "float64")
    tb = cpu_twin(tg, "bfloat16") if dtype == "bfloat16" else None
    g = torch.Generator().manual_seed(11)
    real = torch.rand(B, T, F, generator=g).to(dt)
    noise = torch.randn(B, T, F, generator=g).to(dt)
    alpha = torch.rand(B, generator=g)
    _assert_route(tg, real.to(cuda), direct)
    with torch.no_grad():
        fg = tg.generator.predict(noise.to(cuda))
        scales = wasserstein_half_scales(tc, real.double(), VANISHED[key])
        tg.critic_gp_grads(real.to(cuda), fg, alpha.to(cuda))
        tc.critic_gp_grads(real.double(), fg.double().cpu(), alpha.double())
        if tb is not None:
            tb.critic_gp_grads(real, fg.cpu(), alpha)
        assert_blocks_close(tg.critic, tc.critic, dtype, VANISHED[key], scales, f"conv {dtype} critic",
                            flat_tol=2e-4 if dtype == "float32" else BF16_GLOBAL, model_cpu=tb.critic if tb else None)
        lg = tg.generator_grads(noise.to(cuda))
        lc = tc.generator_grads(noise.double())
        if tb is None:
            assert_blocks_close(tg.generator, tc.generator, dtype, label="conv float32 generator", flat_tol=2e-4)
            assert abs(lg.item() - lc.item()) < 1e-4 * max(1, abs(lc.item()))
        else:
            tb.generator_grads(noise)
            e_cpu = block_errors(tb.generator, tc.generator)[0]
            assert_blocks_close(tg.generator, tc.generator, dtype, label="conv bf16 generator",
                                flat_tol=max(BF16_GLOBAL, 2.0 * e_cpu), model_cpu=tb.generator)


def test_conv_trainer_bitwise_and_route_parity(cuda, monkeypatch):
    """Three training iterations: two direct runs are bitwise identical, and the direct run stays within 1e-4
    (relative, parameters) of the im2col route on the same RNG stream (fp32)."""
    def run(direct):
        monkeypatch.setenv("HFREP_CONV_DIRECT", "1" if direct else "0")
        tr = _trainer(cuda, "float32", seed_ds=1)
        for _ in range(3):
            tr.train_step()
        torch.cuda.synchronize()
        return tr

    a, b, e = run(True), run(True), run(False)
    assert torch.equal(a.critic.flat, b.critic.flat) and torch.equal(a.generator.flat, b.generator.flat)
    for m in ("critic", "generator"):
        pa, pe = getattr(a, m).flat.double().cpu(), getattr(e, m).flat.double().cpu()
        rel = ((pa - pe).norm() / max(pe.norm().item(), 1e-30)).item()
        print(f"{m}: direct vs im2col route parameters rel {rel:.3e}")
        assert rel < 1e-4, f"{m} params drift from the im2col route: {rel:.2e}"


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_conv_graph_replay_matches_eager(cuda, dtype, monkeypatch):
    """The whole ("conv", "wgan_gp") iteration on the direct kernels captures into a hipGraph, and five replayed
    iterations equal five eager ones bit for bit (tests/test_gpu_runtime.py's check, on this model)."""
    from hfrep.train.runner import GraphedStep

    monkeypatch.delenv("HFREP_CONV_DIRECT", raising=False)
    eager, graphed = _trainer(cuda, dtype, seed_ds=2), _trainer(cuda, dtype, seed_ds=2)
    for _ in range(5):
        eager.train_step()
    step = GraphedStep(graphed, warmup=2)  # 2 eager steps, capture, then replays
    for _ in range(5):
        step()
    assert step.graph is not None
    torch.cuda.synchronize()
    assert graphed.iteration == eager.iteration == 5
    assert torch.equal(graphed.generator.flat, eager.generator.flat)
    assert torch.equal(graphed.critic.flat, eager.critic.flat)


@pytest.mark.parametrize("dt", DTS)
def test_conv1d_declined_shape_runs_im2col(cuda, dt, monkeypatch):
    """C_out = 50 has no direct kernel: the functions run im2col + GEMM + col2im, to their usual bounds."""
    monkeypatch.delenv("HFREP_CONV_DIRECT", raising=False)
    shape = (5, 17, 32, 50, 3, 2)
    B, T, Cin, Cout, k, dil = shape
    assert not _ops().conv1d_supported(Cin, Cout, k, dil, dt)
    x, W, b, dz = _inputs(shape, dt)
    assert not Fn.conv1d_direct(x.to(cuda), W.to(cuda), dil)
    ry, rdx, rgW, rgb, sW, sb = _reference(shape, dt)
    y, dx, gW, gb = _run(shape, dt, cuda)
    _close(y, ry, dt, what="declined y")
    _close(dx, rdx, dt, what="declined dx")
    _close(gW, rgW, dt, scale=sW, what="declined gW")
    _close(gb, rgb, dt, scale=sb, what="declined gb")
    with pytest.raises(RuntimeError):  # the op itself refuses: a missing kernel is an error, not a fallback
        _ops().conv1d_causal_fwd(x.to(cuda), W.to(cuda), b.to(cuda), dil, 3)


def test_conv_critic_peak_memory_below_im2col(cuda, monkeypatch):
    """One critic_gp_grads at B = 4096, T = 24, F = 32 (fp32): the direct route's peak allocation is lower."""
    B, T, F = 4096, 24, 32
    g = torch.Generator().manual_seed(5)
    real = torch.rand(B, T, F, generator=g).to(cuda)
    noise = torch.randn(B, T, F, generator=g).to(cuda)
    alpha = torch.rand(B, generator=g).to(cuda)
    peak = {}
    for direct in (True, False):
        monkeypatch.setenv("HFREP_CONV_DIRECT", "1" if direct else "0")
        tr = _trainer(cuda, "float32", B=B)
        with torch.no_grad():
            fake = tr.generator.predict(noise)
            tr.critic_gp_grads(real, fake, alpha)  # (first call: one-time allocations)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(cuda)
            tr.critic_gp_grads(real, fake, alpha)
            torch.cuda.synchronize()
        peak[direct] = torch.cuda.max_memory_allocated(cuda)
        del tr, fake
    print(f"peak bytes: direct {peak[True]}, im2col {peak[False]}")
    assert peak[True] < peak[False], peak
