"""Fused WGAN-GP step of the LReLU + LayerNorm MLP critic, zoo ``("mlp_ln", "wgan_gp")`` (csrc/mlp_*.hip
mlp_lngp_norm / mlp_lngp_critic, train/mlp_fused.py head 3) vs the CPU fp64 explicit engine and the GPU engine
path.

One critic update is W(real, -1) + W(fake, +1) + lambda GP(x_hat) on the per-row critic Dense -> LReLU -> LN
-> Dense -> LReLU -> LN -> Dense(1); its penalty gradient is a reverse over the tangent through both
LayerNorms.  The oracle is ``GANTrainer.critic_gp_grads`` in fp64 on the CPU (itself pinned against autograd
double backward by tests/test_engine.py).  Bound of every gradient comparison: max(TOL, 2 E), TOL the
project's fused-MLP tolerance (2e-4 fp32 / 3e-2 bf16, tests/test_mlp_fused_gpu.py) and E the error of the GPU
engine path (HFREP_MLP_FUSED=0, same weights and inputs) against the same oracle, measured in the test; the
factor 2 is the project's rule for its split-precision kernels.
"""
import numpy as np
import pytest
import torch

from _blocks import VANISHED, assert_blocks_close, cpu_twin, wasserstein_half_scales

pytestmark = pytest.mark.gpu

TOL = {"float32": 2e-4, "bfloat16": 3e-2}
LTOL = {"float32": 1e-4, "bfloat16": 2e-2}
CRITIC_NAMES = ["W1", "b1", "gamma1", "beta1", "W2", "b2", "gamma2", "beta2", "w3", "b3"]
SHAPES = [(48, 24, 32), (37, 24, 32), (20, 48, 36), (6000, 24, 32)]


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / max(ref.norm().item(), 1e-30)).item()


def _cfg(dtype, B, T=24, F=32, **kw):
    from hfrep.train.gan_trainer import GANConfig

    return GANConfig(arch="mlp_ln", loss="wgan_gp", window=T, features=F, batch_size=B, dtype=dtype, **kw)


def _trio(cuda, dtype, B, T, F, monkeypatch, **kw):
    """(fused GPU trainer, engine GPU trainer, fp64 CPU trainer) with the same weights; LayerNorm gamma and
    beta spread off their (1, 0) initial values (gamma enters every adjoint)."""
    from hfrep.train.gan_trainer import GANTrainer

    ds = np.random.RandomState(0).rand(64, T, F).astype(np.float32)
    monkeypatch.delenv("HFREP_MLP_FUSED", raising=False)
    tg = GANTrainer(_cfg(dtype, B, T, F, **kw), ds, device=cuda)
    assert tg._fused is not None and tg._fused.head == 3, "the fused MLP path must be selected on the GPU"
    monkeypatch.setenv("HFREP_MLP_FUSED", "0")
    te = GANTrainer(_cfg(dtype, B, T, F, **kw), ds, device=cuda)
    assert te._fused is None
    monkeypatch.delenv("HFREP_MLP_FUSED")
    tc = GANTrainer(_cfg("float64", B, T, F, **kw), ds, param_dtype=torch.float64)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for v in (tg._fused.cw[2], tg._fused.cw[6]):
            v.add_((0.2 * torch.randn(v.shape, generator=g)).to(v))
        for v in (tg._fused.cw[3], tg._fused.cw[7]):
            v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v))
        for t in (te, tc):
            t.generator.flat.copy_(tg.generator.flat.to(t.generator.flat))
            t.critic.flat.copy_(tg.critic.flat.to(t.critic.flat))
    return tg, te, tc


def _inputs(B, T, F, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, T, F, generator=g), torch.randn(B, T, F, generator=g), torch.rand(B, generator=g)


def _views(model):
    return [model.gview(l, s.name) for l in model.layers for s in l.specs]


def _critic_update(tag, tg, te, tc, real, fake, alpha, dtype):
    """One critic update's gradients and loss pack on the three trainers; asserts the fused path within
    max(TOL, 2 E) of the fp64 oracle, the views W1 ... w3 non-zero each on its own (a missed slab segment or
    operand cannot hide in the flat norm) and the loss pack within LTOL.  Returns the oracle's pack.

    beta2 and b3 are the exceptions to "non-zero": their true gradient in a whole update is 0 (the score is
    s = u2 . w3 + b3 with u2 = gamma2 xh2 + beta2, so both get sum_r ds_r times a constant, and the W terms'
    ds = -1/M on the real rows and +1/M on the fake rows sum to zero; the penalty's tangent sees neither).
    The fp64 oracle gives 8e-17 for them.  They are held to |g| <= TOL instead, and to the per-block rule
    for vanished blocks.

    Every other view is held to the per-block bound on its own (tests/_blocks.py: 2e-4 fp32; bf16
    max(5e-2, 2 e_cpu), e_cpu the CPU bf16 engine's error on the block where the batch is small)."""
    cuda, dt = tg.device, tg.dtype
    for t in (tg, te, tc):
        t.critic.zero_grad()
    rg, fg, ag = real.to(cuda, dt), fake.to(cuda, dt), alpha.to(cuda)
    van = VANISHED["mlp_ln", "wgan_gp"]
    scales = wasserstein_half_scales(tc, rg.double().cpu(), van)
    tb = cpu_twin(tg, "bfloat16") if dtype == "bfloat16" and real.shape[0] <= 64 else None
    if tb is not None:
        tb.critic_gp_grads(rg.cpu(), fg.cpu(), alpha)
    pack = tg._fused._lngp_critic_grads(rg, fg, ag)
    pack_e = te.critic_gp_grads(rg, fg, ag)
    # the oracle sees the inputs the GPU paths see (bf16-rounded where the run is bf16)
    ref = tc.critic_gp_grads(rg.double().cpu(), fg.double().cpu(), alpha.double())
    torch.cuda.synchronize()
    err = _rel(tg.critic.flat.grad, tc.critic.flat.grad)
    eng = _rel(te.critic.flat.grad, tc.critic.flat.grad)
    bound = max(TOL[dtype], 2.0 * eng)
    print(f"[{tag}] critic flat rel: fused {err:.3e} engine {eng:.3e} bound {bound:.3e}")
    for name, got, ge, rv in zip(CRITIC_NAMES, tg._fused.cg, _views(te.critic), _views(tc.critic)):
        print(f"    {name}: fused rel {_rel(got, rv):.3e} engine rel {_rel(ge, rv):.3e} |ref| {rv.norm().item():.3e}")
    print(f"    pack fused {[round(v, 6) for v in pack.tolist()]} engine {[round(v, 6) for v in pack_e.tolist()]} "
          f"ref {[round(v, 6) for v in ref.tolist()]}")
    assert err <= bound, f"critic grad rel err {err:.2e} > {bound:.2e} ({tag})"
    assert_blocks_close(tg.critic, tc.critic, dtype, van, scales, f"mlp_ln {tag} critic",
                        model_cpu=tb.critic if tb else None)
    for i in (0, 1, 2, 3, 4, 5, 6, 8):
        assert tg._fused.cg[i].abs().sum().item() > 0, f"critic gradient {CRITIC_NAMES[i]} is all zero ({tag})"
    for i in (7, 9):
        assert tg._fused.cg[i].abs().max().item() <= TOL[dtype], (CRITIC_NAMES[i], tg._fused.cg[i])
    for i in range(4):
        r = ref[i].item()
        assert abs(pack[i].item() - r) <= LTOL[dtype] * max(1.0, abs(r)), (i, pack.tolist(), ref.tolist())
    return ref


def test_mlp_ln_gp_fused_is_selected(cuda, monkeypatch):
    """The model runs the fused path on a GPU by default with head 3; HFREP_MLP_FUSED=0 keeps the engine."""
    from hfrep.train.gan_trainer import GANTrainer

    ds = np.random.RandomState(0).rand(64, 24, 32).astype(np.float32)
    monkeypatch.delenv("HFREP_MLP_FUSED", raising=False)
    tr = GANTrainer(_cfg("float32", 16), ds, device=cuda)
    assert tr._fused is not None and tr._fused.head == 3
    assert hasattr(torch.ops.hfrep, "mlp_lngp_norm") and hasattr(torch.ops.hfrep, "mlp_lngp_critic")
    monkeypatch.setenv("HFREP_MLP_FUSED", "0")
    assert GANTrainer(_cfg("float32", 16), ds, device=cuda)._fused is None


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("B,T,F", SHAPES)
def test_mlp_ln_gp_fused_grads(cuda, dtype, B, T, F, monkeypatch):
    """A whole critic update (W terms + penalty) and the generator step, fused kernels vs the fp64 engine.
    Shapes: whole tiles, a partial last tile (888 rows), the F = 36 tail tile with samples spanning two waves
    (T = 48 > 32), and 144 000 rows (every wave walks several tiles).  Measured on MI355X: see
    profiles/mlp_ln_gp_fused/README.md."""
    tg, te, tc = _trio(cuda, dtype, B, T, F, monkeypatch)
    fz, dt = tg._fused, tg.dtype
    real, noise, alpha = _inputs(B, T, F)
    lt = LTOL[dtype]
    with torch.no_grad():
        fake = torch.ops.hfrep.mlp_gen_fwd(noise.to(cuda, dt), fz.gw)
        ref = _critic_update(f"{dtype} {B}x{T}x{F}", tg, te, tc, real, fake.float().cpu(), alpha, dtype)
        assert ref[3].item() > 0
        tg.generator.zero_grad()
        tc.generator.zero_grad()
        lg = fz._generator_grads(noise.to(cuda, dt), fake)
        lc = tc.generator_grads(noise.double())
        tb = cpu_twin(tg, "bfloat16") if dtype == "bfloat16" and B <= 64 else None
        if tb is not None:
            tb.generator_grads(noise.to(dt))
        rel = _rel(tg.generator.flat.grad, tc.generator.flat.grad)
        print(f"[{dtype} {B}x{T}x{F}] generator flat rel {rel:.3e} loss {lg.item():.6f} ref {lc.item():.6f}")
        assert_blocks_close(tg.generator, tc.generator, dtype, label=f"mlp_ln {dtype} {B}x{T}x{F} generator",
                            flat_tol=TOL[dtype], model_cpu=tb.generator if tb else None)
        for i, g in enumerate(fz.gg):
            assert g.abs().sum().item() > 0, f"generator gradient view {i} is all zero"
        assert abs(lg.item() - lc.item()) <= lt * max(1.0, abs(lc.item())), (lg.item(), lc.item())


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("B,T,F", SHAPES[1:3])
def test_mlp_ln_gp_terms_on_their_own(cuda, dtype, B, T, F, monkeypatch):
    """gp_weight = 0: the gradients are the W terms alone.  real == fake: x_hat = x, the W terms cancel and
    only the penalty's second-order term remains.  So neither term's error can hide behind the other."""
    real, noise, alpha = _inputs(B, T, F)
    with torch.no_grad():
        tg, te, tc = _trio(cuda, dtype, B, T, F, monkeypatch, gp_weight=0.0)
        fake = torch.ops.hfrep.mlp_gen_fwd(noise.to(cuda, tg.dtype), tg._fused.gw).float().cpu()
        ref = _critic_update(f"{dtype} {B}x{T}x{F} W only", tg, te, tc, real, fake, alpha, dtype)
        assert ref[0].item() == pytest.approx(ref[1].item() + ref[2].item(), abs=1e-12)
        tg, te, tc = _trio(cuda, dtype, B, T, F, monkeypatch)
        x = real.to(tg.dtype).float()  # (one rounding for both copies)
        ref = _critic_update(f"{dtype} {B}x{T}x{F} penalty only", tg, te, tc, x, x, alpha, dtype)
        assert abs(ref[1].item() + ref[2].item()) < 1e-12 and ref[3].item() > 0


def test_mlp_ln_gp_bitwise_and_engine_parity(cuda, monkeypatch):
    """Three training iterations: two fused runs are bitwise identical (fixed-order reductions, no atomics);
    the fused run tracks the GPU engine path (HFREP_MLP_FUSED=0) on the same RNG stream."""
    from hfrep.train.gan_trainer import GANTrainer

    T, F, B = 24, 32, 96
    ds = np.random.RandomState(1).rand(256, T, F).astype(np.float32)
    cfg = _cfg("float32", B, T, F)

    def run(fused):
        monkeypatch.setenv("HFREP_MLP_FUSED", "1" if fused else "0")
        tr = GANTrainer(cfg, ds, device=cuda)
        assert (tr._fused is not None) == fused
        for _ in range(3):
            tr.train_step()
        torch.cuda.synchronize()
        return tr

    a, b, e = run(True), run(True), run(False)
    assert torch.equal(a.critic.flat, b.critic.flat) and torch.equal(a.generator.flat, b.generator.flat)
    assert torch.equal(a._d_acc, b._d_acc) and torch.equal(a._g_acc, b._g_acc)
    for m in ("critic", "generator"):
        pa, pe = getattr(a, m).flat, getattr(e, m).flat
        print(f"{m} params fused vs engine rel {_rel(pa, pe):.3e}")
        assert _rel(pa, pe) < 1e-4, f"{m} params drift from the engine path: {_rel(pa, pe):.2e}"
    la, le = a.losses(), e.losses()
    print(la, le)
    for k in ("d_loss", "g_loss"):
        assert abs(la[k] - le[k]) <= 1e-3 * max(1.0, abs(le[k])), (la, le)
    assert la["gp"] > 0


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_mlp_ln_gp_poisoned_outputs_all_written(cuda, dtype):
    """With the debug poison mode every output, slab and workspace of the new ops starts as NaN, so an element
    a kernel leaves unwritten turns the losses or parameters non-finite.  Odd batch (37) and window (23): the
    last row tile is partial."""
    from hfrep.ops import _native
    from hfrep.train.gan_trainer import GANTrainer

    ops = _native.native()
    prev = ops.set_debug_poison(True)
    try:
        ds = np.random.RandomState(0).rand(64, 23, 32).astype(np.float32)
        tr = GANTrainer(_cfg(dtype, 37, 23, 32), ds, device=cuda)
        assert tr._fused is not None
        for _ in range(2):
            tr.train_step()
        torch.cuda.synchronize()
        rec = tr.losses()
        assert all(np.isfinite(v) for k, v in rec.items() if k != "iteration"), rec
        for m in (tr.generator, tr.critic):
            assert bool(torch.isfinite(m.flat).all()), m.model_name
    finally:
        ops.set_debug_poison(prev)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_mlp_ln_gp_graph_replay_matches_eager(cuda, dtype, monkeypatch):
    """The step replayed from a captured hipGraph (GraphedStep: 2 eager steps, capture, replays) equals the
    eager step bit for bit."""
    from hfrep.train.gan_trainer import GANTrainer
    from hfrep.train.runner import GraphedStep

    monkeypatch.delenv("HFREP_MLP_FUSED", raising=False)
    ds = np.random.RandomState(2).rand(256, 24, 32).astype(np.float32)
    eager, graphed = (GANTrainer(_cfg(dtype, 64, seed=11), ds, device=cuda) for _ in range(2))
    assert eager._fused is not None and graphed._fused is not None
    for _ in range(4):
        eager.train_step()
    step = GraphedStep(graphed, warmup=2)
    for _ in range(4):
        step()
    assert step.graph is not None
    torch.cuda.synchronize()
    assert graphed.iteration == eager.iteration == 4
    assert torch.equal(graphed.generator.flat, eager.generator.flat)
    assert torch.equal(graphed.critic.flat, eager.critic.flat)
    assert torch.equal(graphed._d_acc, eager._d_acc) and torch.equal(graphed._g_acc, eager._g_acc)
