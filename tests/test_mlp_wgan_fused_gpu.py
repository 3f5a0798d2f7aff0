"""Fused clipped-WGAN kernels (csrc/mlp_clip.hip mlp_wgan_critic / mlp_wgan_critic_dx, train/mlp_fused.py)
vs the CPU fp64 explicit engine and the GPU engine path.

The clipped MLP WGAN of GAN/WGAN.py: per-row critic Dense -> LReLU -> LN -> Dense -> LReLU -> LN ->
Dense(1), W loss mean(label * s), weight clipping after the fake step.  Checked: path selection, all
ten critic gradients and the loss against the fp64 engine for both labels, the generator gradient
through the frozen critic, run-to-run bitwise determinism, whole training steps against the engine
path (HFREP_MLP_FUSED=0), the debug-poison run and the decline log.
"""
import logging

import numpy as np
import pytest
import torch

from _blocks import assert_blocks_close, cpu_twin

pytestmark = pytest.mark.gpu

TOL = {"float32": 2e-4, "bfloat16": 3e-2}
LTOL = {"float32": 1e-4, "bfloat16": 2e-2}
CRITIC_NAMES = ["W1", "b1", "gamma1", "beta1", "W2", "b2", "gamma2", "beta2", "w3", "b3"]


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / max(ref.norm().item(), 1e-30)).item()


def _cfg(dtype, B, T=24, F=32, **kw):
    from hfrep.train.gan_trainer import GANConfig

    return GANConfig(arch="mlp", loss="wgan", window=T, features=F, batch_size=B, dtype=dtype, **kw)


def _pair(cuda, dtype, B, T=24, F=32):
    from hfrep.train.gan_trainer import GANTrainer

    ds = np.random.RandomState(0).rand(64, T, F).astype(np.float32)
    tg = GANTrainer(_cfg(dtype, B, T, F), ds, device=cuda)
    assert tg._fused is not None, "the fused MLP path must be selected on the GPU"
    tc = GANTrainer(_cfg("float64", B, T, F), ds, param_dtype=torch.float64)
    with torch.no_grad():
        # spread the LayerNorm parameters off their (1, 0) initial values: gamma enters every adjoint
        g = torch.Generator().manual_seed(5)
        for v in (tg._fused.cw[2], tg._fused.cw[6]):
            v.add_((0.2 * torch.randn(v.shape, generator=g)).to(v))
        for v in (tg._fused.cw[3], tg._fused.cw[7]):
            v.add_((0.1 * torch.randn(v.shape, generator=g)).to(v))
        tc.generator.flat.copy_(tg.generator.flat.double().cpu())
        tc.critic.flat.copy_(tg.critic.flat.double().cpu())
    return tg, tc


def _inputs(B, T, F, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, T, F, generator=g), torch.randn(B, T, F, generator=g)


def test_mlp_wgan_fused_is_selected(cuda, monkeypatch):
    """The clipped MLP WGAN runs the fused path on a GPU by default; HFREP_MLP_FUSED=0 keeps the engine."""
    from hfrep.train.gan_trainer import GANTrainer

    ds = np.random.RandomState(0).rand(64, 24, 32).astype(np.float32)
    monkeypatch.delenv("HFREP_MLP_FUSED", raising=False)
    tr = GANTrainer(_cfg("float32", 16), ds, device=cuda)
    assert tr._fused is not None and tr._fused.head == 2
    assert hasattr(torch.ops.hfrep, "mlp_wgan_critic") and hasattr(torch.ops.hfrep, "mlp_wgan_critic_dx")
    monkeypatch.setenv("HFREP_MLP_FUSED", "0")
    assert GANTrainer(_cfg("float32", 16), ds, device=cuda)._fused is None


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("B,T,F", [(48, 24, 32), (37, 24, 32), (20, 48, 36), (6000, 24, 32)])
def test_mlp_wgan_fused_grads(cuda, dtype, B, T, F):
    """One critic update's gradients (labels -1 and +1) and the generator gradient through the frozen
    critic, fused kernels vs the fp64 engine (efwd / gan_loss / ebwd; same weights, same batch).  Shapes:
    whole tiles, a partial last tile (888 rows), the F = 36 tail tile, and 144 000 rows (every wave walks
    several tiles: the per-lane partial sums accumulate across the persistent loop).  Each of the ten
    critic gradient views and each generator gradient view is held to the per-block bound on its own
    (tests/_blocks.py: 2e-4 fp32; bf16 max(5e-2, 2 e_cpu) with the CPU bf16 engine's error where B <= 64), so
    a missed slab segment or operand cannot hide in the flat norm.  No block vanishes: one label per pass."""
    from hfrep.ops import functional as Fn

    tg, tc = _pair(cuda, dtype, B, T, F)
    fz, dt = tg._fused, tg.dtype
    tb = cpu_twin(tg, "bfloat16") if dtype == "bfloat16" and B <= 64 else None
    real, noise = _inputs(B, T, F)
    lt = LTOL[dtype]
    ref_views = [tc.critic.gview(l, s.name) for l in tc.critic.layers for s in l.specs]
    assert [tuple(v.shape) for v in ref_views] == [tuple(v.shape) for v in fz.cg]
    with torch.no_grad():
        fake = torch.ops.hfrep.mlp_gen_fwd(noise.to(cuda, dt), fz.gw)
        for x, label in ((real.to(cuda, dt), -1.0), (fake, 1.0)):
            tg.critic.zero_grad()
            tc.critic.zero_grad()
            lg = fz._wgan_critic_grads(x, label)
            s, tape = tc.critic.efwd(x.double().cpu(), save=True)
            out, ds = Fn.gan_loss(s, s.numel(), label, label, 0)
            tc.critic.ebwd(tape, ds)
            if tb is not None:
                tb.critic.zero_grad()
                sb, tape_b = tb.critic.efwd(x.cpu(), save=True)
                tb.critic.ebwd(tape_b, Fn.gan_loss(sb, sb.numel(), label, label, 0)[1])
            rel = _rel(tg.critic.flat.grad, tc.critic.flat.grad)
            print(f"[{dtype} {B}x{T}x{F} label {label:+.0f}] critic flat rel {rel:.3e} loss {lg.item():.6f} "
                  f"ref {out[0].item():.6f}")
            for name, got, ref in zip(CRITIC_NAMES, fz.cg, ref_views):
                r = _rel(got, ref)
                print(f"    {name}: rel {r:.3e} |ref| {ref.norm().item():.3e}")
            assert_blocks_close(tg.critic, tc.critic, dtype, label=f"mlp wgan {dtype} {B}x{T}x{F} critic label {label:+.0f}",
                                flat_tol=TOL[dtype], model_cpu=tb.critic if tb else None)
            for name, got in zip(CRITIC_NAMES, fz.cg):
                assert got.abs().sum().item() > 0, f"critic gradient {name} is all zero (label {label})"
            assert abs(lg.item() - out[0].item()) <= lt * max(1.0, abs(out[0].item())), (lg.item(), out[0].item())
        tg.generator.zero_grad()
        tc.generator.zero_grad()
        lg = fz._generator_grads(noise.to(cuda, dt), fake)
        lc = tc.generator_grads(noise.double())
        if tb is not None:
            tb.generator.zero_grad()
            tb.generator_grads(noise.to(dt))
        rel = _rel(tg.generator.flat.grad, tc.generator.flat.grad)
        print(f"[{dtype} {B}x{T}x{F}] generator flat rel {rel:.3e} loss {lg.item():.6f} ref {lc.item():.6f}")
        assert_blocks_close(tg.generator, tc.generator, dtype, label=f"mlp wgan {dtype} {B}x{T}x{F} generator",
                            flat_tol=TOL[dtype], model_cpu=tb.generator if tb else None)
        for i, g in enumerate(fz.gg):
            assert g.abs().sum().item() > 0, f"generator gradient view {i} is all zero"
        assert abs(lg.item() - lc.item()) <= lt * max(1.0, abs(lc.item())), (lg.item(), lc.item())


def test_mlp_wgan_fused_bitwise_and_engine_parity(cuda, monkeypatch):
    """Three training iterations with the clip active: two fused runs are bitwise identical (fixed-order
    reductions, no atomics); the fused run tracks the GPU engine path (HFREP_MLP_FUSED=0) on the same RNG
    stream; every critic parameter ends inside [-clip, clip]."""
    from hfrep.train.gan_trainer import GANTrainer

    T, F, B = 24, 32, 96
    ds = np.random.RandomState(1).rand(256, T, F).astype(np.float32)
    cfg = _cfg("float32", B, T, F)

    def run(fused):
        monkeypatch.setenv("HFREP_MLP_FUSED", "1" if fused else "0")
        tr = GANTrainer(cfg, ds, device=cuda)
        assert (tr._fused is not None) == fused
        assert tr.clip > 0
        for _ in range(3):
            tr.train_step()
        torch.cuda.synchronize()
        return tr

    a, b, e = run(True), run(True), run(False)
    assert torch.equal(a.critic.flat, b.critic.flat) and torch.equal(a.generator.flat, b.generator.flat)
    assert torch.equal(a._d_acc, b._d_acc) and torch.equal(a._g_acc, b._g_acc)
    for m in ("critic", "generator"):
        pa, pe = getattr(a, m).flat, getattr(e, m).flat
        assert _rel(pa, pe) < 1e-4, f"{m} params drift from the engine path: {_rel(pa, pe):.2e}"
    la, le = a.losses(), e.losses()
    for k in ("d_loss", "g_loss"):
        assert abs(la[k] - le[k]) <= 1e-3 * max(1.0, abs(le[k])), (la, le)
    assert a.critic.flat.abs().max().item() <= a.clip
    assert a.critic.flat.abs().max().item() > 0


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_mlp_wgan_poisoned_outputs_all_written(cuda, dtype):
    """With the debug poison mode every output, slab and workspace of the new ops starts as NaN, so an
    element a kernel leaves unwritten turns the losses or parameters non-finite.  Odd batch (37) and
    window (23): the last row tile is partial."""
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


def test_mlp_wgan_decline_is_logged_once(cuda, caplog, monkeypatch):
    """A width the kernels are not instantiated for (F = 35) runs the engine, and says so in exactly
    one log line that names the width."""
    from hfrep.train.gan_trainer import GANTrainer
    from hfrep.train.mlp_fused import FusedMLP

    monkeypatch.delenv("HFREP_MLP_FUSED", raising=False)
    ds = np.random.RandomState(0).rand(64, 24, 35).astype(np.float32)
    with caplog.at_level(logging.INFO, logger="hfrep.mlp_fused"):
        tr = GANTrainer(_cfg("float32", 16, 24, 35), ds, device=cuda)
        assert tr._fused is None
        assert not FusedMLP.supported(tr)  # asking again does not log again
    lines = [r.getMessage() for r in caplog.records if r.name == "hfrep.mlp_fused"]
    assert len(lines) == 1, lines
    assert "declined" in lines[0] and "(35, 100)" in lines[0] and "not instantiated" in lines[0]
