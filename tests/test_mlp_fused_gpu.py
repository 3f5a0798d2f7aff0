"""Fused MLP-GAN kernels (csrc/mlp_*.hip, train/mlp_fused.py) vs the CPU fp64 explicit engine.

BASELINE configs 3 / 4: the vanilla GAN (GAN/GAN.py) and the MLP WGAN-GP (GAN/WGAN_GP.py).  Every
fused pass is checked against the layer-by-layer fp64 reference of the same quantity: the generator
forward, the WGAN-GP critic gradient (W terms + reverse-over-tangent penalty), the GAN discriminator
gradient, the generator gradient through the frozen critic and the loss values; plus run-to-run
bitwise determinism and whole training steps against the GPU engine path (HFREP_MLP_FUSED=0).
"""
import numpy as np
import pytest
import torch

from _blocks import VANISHED, assert_blocks_close, block_norms, cpu_twin, wasserstein_half_scales

pytestmark = pytest.mark.gpu

TOL = {"float32": 2e-4, "bfloat16": 3e-2}
# the three biases of the affine GP critic: zero in a whole update, held to their real-half term (tests/_blocks.py)
BIASES = VANISHED["mlp", "wgan_gp"]


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / max(ref.norm().item(), 1e-30)).item()


def _pair(cuda, loss, dtype, B, T=24, F=32):
    from hfrep.train.gan_trainer import GANConfig, GANTrainer

    ds = np.random.RandomState(0).rand(64, T, F).astype(np.float32)
    kw = dict(arch="mlp", loss=loss, window=T, features=F, batch_size=B)
    tg = GANTrainer(GANConfig(dtype=dtype, **kw), ds, device=cuda)
    assert tg._fused is not None, "the fused MLP path must be selected on the GPU"
    return tg, cpu_twin(tg, "float64")


def _bf16_twin(tg, B):
    """The CPU bf16 engine on ``tg``'s weights where it is cheap (B <= 64): its per-block error e_cpu raises a
    block's bound to max(5e-2, 2 e_cpu) (tests/_blocks.py).  None for fp32 runs and at the large batches."""
    return cpu_twin(tg, "bfloat16") if tg.dtype == torch.bfloat16 and B <= 64 else None


def _gp_critic_blocks(tg, tc, tb, real, fake, alpha, dtype, tag, got=None):
    """The fp64 engine's GP critic gradient of (real, fake) into ``tc`` and, block by block, the fused
    gradient (``got``, default ``tg``'s flat gradient) against it; the flat error at TOL as before.  Returns
    the fp64 loss pack."""
    x, f = real.to(tg.dtype).cpu(), fake.cpu()  # the inputs the GPU path saw
    scales = wasserstein_half_scales(tc, x.double(), BIASES)
    tc.critic.zero_grad()
    pack_c = tc.critic_gp_grads(x.double(), f.double(), alpha.double())
    if tb is not None:
        tb.critic.zero_grad()
        tb.critic_gp_grads(x, f, alpha)
    assert_blocks_close(tg.critic, tc.critic, dtype, BIASES, scales, f"{tag} critic", flat_tol=TOL[dtype], got=got,
                        model_cpu=tb.critic if tb else None)
    return pack_c


def _generator_blocks(tg, tc, tb, noise, dtype, tag):
    """The fp64 engine's generator gradient into ``tc`` and the fused one against it, block by block."""
    z = noise.to(tg.dtype).cpu()
    tc.generator.zero_grad()
    lc = tc.generator_grads(z.double())
    if tb is not None:
        tb.generator.zero_grad()
        tb.generator_grads(z)
    assert_blocks_close(tg.generator, tc.generator, dtype, label=f"{tag} generator", flat_tol=TOL[dtype],
                        model_cpu=tb.generator if tb else None)
    return lc


def _inputs(B, T, F, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, T, F, generator=g), torch.randn(B, T, F, generator=g), torch.rand(B, generator=g)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("B,T,F", [(48, 24, 32), (37, 24, 32), (20, 48, 36)])
def test_mlp_wgan_gp_fused_grads(cuda, dtype, B, T, F):
    """Config 4: generator forward, the critic update's gradient and loss pack, and the generator
    gradient, fused kernels vs the fp64 engine (same weights, same batch): the flat gradients and every
    parameter block on its own."""
    tg, tc = _pair(cuda, "wgan_gp", dtype, B, T, F)
    tb, tag = _bf16_twin(tg, B), f"mlp wgan_gp {dtype} {B}x{T}x{F}"
    fz = tg._fused
    ops = torch.ops.hfrep
    dt = tg.dtype
    real, noise, alpha = _inputs(B, T, F)
    with torch.no_grad():
        fake = ops.mlp_gen_fwd(noise.to(cuda, dt), fz.gw)
        fc = tc.generator.predict(noise.double())
        assert _rel(fake, fc) < TOL[dtype], f"G(z) rel err {_rel(fake, fc):.2e}"
        pack_g = fz._wgp_critic_grads(real.to(cuda, dt), fake)
        pack_c = _gp_critic_blocks(tg, tc, tb, real, fake, alpha, dtype, tag)
        lt = 1e-4 if dtype == "float32" else 2e-2
        for a, b in zip(pack_g.cpu().tolist(), pack_c.tolist()):
            assert abs(a - b) <= lt * max(1.0, abs(b)), (pack_g, pack_c)
        lg = fz._generator_grads(noise.to(cuda, dt), fake)
        lc = _generator_blocks(tg, tc, tb, noise, dtype, tag)
        assert abs(lg.item() - lc.item()) <= lt * max(1.0, abs(lc.item()))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("B", [48, 37])
def test_mlp_gan_fused_grads(cuda, dtype, B):
    """Config 3: the discriminator update on real (label 1) and fake (label 0) and the generator update
    (label 1 through the frozen discriminator), fused vs the fp64 engine: the flat gradients and every
    parameter block on its own (no block of the discriminator vanishes: one label per update)."""
    from hfrep.ops import functional as Fn

    T, F = 24, 32
    tg, tc = _pair(cuda, "gan", dtype, B, T, F)
    tb, tag = _bf16_twin(tg, B), f"mlp gan {dtype} B {B}"
    fz = tg._fused
    dt = tg.dtype
    real, noise, _ = _inputs(B, T, F)
    lt = 1e-4 if dtype == "float32" else 2e-2
    with torch.no_grad():
        for x, label in ((real, 1.0), (torch.sigmoid(noise), 0.0)):
            tg.critic.zero_grad()
            lg = fz._gan_d_grads(x.to(cuda, dt), label)
            xs = x.to(dt)  # the input the GPU path saw
            for t in filter(None, (tc, tb)):
                t.critic.zero_grad()
                p, tape = t.critic.efwd(xs.double() if t is tc else xs, save=True)
                o, dp = Fn.gan_loss(p, p.numel(), label, label, 1)
                t.critic.ebwd(tape, dp)
                if t is tc:
                    out = o
            assert_blocks_close(tg.critic, tc.critic, dtype, label=f"{tag} D label {label}", flat_tol=TOL[dtype],
                                model_cpu=tb.critic if tb else None)
            assert abs(lg.item() - out[0].item()) <= lt * max(1.0, abs(out[0].item()))
        fake = torch.ops.hfrep.mlp_gen_fwd(noise.to(cuda, dt), fz.gw)
        lg = fz._generator_grads(noise.to(cuda, dt), fake)
        lc = _generator_blocks(tg, tc, tb, noise, dtype, tag)
        assert abs(lg.item() - lc.item()) <= lt * max(1.0, abs(lc.item()))


@pytest.mark.parametrize("loss", ["wgan_gp", "gan"])
def test_mlp_fused_bitwise_and_engine_parity(cuda, loss, monkeypatch):
    """Three training iterations: two fused runs are bitwise identical (fixed-order reductions, no
    atomics); the fused run tracks the GPU engine path (HFREP_MLP_FUSED=0) on the same RNG stream."""
    from hfrep.train.gan_trainer import GANConfig, GANTrainer

    T, F, B = 24, 32, 96
    ds = np.random.RandomState(1).rand(256, T, F).astype(np.float32)
    cfg = GANConfig(arch="mlp", loss=loss, window=T, features=F, batch_size=B, dtype="float32")

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
        assert _rel(pa, pe) < 1e-4, f"{m} params drift from the engine path: {_rel(pa, pe):.2e}"
    la, le = a.losses(), e.losses()
    for k in ("d_loss", "g_loss"):
        assert abs(la[k] - le[k]) <= 1e-3 * max(1.0, abs(le[k])), (la, le)


def test_mlp_fused_large_batch_slices(cuda):
    """At a batch spanning many persistent-grid rounds the fused critic gradient is the average of
    the gradients of its four quarter batches (bf16 and fp32)."""
    T, F = 24, 32
    for dtype in ("float32", "bfloat16"):
        B = 4 * 8192
        tg, _ = _pair(cuda, "wgan_gp", dtype, B, T, F)
        fz, dt = tg._fused, tg.dtype
        real, noise, _ = _inputs(B, T, F, seed=3)
        with torch.no_grad():
            fake = torch.ops.hfrep.mlp_gen_fwd(noise.to(cuda, dt), fz.gw)
            tg.critic.zero_grad()
            fz._wgp_critic_grads(real.to(cuda, dt), fake)
            full = tg.critic.flat.grad.clone()
            acc = torch.zeros_like(full)
            r = real.to(cuda, dt)
            for q in range(4):
                tg.critic.zero_grad()
                sl = slice(q * B // 4, (q + 1) * B // 4)
                fz._wgp_critic_grads(r[sl].contiguous(), fake[sl].contiguous())
                acc += tg.critic.flat.grad / 4
        rel = _rel(full, acc)
        assert rel < (1e-5 if dtype == "float32" else 2e-2), f"{dtype}: full vs slice-average rel {rel:.2e}"


@pytest.mark.parametrize("loss,B,T,F", [("wgan_gp", 37, 24, 32), ("gan", 300, 40, 32), ("wgan_gp", 45, 24, 36),
                                        ("gan", 6000, 24, 32)])
def test_mlp_gen_bwd_inkernel_matches_operand_path(cuda, loss, B, T, F):
    """bf16 configs 3 / 4: the generator reverse with its ten parameter gradients accumulated in the
    kernel (mlp_gen_bwd_w: u1 / u2 / dz1 / dz2 / dfake / noise staged transposed in LDS, bias gradients
    from a ones row of each X image) vs the operand path (mlp_gen_bwd + linear_wgrad_ + slab sums):
    same bf16 operands, different fp32 summation order; two in-kernel runs bitwise identical."""
    ops = torch.ops.hfrep
    tg, _ = _pair(cuda, loss, "bfloat16", B, T, F)
    fz, dt = tg._fused, tg.dtype
    assert fz.gen_wgrad_inkernel
    _, noise, _ = _inputs(B, T, F, seed=9)
    grads, losses = [], []
    with torch.no_grad():
        z = noise.to(cuda, dt)
        fake = ops.mlp_gen_fwd(z, fz.gw)
        for inkernel in (True, True, False):
            fz.gen_wgrad_inkernel = inkernel
            tg.generator.zero_grad()
            losses.append(fz._generator_grads(z, fake).clone())
            grads.append(tg.generator.flat.grad.clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(losses[0], losses[2])
    rel = _rel(grads[0], grads[2])
    assert rel < 1e-4, f"in-kernel vs operand-path generator gradient rel {rel:.2e}"
    # every parameter tensor on its own (a missed slab segment or a wrong ones row cannot hide in the flat norm).
    # Both paths sum the same bf16 products in fp32, in another order: two fp32 implementations of one sum,
    # so the project's fp32 bound of 2e-4 per block
    assert_blocks_close(tg.generator, tg.generator, "bfloat16", label=f"gen in-kernel vs operand {loss} {B}x{T}x{F}",
                        flat_tol=1e-4, tol_block=2e-4, got=grads[0], ref=grads[2])
    assert all(v > 0 for v in block_norms(tg.generator, grads[0]).values())


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("B,F", [(37, 32), (5000, 32), (45, 36)])
def test_mlp_gan_critic_colsum_matches_operand_path(cuda, dtype, B, F):
    """Config 3: the discriminator update with its gradients as dz-weighted column sums in the kernel
    (mlp_gan_critic_g) vs the operand path (mlp_gan_critic + linear_wgrad_), labels 1 and 0; two
    column-sum runs are bitwise identical; the column sums also against the fp64 engine, block by block."""
    T = 24
    from hfrep.ops import functional as Fn

    tg, tc = _pair(cuda, "gan", dtype, B, T, F)
    fz, dt = tg._fused, tg.dtype
    assert fz.gan_colsum
    real, noise, _ = _inputs(B, T, F, seed=13)
    with torch.no_grad():
        for x, label in ((real, 1.0), (torch.sigmoid(noise), 0.0)):
            xg = x.to(cuda, dt)
            grads, losses = [], []
            for colsum in (True, True, False):
                fz.gan_colsum = colsum
                tg.critic.zero_grad()
                losses.append(fz._gan_d_grads(xg, label).clone())
                grads.append(tg.critic.flat.grad.clone())
            assert torch.equal(grads[0], grads[1]) and torch.equal(losses[0], losses[1])
            rel = _rel(grads[0], grads[2])
            assert rel < (1e-5 if dtype == "float32" else 5e-3), f"label {label}: column-sum vs operand rel {rel:.2e}"
            # and the column sums against the fp64 engine, every parameter block on its own
            tc.critic.zero_grad()
            p, tape = tc.critic.efwd(xg.double().cpu(), save=True)
            tc.critic.ebwd(tape, Fn.gan_loss(p, p.numel(), label, label, 1)[1])
            assert_blocks_close(tg.critic, tc.critic, dtype, label=f"gan colsum {dtype} B {B} F {F} label {label}",
                                flat_tol=TOL[dtype], got=grads[0])
            torch.testing.assert_close(losses[0], losses[2], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("B,T,F", [(37, 24, 32), (300, 40, 32), (45, 48, 36), (6000, 24, 32)])
def test_mlp_wgp_tsum_matches_operand_path(cuda, dtype, B, T, F):
    """Config 4: the GP critic update with rows walked t-major and the weight gradients as per-t column
    sums (mlp_wgp_critic_t: gW2 = sum_t S2[t] (x) w3_t, gW1 = sum_t S1[t] (x) W2 w3_t, gw3_t = S3[t]) vs
    the operand path on the same batch: the loss pack to fp32 rounding (the score sums run in another
    order), the gradient to the summation order (fp32) / the operand path's bf16 operand rounding (bf16);
    two runs bitwise identical."""
    tg, tc = _pair(cuda, "wgan_gp", dtype, B, T, F)
    fz, dt = tg._fused, tg.dtype
    assert fz.wgrad_tsum  # the t-major kernel is what a fresh trainer selects with the affine path off
    fz.affine = False  # the per-row kernels under test
    real, noise, alpha = _inputs(B, T, F, seed=7)
    packs, grads = [], []
    with torch.no_grad():
        fake = torch.ops.hfrep.mlp_gen_fwd(noise.to(cuda, dt), fz.gw)
        r = real.to(cuda, dt)
        for mode in ("t", "t", "op"):
            fz.wgrad_tsum = mode == "t"
            tg.critic.zero_grad()
            packs.append(fz._wgp_critic_grads(r, fake).clone())
            grads.append(tg.critic.flat.grad.clone())
        _gp_critic_blocks(tg, tc, _bf16_twin(tg, B), real, fake, alpha, dtype, f"mlp wgp t-sum {dtype} {B}x{T}x{F}",
                          got=grads[0])
    assert torch.equal(grads[0], grads[1]) and torch.equal(packs[0], packs[1])
    torch.testing.assert_close(packs[0], packs[2], rtol=1e-5, atol=1e-6)
    rel = _rel(grads[0], grads[2])
    assert rel < (1e-5 if dtype == "float32" else 3e-3), f"per-t sums vs operand path rel {rel:.2e}"


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("B,T,F", [(37, 24, 32), (300, 40, 32), (45, 48, 36), (6000, 24, 32), (40000, 24, 32)])
def test_mlp_wgp_affine_matches_per_row_path(cuda, dtype, B, T, F):
    """Config 4, the default critic path: the affine critic's update from per-t batch sums
    (mlp_wgp_affine: column sums of real and fake-real, one-workgroup fp32 finish) and the generator
    step's broadcast dfake (mlp_critic_dx_affine) vs the per-row kernels (mlp_wgp_critic_t /
    mlp_critic_dx) on the same batch and vs the fp64 engine: gradient, loss pack, dfake and the
    generator loss; two runs bitwise identical.  fp32: summation order only; bf16: the per-row kernels
    also round h1 / h2 to bf16 (the sums path does not), so vs the fp64 engine at the bf16 tolerance."""
    ops = torch.ops.hfrep
    tg, tc = _pair(cuda, "wgan_gp", dtype, B, T, F)
    fz, dt = tg._fused, tg.dtype
    assert fz.affine and ops.mlp_affine_supported(F, T) and not ops.mlp_affine_supported(36, 7)
    real, noise, alpha = _inputs(B, T, F, seed=13)
    packs, grads = [], []
    with torch.no_grad():
        fake = ops.mlp_gen_fwd(noise.to(cuda, dt), fz.gw)
        r = real.to(cuda, dt)
        for affine in (True, True, False):
            fz.affine = affine
            tg.critic.zero_grad()
            packs.append(fz._wgp_critic_grads(r, fake).clone())
            grads.append(tg.critic.flat.grad.clone())
        pack_c = _gp_critic_blocks(tg, tc, _bf16_twin(tg, B), real, fake, alpha, dtype,
                                   f"mlp wgp affine {dtype} {B}x{T}x{F}", got=grads[0])
        gd_a, sl_a = ops.mlp_critic_dx_affine(fake, fz.cw)
        gd_b, sl_b = ops.mlp_critic_dx_affine(fake, fz.cw)
        gd_r, sl_r = ops.mlp_critic_dx(fake, fz.cw, 0, -1.0)
        la = ops.mlp_finish(sl_a, None, 1, 1.0 / B, fz.cw[5], 0.0)[0]
        lr = ops.mlp_finish(sl_r, None, 1, 1.0 / B, fz.cw[5], 0.0)[0]
        fz.affine = True
    assert torch.equal(grads[0], grads[1]) and torch.equal(packs[0], packs[1])
    assert torch.equal(gd_a, gd_b) and torch.equal(sl_a, sl_b)
    rel = _rel(grads[0], grads[2])
    assert rel < (2e-5 if dtype == "float32" else TOL[dtype]), f"sums vs per-row path rel {rel:.2e}"
    lt = 1e-5 if dtype == "float32" else 2e-2
    for a, b, c in zip(packs[0].cpu().tolist(), packs[2].cpu().tolist(), pack_c.tolist()):
        assert abs(a - b) <= lt * max(1.0, abs(b)) and abs(a - c) <= 10 * lt * max(1.0, abs(c)), (packs, pack_c)
    # dfake: the same per-t row for every sample; the per-row kernel's value to its rounding
    assert torch.equal(gd_a, gd_a[:1].expand_as(gd_a))
    assert _rel(gd_a, gd_r) < (1e-5 if dtype == "float32" else 2e-2)
    assert abs(la.item() - lr.item()) <= lt * max(1.0, abs(lr.item()))
