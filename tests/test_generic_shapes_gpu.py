"""Kernels off the model's own shapes (run on an MI355X with -m gpu).

tests/test_kernels_gpu.py exercises the fused LSTM kernels at the input widths they are specialised for
(K in {32, 35, 36, 100}) and LayerNorm at a few hundred rows.  Here: the runtime-K path of the bf16 fused
LSTM (csrc/lstm2.hip, ``KX = 0``) and of the fused weight gradient (csrc/gemm2.hip), the trainers at
F in {20, 120}, and LayerNorm (csrc/misc.hip) at its width edges and at more rows than one grid pass
covers.  Every reference is fp64 on the CPU through ``hfrep.ops.reference``; every case runs with the
debug poison on, so an output element that no kernel wrote is NaN and cannot pass by luck.
"""
import numpy as np
import pytest
import torch

import test_kernels_gpu as TK
from _generic_shapes import ACTS, H, LSTM_SHAPES, lstm_inputs
from hfrep.ops import reference as R
from _blocks import BF16_GLOBAL, VANISHED, assert_blocks_close, cpu_twin, wasserstein_half_scales
from test_kernels_gpu import _close, _ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def poison(cuda):
    """Every op output and workspace starts as NaN for the duration of a test."""
    ops = _ops()
    prev = ops.set_debug_poison(True)
    try:
        yield
    finally:
        ops.set_debug_poison(prev)


def _close_cols(got, ref, bound):
    """``_close`` column by column: ``bound`` (.., K) holds the |a| @ |b| magnitude of every element, and
    each input column is measured against its own largest one, so the two heavy edge columns of
    ``lstm_inputs`` do not set the allowance of the columns between them."""
    cs = bound.reshape(-1, bound.shape[-1]).amax(0).clamp_min(1e-3)
    _close(got.double().cpu() / cs, ref / cs, BF, scale=1.0)


# ---------------------------------------------------------------------------------------------------
# 1. bf16 fused LSTM at generic widths
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B,T,K", LSTM_SHAPES)
def test_lstm2_generic_width(cuda, act, B, T, K):
    """Forward, BPTT, tangent forward and tangent reverse of the fused bf16 layer vs the fp64 reference at
    widths that take the runtime-K instantiations (act = sigmoid: lstm_tfwd2_kernel<.., 0, ..> for the
    tangent forward, otherwise lstm_fwd4_kernel<.., 0, .., TAN>), with the fused input gradient on both
    sides of its K = 112 limit."""
    from hfrep.ops import functional as Fn

    x, W, b, U, g = lstm_inputs(B, T, K)
    Wc, bc, Uc = W.to(cuda), b.to(cuda), U.to(cuda)
    Wd, Ud = W.double(), U.double()
    hs, tape = Fn.lstm_layer_fwd(x.to(cuda), Wc, bc, Uc, act, True)
    assert isinstance(tape, torch.Tensor), "bf16 H=100 K<=128 must take the fused v2 path"
    rh, rg, rc = R.lstm_seq_fwd(x.double() @ Wd + b.double(), Ud, act)
    _close(hs, rh, BF)
    hs0, none = Fn.lstm_layer_fwd(x.to(cuda), Wc, bc, Uc, act, False)  # the no-tape instantiation
    assert none is None
    _close(hs0, rh, BF)

    dH = torch.randn(B, T, H, generator=g).to(BF)
    rdz = R.lstm_seq_bwd(dH.double(), rg, rc, Ud, act)
    rdx, bdx = rdz @ Wd.t(), rdz.abs() @ Wd.abs().t()
    _close(Fn.lstm_layer_bwd(dH.to(cuda), tape, Uc, act), rdz, BF)
    for need_dz in (True, False):
        dZ, dX = Fn.lstm_layer_bwd(dH.to(cuda), tape, Uc, act, W=Wc, need_dz=need_dz)
        assert dX.shape == (B, T, K)
        if need_dz:
            _close(dZ, rdz, BF)
        else:
            assert dZ is None
        _close(dX, rdx, BF, scale=bdx.max().item())
        _close_cols(dX, rdx, bdx)

    xd = (torch.randn(B, T, K, generator=g) * 0.3).to(BF)
    hds, ttape = Fn.lstm_layer_tfwd(xd.to(cuda), Wc, tape, Uc, act)
    th, tz, tc = R.lstm_seq_tfwd(xd.double() @ Wd, rg, rc, Ud, act)
    _close(hds, th, BF)
    dHd = torch.randn(B, T, H, generator=g).to(BF)
    for with_dh in (True, False):
        dHc = dH.to(cuda) if with_dh else None
        rz, rzd = R.lstm_seq_tbwd(dH.double() if with_dh else torch.zeros(B, T, H, dtype=torch.float64),
                                  dHd.double(), rg, rc, tz, tc, Ud, act)
        dZ2, dZd2 = Fn.lstm_layer_tbwd(dHc, dHd.to(cuda), tape, ttape, Uc, act)
        _close(dZ2, rz, BF)
        _close(dZd2, rzd, BF)
        dZ3, dZd3, dX3, dXd3 = Fn.lstm_layer_tbwd(dHc, dHd.to(cuda), tape, ttape, Uc, act, W=Wc)
        _close(dZ3, rz, BF)
        _close(dZd3, rzd, BF)
        assert dX3.shape == (B, T, K) and dXd3.shape == (B, T, K)
        for got, z in ((dX3, rz), (dXd3, rzd)):
            ref, bound = z @ Wd.t(), z.abs() @ Wd.abs().t()
            _close(got, ref, BF, scale=bound.max().item())
            _close_cols(got, ref, bound)


@pytest.mark.parametrize("B,T,K", [(40, 5, 20)])
def test_lstm2_head_adjoint_in_kernel_generic_width(cuda, B, T, K):
    """test_lstm2_head_adjoint_in_kernel at a runtime K: the generated-head (GEN) and fused-dX (DX)
    instantiations of the reverse kernels == the launches fed the materialised outer product."""
    from hfrep.ops import functional as Fn

    act = 2
    g = torch.Generator().manual_seed(62)
    x = (torch.randn(B, T, K, generator=g) * 0.5).to(BF).to(cuda)
    W = (torch.randn(K, 4 * H, generator=g) * K ** -0.5).to(cuda)
    U = (torch.randn(H, 4 * H, generator=g) * H ** -0.5).to(cuda)
    b = torch.zeros(4 * H, device=cuda)
    _, tape = Fn.lstm_layer_fwd(x, W, b, U, act, True)
    xd = (torch.randn(B, T, K, generator=g) * 0.3).to(BF).to(cuda)
    _, ttape = Fn.lstm_layer_tfwd(xd, W, tape, U, act)
    w = (torch.randn(T * H, 1, generator=g) * 0.05).to(cuda)
    d = torch.randn(B, 1, generator=g).to(BF).to(cuda)
    dd = torch.randn(B, 1, generator=g).to(BF).to(cuda)
    oa, oad = Fn.OuterAdjoint(d, w, (B, T, H)), Fn.OuterAdjoint(dd, w, (B, T, H))
    # the materialised adjoint with the kernels' rounding, bf16(float(d) * w).  (T H = 500 is no multiple of
    # 8, so materialize() runs the dgrad GEMM here, not the skinny kernel, and rounds w to bf16 first: equal
    # at bf16 tolerance only)
    mat = lambda v: (v.float() * w.reshape(1, -1)).to(BF).reshape(B, T, H)
    dHm, dHdm = mat(d), mat(dd)
    _close(oa.materialize(), dHm.double(), BF)
    _close(oad.materialize(), dHdm.double(), BF)
    for Wx in (None, W):
        r1 = Fn.lstm_layer_bwd(oa, tape, U, act, W=Wx)
        r2 = Fn.lstm_layer_bwd(dHm, tape, U, act, W=Wx)
        for a, c in zip(r1 if Wx is not None else (r1,), r2 if Wx is not None else (r2,)):
            assert torch.equal(a, c)
        for seeds, mats in (((None, oad), (None, dHdm)), ((oa, oad), (dHm, dHdm))):
            t1 = Fn.lstm_layer_tbwd(seeds[0], seeds[1], tape, ttape, U, act, W=Wx)
            t2 = Fn.lstm_layer_tbwd(mats[0], mats[1], tape, ttape, U, act, W=Wx)
            t1b = Fn.lstm_layer_tbwd(seeds[0], seeds[1], tape, ttape, U, act, W=Wx)
            assert all(torch.equal(a, c) for a, c in zip(t1, t1b))
            # (the GEN and tensor-fed instantiations may contract the gate math differently: 1-ulp
            # bf16 differences that the recurrence carries back, so compare at bf16 tolerance)
            for a, c in zip(t1, t2):
                _close(a, c.double(), BF)
    ops = _ops()
    o1 = ops.lstm2_tbwd(None, None, tape, ttape, U, act, W, d, dd, w.reshape(-1))
    o2 = ops.lstm2_tbwd(dHm, dHdm, tape, ttape, U, act, W)
    assert all(torch.equal(a, c) for a, c in zip(o1, o2))
    o3 = ops.lstm2_tbwd(None, None, tape, ttape, U, act, W, d, dd, w.reshape(-1))
    assert all(torch.equal(a, c) for a, c in zip(o1, o3))


# ---------------------------------------------------------------------------------------------------
# 2. bf16 fused weight gradient at generic widths (lstm_wgrad2_kernel: the staging branches on K & 3 and on
#    chunks that straddle the X | H | 1 boundaries)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,K,tangent", [(33, 5, 1, True), (70, 2, 20, True), (40, 3, 33, False), (33, 5, 97, True),
                                           (33, 3, 128, True), (40, 1, 20, False)])
def test_lstm_wgrad_fused_generic_width(cuda, B, T, K, tangent):
    from hfrep.ops import functional as Fn

    N = 4 * H
    g = torch.Generator().manual_seed(30)
    bf = lambda *s: torch.randn(*s, generator=g).to(BF)
    x, hs, dZ = bf(B, T, K), bf(B, T, H), bf(B, T, N)
    xd, hds, dZd = bf(B, T, K), bf(B, T, H), bf(B, T, N)
    gW0, gU0, gb0 = torch.randn(K, N, generator=g), torch.randn(H, N, generator=g), torch.randn(N, generator=g)
    gW, gU, gb = gW0.clone().to(cuda), gU0.clone().to(cuda), gb0.clone().to(cuda)
    Fn.lstm_wgrad_(x.to(cuda), hs.to(cuda), dZ.to(cuda), gW, gU, gb, *(
        (xd.to(cuda), hds.to(cuda), dZd.to(cuda)) if tangent else (None, None, None)), impl=0)
    d = lambda t: t.double().reshape(-1, t.shape[-1])
    rW = gW0.double() + d(x).t() @ d(dZ)
    rU = gU0.double() + d(R.shift_prev(hs.double())).t() @ d(dZ)
    rb = gb0.double() + d(dZ).sum(0)
    if tangent:
        rW += d(xd).t() @ d(dZd)
        rU += d(R.shift_prev(hds.double())).t() @ d(dZd)
    sc = lambda a, b: (d(a).abs().t() @ d(b).abs()).max().item() * (2 if tangent else 1)
    _close(gW, rW, BF, scale=sc(x, dZ))
    _close(gU, rU, BF, scale=sc(hs, dZ))
    _close(gb, rb, BF, scale=d(dZ).abs().sum(0).max().item())
    # tight check against fp32 accumulation of the same bf16 inputs (the kernel's exact math)
    err = (gW.cpu().double() - rW).abs().max().item()
    assert err < 1e-3 * sc(x, dZ), err
    err = (gU.cpu().double() - rU).abs().max().item()
    assert err < 1e-3 * sc(hs, dZ), err
    if T == 1:  # every h_{t-1} is zero: nothing may reach gU
        assert torch.equal(gU.cpu(), gU0)


# ---------------------------------------------------------------------------------------------------
# 3. end to end at generic feature counts
# ---------------------------------------------------------------------------------------------------
HEAD = VANISHED["lstm", "wgan_gp"]  # the critic's head bias: zero in a whole update (tests/_blocks.py)


def _trainers(cuda, dtype, F, T=6, B=40):
    from hfrep.train.gan_trainer import GANConfig, GANTrainer

    ds = np.random.RandomState(0).rand(64, T, F).astype(np.float32)
    kw = dict(arch="lstm", loss="wgan_gp", window=T, features=F, batch_size=B, lrelu_after_first=False)
    tg = GANTrainer(GANConfig(dtype=dtype, **kw), ds, device=cuda)
    tc = GANTrainer(GANConfig(dtype="float64", **kw), ds, param_dtype=torch.float64)
    with torch.no_grad():
        tc.generator.flat.copy_(tg.generator.flat.double().cpu())
        tc.critic.flat.copy_(tg.critic.flat.double().cpu())
    return tg, tc


@pytest.mark.parametrize("F", [20, 120])
def test_trainer_gradients_generic_features_fp32(cuda, F):
    """test_trainer_gradients_gpu_vs_cpu at feature counts off the fp32 kernels' widths."""
    T, B = 6, 40
    tg, tc = _trainers(cuda, "float32", F)
    g = torch.Generator().manual_seed(11)
    real = torch.rand(B, T, F, generator=g)
    noise = torch.randn(B, T, F, generator=g)
    alpha = torch.rand(B, generator=g)
    with torch.no_grad():
        fg = tg.generator.predict(noise.to(cuda))
        fc = tc.generator.predict(noise.double())
        _close(fg, fc, torch.float32)
        scales = wasserstein_half_scales(tc, real.double(), HEAD)
        tg.critic_gp_grads(real.to(cuda), fg, alpha.to(cuda))
        tc.critic_gp_grads(real.double(), fg.double().cpu(), alpha.double())
        assert_blocks_close(tg.critic, tc.critic, "float32", HEAD, scales, f"F = {F} critic fp32", flat_tol=2e-4)
        lg = tg.generator_grads(noise.to(cuda))
        lc = tc.generator_grads(noise.double())
        assert_blocks_close(tg.generator, tc.generator, "float32", label=f"F = {F} generator fp32", flat_tol=2e-4)
        assert abs(lg.item() - lc.item()) < 1e-4 * max(1, abs(lc.item()))


@pytest.mark.parametrize("F", [20, 120])
def test_trainer_gradients_generic_features_bf16(cuda, F):
    """test_trainer_gradients_bf16_fused at feature counts that take the runtime-K fused kernels (and, at
    F = 120, the critic's first-layer input gradient past the fused limit of 112 columns)."""
    T, B = 6, 40
    tg, tc = _trainers(cuda, "bfloat16", F)
    g = torch.Generator().manual_seed(12)
    real = torch.rand(B, T, F, generator=g).to(BF)
    noise = torch.randn(B, T, F, generator=g).to(BF)
    alpha = torch.rand(B, generator=g)
    tb = cpu_twin(tg, "bfloat16")  # the CPU bf16 engine: a block's bound is max(5e-2, 2 e_cpu), tests/_blocks.py
    with torch.no_grad():
        fg = tg.generator.predict(noise.to(cuda))
        scales = wasserstein_half_scales(tc, real.double(), HEAD)
        tg.critic_gp_grads(real.to(cuda), fg, alpha.to(cuda))
        tc.critic_gp_grads(real.double(), fg.double().cpu(), alpha.double())
        tb.critic_gp_grads(real, fg.cpu(), alpha)
        assert_blocks_close(tg.critic, tc.critic, "bfloat16", HEAD, scales, f"F = {F} critic bf16", flat_tol=BF16_GLOBAL,
                            model_cpu=tb.critic)
        tg.generator_grads(noise.to(cuda))
        tc.generator_grads(noise.double())
        tb.generator_grads(noise)
        assert_blocks_close(tg.generator, tc.generator, "bfloat16", label=f"F = {F} generator bf16",
                            flat_tol=BF16_GLOBAL, model_cpu=tb.generator)


# ---------------------------------------------------------------------------------------------------
# 4. LayerNorm: the width edges and several grid passes
# ---------------------------------------------------------------------------------------------------
# D = 128: every lane of the half wave on; D = 4: one lane; D = 132: the first width on the generic
# (one wave per row) kernels; D = 256: their last
@pytest.mark.parametrize("D", [4, 128, 132, 256])
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_layernorm_width_edges(cuda, dt, D):
    TK.test_layernorm(cuda, dt, D)  # forward (save / no-save / fused LeakyReLU equalities) + backward


@pytest.mark.parametrize("D", [4, 128, 132])
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_layernorm_tangent_width_edges(cuda, dt, D):
    TK.test_layernorm_tangent(cuda, dt, D)


ROW_SETS = [None, (8192, 8197), (16384, 16393)]  # None: the last 11 rows


def _many_rows():
    """More rows than any LayerNorm grid covers in one pass (bf16 forward: 8 * CUs workgroups of 16 rows;
    x4 backward: 2048 x 8 rows; generic and tangent backward: 2048 x 4 rows), and no multiple of them."""
    rows = 128 * torch.cuda.get_device_properties(0).multi_processor_count + 11
    assert rows > 16393, "the row sets below assume at least 128 CUs"
    return rows


def _row_sets(rows):
    return [torch.arange(rows - 11, rows) if s is None else torch.arange(*s) for s in ROW_SETS]


def _only(t, idx):
    """t (on the GPU) zeroed outside the rows idx."""
    out = torch.zeros_like(t)
    out[idx.to(t.device)] = t[idx.to(t.device)]
    return out


@pytest.mark.parametrize("D", [100, 35])  # the x4 kernels / the generic kernels
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_layernorm_many_rows(cuda, dt, D):
    """Forward and backward when rows are reached by the kernels' stride loops (their per-column dgamma /
    dbeta partials live in registers across passes).  One lost row in 32 779 is invisible in a column sum, so
    the backward also runs with the seed zeroed outside a few rows -- the last 11, rows of pass two of the
    4-row kernels and of pass two of the 8-row kernel -- and dgamma / dbeta are compared on those alone."""
    ops, rows = _ops(), _many_rows()
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(dt)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    xc, gc, bc = x.to(cuda), gamma.to(cuda), beta.to(cuda)
    y, xhat, rstd = ops.layernorm_fwd(xc, gc, bc, 1e-3)
    ry, rxh, rrs = R.layer_norm_fwd(x.double(), gamma.double(), beta.double(), 1e-3)
    _close(y, ry, dt)
    _close(xhat, rxh, dt)
    _close(rstd, rrs, dt)
    y2, xh2, rs2 = ops.layernorm_fwd(xc, gc, bc, 1e-3, False)
    _close(y2, ry, dt)
    assert torch.equal(y2, y) and xh2.numel() == 0 and rs2.numel() == 0
    # fused LeakyReLU -> LN: the LN of the activation as the separate activation kernel stores it (rounded
    # to dt), bitwise that kernel followed by LN
    xa = ops.act_fwd(xc, 3)
    _close(xa, R.apply_act(x.double(), 3), dt)
    ya, xha, rsa = ops.layernorm_fwd(xa, gc, bc, 1e-3)
    rya, rxa, rra = R.layer_norm_fwd(xa.double().cpu(), gamma.double(), beta.double(), 1e-3)
    for save in (True, False):
        yf, xhf, rsf = ops.layernorm_fwd(xc, gc, bc, 1e-3, save, 0.2)
        _close(yf, rya, dt)
        assert torch.equal(yf, ya)
        if save:
            _close(xhf, rxa, dt)
            _close(rsf, rra, dt)
            assert torch.equal(xhf, xha) and torch.equal(rsf, rsa)

    dy = torch.randn(rows, D, generator=g).to(dt)
    dyc = dy.to(cuda)
    xh64, rs64 = xhat.double().cpu(), rstd.double().cpu()
    gg, gb = torch.zeros(D, device=cuda), torch.zeros(D, device=cuda)
    dx = ops.layernorm_bwd_(dyc, xhat, rstd, gc, gg, gb)
    rdx, rdg, rdb = R.layer_norm_bwd(dy.double(), xh64, rs64, gamma.double())
    _close(dx, rdx, dt)
    _close(gg, rdg, dt, scale=(dy.double().abs() * xh64.abs()).sum(0).max().item())
    _close(gb, rdb, dt, scale=dy.double().abs().sum(0).max().item())
    for idx in _row_sets(rows):
        gg, gb = torch.zeros(D, device=cuda), torch.zeros(D, device=cuda)
        dxs = ops.layernorm_bwd_(_only(dyc, idx), xhat, rstd, gc, gg, gb)
        d, xh = dy[idx].double(), xh64[idx]
        sdx, sdg, sdb = R.layer_norm_bwd(d, xh, rs64[idx], gamma.double())
        _close(dxs[idx.to(cuda)], sdx, dt)
        _close(gg, sdg, dt, scale=(d.abs() * xh.abs()).sum(0).max().item())
        _close(gb, sdb, dt, scale=d.abs().sum(0).max().item())


@pytest.mark.parametrize("D", [100, 35])
@pytest.mark.parametrize("dt", [torch.float32, BF])
def test_layernorm_tangent_many_rows(cuda, dt, D):
    """LN JVP and its reverse (with and without a primal seed, with and without dx / dxd) at more rows than
    one pass of the 2048 x 4-row grid, vs the closed form of hfrep.ops.reference in fp64; dgamma / dbeta
    again also from seeds that live on a few rows only."""
    ops, rows = _ops(), _many_rows()
    g = torch.Generator().manual_seed(17)
    mk = lambda: torch.randn(rows, D, generator=g).to(dt)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(dt)
    xd, dy, dyd = mk(), mk(), mk()
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    gc = gamma.to(cuda)
    _, xhat, rstd = ops.layernorm_fwd(x.to(cuda), gc, beta.to(cuda), 1e-3)
    xh64, rs64, ga64 = xhat.double().cpu(), rstd.double().cpu(), gamma.double()
    xdc, dyc, dydc = xd.to(cuda), dy.to(cuda), dyd.to(cuda)
    _close(ops.layernorm_tfwd(xdc, xhat, rstd, gc), R.layer_norm_tfwd(xd.double(), xh64, rs64, ga64), dt)
    xhatd = R.layer_norm_tfwd(xd.double(), xh64, rs64, torch.ones(D, dtype=torch.float64))

    def check(idx):
        """All four instantiations with the seeds restricted to the rows idx (None: every row)."""
        sel = slice(None) if idx is None else idx
        a, ad = (dyc, dydc) if idx is None else (_only(dyc, idx), _only(dydc, idx))
        d, dd, h, hd = dy[sel].double(), dyd[sel].double(), xh64[sel], xhatd[sel]
        for with_dy in (True, False):
            rdx, rdxd, rdg, rdb = R.layer_norm_tbwd(d if with_dy else None, dd, xd[sel].double(), h, rs64[sel], ga64)
            sg = ((d.abs() * h.abs() if with_dy else 0) + dd.abs() * hd.abs()).sum(0).max().item()
            for need_dx in (True, False):
                gg, gb = torch.zeros(D, device=cuda), torch.zeros(D, device=cuda)
                dx, dxd = ops.layernorm_tbwd_(a if with_dy else None, ad, xdc, xhat, rstd, gc, gg, gb, need_dx)
                if need_dx:
                    _close(dx[sel if idx is None else idx.to(cuda)], rdx, dt)
                    _close(dxd[sel if idx is None else idx.to(cuda)], rdxd, dt)
                else:
                    assert dx.numel() == 0 and dxd.numel() == 0
                _close(gg, rdg, dt, scale=sg)
                if with_dy:
                    _close(gb, rdb, dt, scale=d.abs().sum(0).max().item())
                else:
                    assert torch.count_nonzero(gb).item() == 0  # (a NaN counts)

    check(None)
    for idx in _row_sets(rows):
        check(idx)
