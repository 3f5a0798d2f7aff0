"""``Fn.conv1d_fwd`` / ``conv1d_dgrad`` / ``conv1d_wgrad_`` on CPU tensors (fp64) against ``R.conv1d_causal`` and
its autograd gradients, and the ``Conv1D`` engine methods (which run through those functions) against
autograd and double backward.  CPU only: on CPU tensors the functions take the unfolded route."""
import numpy as np
import pytest
import torch

from hfrep.models.layers import Conv1D, Sequential
from hfrep.ops import functional as Fn
from hfrep.ops import reference as R
from hfrep.train.gan_trainer import GANConfig, GANTrainer

CASES = [(3, 5, 7, 6, 3, 2), (2, 1, 4, 5, 4, 3)]


def _rel(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _inputs(B, T, Cin, Cout, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, Cin, dtype=torch.float64, generator=g)
    W = torch.randn(k, Cin, Cout, dtype=torch.float64, generator=g) / (k * Cin) ** 0.5
    b = torch.randn(Cout, dtype=torch.float64, generator=g) * 0.1
    dz = torch.randn(B, T, Cout, dtype=torch.float64, generator=g)
    return x, W, b, dz


@pytest.mark.parametrize("B,T,Cin,Cout,k,dil", CASES)
@pytest.mark.parametrize("act", [0, 2, 3])
def test_conv1d_fwd_matches_reference(B, T, Cin, Cout, k, dil, act):
    x, W, b, _ = _inputs(B, T, Cin, Cout, k)
    assert not Fn.conv1d_direct(x, W, dil)  # CPU tensors: the unfolded route
    assert _rel(Fn.conv1d_fwd(x, W, b, act, dil), R.conv1d_causal(x, W, b, act, dil)) <= 1e-12
    assert _rel(Fn.conv1d_fwd(x, W, None, act, dil), R.conv1d_causal(x, W, None, act, dil)) <= 1e-12
    # the caller's unfolded copy gives the same numbers
    cols = Fn.im2col_causal(x, k, dil)
    assert torch.equal(Fn.conv1d_fwd(x, W, b, act, dil, cols=cols), Fn.conv1d_fwd(x, W, b, act, dil))


@pytest.mark.parametrize("B,T,Cin,Cout,k,dil", CASES)
def test_conv1d_dgrad_and_wgrad_match_autograd(B, T, Cin, Cout, k, dil):
    x, W, b, dz = _inputs(B, T, Cin, Cout, k, seed=1)
    xr, Wr, br = x.clone().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    dx_ref, gW_ref, gb_ref = torch.autograd.grad(R.conv1d_causal(xr, Wr, br, None, dil), (xr, Wr, br), dz)
    assert _rel(Fn.conv1d_dgrad(dz, W, dil), dx_ref) <= 1e-12
    g = torch.Generator().manual_seed(7)
    gW0 = torch.randn(k, Cin, Cout, dtype=torch.float64, generator=g)
    gb0 = torch.randn(Cout, dtype=torch.float64, generator=g)
    gW, gb = gW0.clone(), gb0.clone()
    Fn.conv1d_wgrad_(x, dz, gW, gb, dil)  # accumulates
    assert _rel(gW - gW0, gW_ref) <= 1e-12
    assert _rel(gb - gb0, gb_ref) <= 1e-12
    gW2 = gW0.clone()
    Fn.conv1d_wgrad_(None, dz, gW2, None, dil, cols=Fn.im2col_causal(x, k, dil))  # the saved unfolded x, no bias
    assert torch.equal(gW2, gW)


def _model(T, Cin, seed=3):
    m = Sequential([Conv1D(6, 3, "tanh"), Conv1D(5, 2, "leaky_relu", dilation=2)], (T, Cin), name="convtest", seed=seed,
                   dtype=torch.float64)
    with torch.no_grad():
        m.flat.add_(0.05 * torch.randn(m.flat.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5)))
    return m


def test_conv1d_engine_ebwd_matches_autograd():
    B, T, Cin = 3, 5, 4
    m = _model(T, Cin)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, Cin, dtype=torch.float64, generator=g)
    dy = torch.randn(B, T, 5, dtype=torch.float64, generator=g)
    m.zero_grad()
    with torch.no_grad():
        y, tape = m.efwd(x, save=True)
        dx = m.ebwd(tape, dy, need_dx=True)
    explicit = m.flat.grad.clone()
    m.flat.grad = None
    xr = x.clone().requires_grad_(True)
    yr = m(xr)
    dx_ref, oracle = torch.autograd.grad(yr, (xr, m.flat), dy)
    torch.testing.assert_close(y, yr.detach(), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dx, dx_ref, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(explicit, oracle, rtol=1e-9, atol=1e-11)


def test_conv1d_engine_etbwd_matches_double_backward():
    """d/dtheta and d/dx of <v, d(sum_o a_o y_o)/dx>: the tangent pass seeded with v, reversed with seed a."""
    B, T, Cin = 3, 5, 4
    m = _model(T, Cin)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(B, T, Cin, dtype=torch.float64, generator=g)
    v = torch.randn(B, T, Cin, dtype=torch.float64, generator=g)
    a = torch.randn(B, T, 5, dtype=torch.float64, generator=g)
    m.zero_grad()
    with torch.no_grad():
        ctxs, tctxs, h, hd = [], [], x, v
        for layer in m.layers:
            h, c = layer.efwd(h, save=True)
            ctxs.append(c)
        for layer, c in zip(m.layers, ctxs):
            hd, tc = layer.etfwd(c, hd)
            tctxs.append(tc)
        dy, dyd = None, a
        for layer, c, tc in zip(reversed(m.layers), reversed(ctxs), reversed(tctxs)):
            dy, dyd = layer.etbwd(c, tc, dy, dyd, need_dx=True)
    explicit = m.flat.grad.clone()
    m.flat.grad = None
    xr, vr = x.clone().requires_grad_(True), v.clone().requires_grad_(True)
    # the tangent output as a function of (theta, x, v): J(x) v by double backward
    yr = m(xr)
    u = torch.zeros_like(yr, requires_grad=True)
    jt, = torch.autograd.grad(yr, xr, u, create_graph=True)  # J^T u
    jv, = torch.autograd.grad(jt, u, vr, create_graph=True)  # J v
    torch.testing.assert_close(hd, jv.detach(), rtol=1e-9, atol=1e-11)
    oracle, dx_ref, dv_ref = torch.autograd.grad((jv * a).sum(), (m.flat, xr, vr))
    torch.testing.assert_close(explicit, oracle, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(dy, dx_ref, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(dyd, dv_ref, rtol=1e-9, atol=1e-11)


def test_conv_critic_gp_gradient_matches_double_backward():
    """The ("conv", "wgan_gp") trainer's critic update through the engine, as tests/test_engine.py pins it."""
    T, F, B = 6, 5, 4
    cfg = GANConfig(arch="conv", loss="wgan_gp", window=T, features=F, batch_size=B, hidden=7, dtype="float64")
    tr = GANTrainer(cfg, np.random.RandomState(0).rand(20, T, F), param_dtype=torch.float64)
    C, G = tr.critic, tr.generator
    g = torch.Generator().manual_seed(0)
    real = torch.rand(B, T, F, dtype=torch.float64, generator=g)
    noise = torch.randn(B, T, F, dtype=torch.float64, generator=g)
    alpha = torch.rand(B, dtype=torch.float64, generator=g)
    with torch.no_grad():
        fake = G.predict(noise)
        C.zero_grad()
        tr.critic_gp_grads(real, fake, alpha)
    explicit = C.flat.grad.clone()
    C.flat.grad = None
    xh = (alpha[:, None, None] * real + (1 - alpha[:, None, None]) * fake).requires_grad_(True)
    gx, = torch.autograd.grad(C(xh).sum(), xh, create_graph=True)
    L = -C(real).mean() + C(fake).mean() + tr.gp_weight * R.gradient_penalty_from_grad(gx)
    oracle, = torch.autograd.grad(L, C.flat)
    torch.testing.assert_close(explicit, oracle, rtol=1e-9, atol=1e-11)
