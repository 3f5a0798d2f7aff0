"""Adjoint reuse in the gradient penalty's reverse-over-tangent pass (CPU, reference path).

The tangent system is the linearisation of the primal one, so the adjoints of its tangent quantities are
the plain BPTT of the tangent seed.  ``critic_gp_grads`` seeds the x_hat BPTT and the tangent reverse with
the same ones, keeps the BPTT's dZ and per-step h adjoints and runs a single-stream tangent reverse
(``R.lstm_seq_tbwd_ahd``); ``HFREP_GP_REUSE=0`` restores the two-stream pass.
"""
import numpy as np
import pytest
import torch

from hfrep.ops import reference as R
from hfrep.train.gan_trainer import GANConfig, GANTrainer

H, K = 7, 5


def _point(B, T, act, seed=3):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    x, xd = rn(B, T, K) * 0.5, rn(B, T, K) * 0.5
    W, U, b = rn(K, 4 * H) * K ** -0.5, rn(H, 4 * H) * H ** -0.5, rn(4 * H) * 0.1
    _, gates, cs = R.lstm_seq_fwd(x @ W + b, U, act)
    _, zds, cds = R.lstm_seq_tfwd(xd @ W, gates, cs, U, act)
    return gates, cs, zds, cds, U, rn(B, T, H), rn(B, T, H)


@pytest.mark.parametrize("act", [2, 0])
@pytest.mark.parametrize("T", [1, 4])
def test_tangent_adjoints_are_the_plain_bptt(T, act):
    gates, cs, zds, cds, U, dH, dHd = _point(3, T, act)
    _, dZd = R.lstm_seq_tbwd(dH, dHd, gates, cs, zds, cds, U, act)
    ref = R.lstm_seq_bwd(dHd, gates, cs, U, act)
    assert (dZd - ref).abs().max().item() <= 1e-12


@pytest.mark.parametrize("act", [2, 0])
@pytest.mark.parametrize("T", [1, 4])
def test_single_stream_reference_reproduces_dz(T, act):
    gates, cs, zds, cds, U, dH, dHd = _point(3, T, act)
    dZ, dZd = R.lstm_seq_tbwd(dH, dHd, gates, cs, zds, cds, U, act)
    dZb, ahd = R.lstm_seq_bwd_ahd(dHd, gates, cs, U, act)
    assert torch.equal(dZb, R.lstm_seq_bwd(dHd, gates, cs, U, act))
    assert (dZb - dZd).abs().max().item() <= 1e-12
    got = R.lstm_seq_tbwd_ahd(dH, ahd, gates, cs, zds, cds, U, act)
    assert (got - dZ).abs().max().item() <= 1e-12
    # no primal seed
    dZ0, _ = R.lstm_seq_tbwd(torch.zeros_like(dH), dHd, gates, cs, zds, cds, U, act)
    got0 = R.lstm_seq_tbwd_ahd(None, ahd, gates, cs, zds, cds, U, act)
    assert (got0 - dZ0).abs().max().item() <= 1e-12


def test_critic_gp_grads_switch_on_and_off(monkeypatch):
    """2-LSTM critic, B = 5, T = 3, fp32 on the CPU path: same flat gradient and loss pack either way."""
    B, T, F = 5, 3, 4
    cfg = GANConfig(arch="lstm", loss="wgan_gp", window=T, features=F, batch_size=B, hidden=6, dtype="float32")
    tr = GANTrainer(cfg, np.random.RandomState(0).rand(12, T, F).astype(np.float32))
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        tr.critic.flat.add_(0.05 * torch.randn(tr.critic.flat.shape, generator=g))
    real, fake, alpha = torch.rand(B, T, F, generator=g), torch.randn(B, T, F, generator=g), torch.rand(B, generator=g)
    out = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("HFREP_GP_REUSE", sw)
        tr.critic.zero_grad()
        with torch.no_grad():
            pack = tr.critic_gp_grads(real, fake, alpha)
        out[sw] = (tr.critic.flat.grad.clone(), pack.clone())
    (g1, p1), (g0, p0) = out["1"], out["0"]
    assert g0.abs().max().item() > 0
    assert (g1 - g0).norm().item() <= 1e-6 * g0.norm().item()
    assert (p1 - p0).abs().max().item() <= 1e-6 * p0.abs().max().item()


def test_reuse_runs_the_single_stream_reference(monkeypatch):
    """With the switch on the two-stream reference is never called on a 2-LSTM critic; off, it is."""
    B, T, F = 3, 2, 4
    cfg = GANConfig(arch="lstm", loss="wgan_gp", window=T, features=F, batch_size=B, hidden=6, dtype="float32")
    tr = GANTrainer(cfg, np.random.RandomState(0).rand(12, T, F).astype(np.float32))
    calls = []
    two, one = R.lstm_seq_tbwd, R.lstm_seq_tbwd_ahd
    monkeypatch.setattr(R, "lstm_seq_tbwd", lambda *a, **k: (calls.append("two"), two(*a, **k))[1])
    monkeypatch.setattr(R, "lstm_seq_tbwd_ahd", lambda *a, **k: (calls.append("one"), one(*a, **k))[1])
    g = torch.Generator().manual_seed(4)
    real, fake, alpha = torch.rand(B, T, F, generator=g), torch.randn(B, T, F, generator=g), torch.rand(B, generator=g)
    for sw, want in (("1", ["one", "one"]), ("0", ["two", "two"])):
        monkeypatch.setenv("HFREP_GP_REUSE", sw)
        calls.clear()
        with torch.no_grad():
            tr.critic_gp_grads(real, fake, alpha)
        assert calls == want
