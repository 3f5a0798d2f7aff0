"""Adjoint reuse in the fp32 gradient-penalty path on the GPU (csrc/lstm_f32.hip): the single-stream
tangent reverse ``lstmf_tbwd1`` and the BPTT's stored h adjoints (``lstmf_bwd(..., ah_out)``), H = 100.

Shapes: one row, a full 32-row tile, one row into the second tile, a third partial tile; T = 1 (the
``t = 0`` / ``c_{-1}`` masks with no recurrence at all), 2 and 5.  The tangent reverse is the exact-fp32
MFMA product (lstmf_tbwdp_kernel's layout minus the tangent stream), so the bound applied is the plain one:
its max error against fp64 must not exceed twice the two-stream kernel's on the same inputs (no additive
slack: the `2 x + 2e-6` rule of the split-against-exact tests is for kernels on the split product).
"""
import numpy as np
import pytest
import torch

from _blocks import VANISHED, assert_blocks_close
from hfrep.ops import functional as Fn
from hfrep.ops import reference as R

pytestmark = pytest.mark.gpu

H, K = 100, 32
SHAPES = [(B, T) for B in (1, 32, 33, 70) for T in (1, 2, 5)]
TOL32 = dict(rtol=2e-4, atol=2e-5)  # the suite's fp32-kernel-against-fp64 tolerance (tests/test_kernels_gpu.py)


def _ops():
    from hfrep.ops import _native

    return _native.native()


_CACHE = {}


def _point(B, T, act):
    """Inputs and the fp64 reference of one (B, T, act) point, computed once and shared (read-only)."""
    key = (B, T, act)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(1000 * B + 10 * T + act)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    p = dict(x=rn(B, T, K) * 0.5, xd=rn(B, T, K) * 0.3, W=rn(K, 4 * H) * K ** -0.5, b=rn(4 * H) * 0.1,
             U=rn(H, 4 * H) * H ** -0.5, dH=rn(B, T, H), dHd=rn(B, T, H), d1=rn(B, 1), d2=rn(B, 1), w=rn(T * H, 1))
    d = {k: v.double() for k, v in p.items()}
    _, rg, rc = R.lstm_seq_fwd(d["x"] @ d["W"] + d["b"], d["U"], act)
    _, tz, tc = R.lstm_seq_tfwd(d["xd"] @ d["W"], rg, rc, d["U"], act)
    outer = lambda v: (v * d["w"].reshape(1, -1)).reshape(B, T, H)  # noqa: E731
    ref = {}
    for head in (False, True):
        sd = outer(d["d2"]) if head else d["dHd"]
        dzd, ahd = R.lstm_seq_bwd_ahd(sd, rg, rc, d["U"], act)
        for seed in (True, False):
            s = (outer(d["d1"]) if head else d["dH"]) if seed else torch.zeros(B, T, H, dtype=torch.float64)
            ref[(head, seed)] = R.lstm_seq_tbwd(s, sd, rg, rc, tz, tc, d["U"], act)[0]
        ref[("ahd", head)], ref[("dzd", head)] = ahd, dzd
    _CACHE[key] = (p, ref)
    return _CACHE[key]


def _err(a, ref):
    return (a.double().cpu() - ref).abs().max().item()


def _close(a, ref):
    s = max(ref.abs().max().item(), 1e-3)
    assert _err(a, ref) <= TOL32["atol"] * max(1.0, s) + TOL32["rtol"] * s


@pytest.mark.parametrize("act", [2, 0])
@pytest.mark.parametrize("B,T", SHAPES)
def test_single_stream_tangent_reverse(cuda, B, T, act):
    """dZ of lstmf_tbwd1 (a_hd = the fp64 reference's, rounded to fp32) vs fp64, HEAD and plain adjoint,
    primal seed present and absent: at most twice the two-stream kernel's error on the same inputs."""
    p, ref = _point(B, T, act)
    dev = {k: v.to(cuda) for k, v in p.items()}
    _, tape = Fn.lstm_layer_fwd(dev["x"], dev["W"], dev["b"], dev["U"], act, True)
    _, ttape = Fn.lstm_layer_tfwd(dev["xd"], dev["W"], tape, dev["U"], act)
    assert isinstance(tape, Fn.FTape)
    ops, U = _ops(), dev["U"]
    o1 = Fn.OuterAdjoint(dev["d1"], dev["w"], (B, T, H))
    o2 = Fn.OuterAdjoint(dev["d2"], dev["w"], (B, T, H))
    for head in (False, True):
        ahd = ref[("ahd", head)].float().to(cuda)
        for seed in (True, False):
            if head:
                old, _ = Fn.lstm_layer_tbwd(o1 if seed else None, o2, tape, ttape, U, act)
                new = ops.lstmf_tbwd1(None, ahd, tape.t, ttape.t, U, act, B, T, dev["d1"].contiguous() if seed else None,
                                      dev["w"].reshape(-1).contiguous())
                if seed:  # the layer-level entry takes the same kernel
                    assert torch.equal(new, Fn.lstm_layer_tbwd1(o1, ahd, tape, ttape, U, act))
            else:
                old, _ = Fn.lstm_layer_tbwd(dev["dH"] if seed else None, dev["dHd"], tape, ttape, U, act)
                new = Fn.lstm_layer_tbwd1(dev["dH"] if seed else None, ahd, tape, ttape, U, act)
            assert torch.isfinite(new).all()
            e_old, e_new = _err(old, ref[(head, seed)]), _err(new, ref[(head, seed)])
            print(f"B {B} T {T} act {act} head {head} seed {seed}: max abs err two-stream {e_old:.3e} single {e_new:.3e}")
            assert e_new <= 2 * e_old, (head, seed, e_old, e_new)


@pytest.mark.parametrize("act", [2, 0])
@pytest.mark.parametrize("B,T", SHAPES)
def test_bptt_stores_h_adjoints(cuda, B, T, act):
    """lstmf_bwd's extra output a_hd vs the reference dht (the suite's fp32 tolerance), plain and HEAD; the
    BPTT's dZ is bitwise what it is without the option."""
    p, ref = _point(B, T, act)
    dev = {k: v.to(cuda) for k, v in p.items()}
    _, tape = Fn.lstm_layer_fwd(dev["x"], dev["W"], dev["b"], dev["U"], act, True)
    assert _ops().lstmf_ahd_supported()
    o2 = Fn.OuterAdjoint(dev["d2"], dev["w"], (B, T, H))
    for head, seed in ((False, dev["dHd"]), (True, o2)):
        dZ, dX, ahd = Fn.lstm_layer_bwd_keep(seed, tape, dev["U"], act)
        assert dX is None and ahd.shape == (B, T, H)
        assert torch.equal(dZ, Fn.lstm_layer_bwd(seed, tape, dev["U"], act))
        _close(ahd, ref[("ahd", head)])
        _close(dZ, ref[("dzd", head)])


def test_single_stream_bitwise_run_to_run(cuda):
    B, T, act = 70, 5, 2
    p, ref = _point(B, T, act)
    dev = {k: v.to(cuda) for k, v in p.items()}
    _, tape = Fn.lstm_layer_fwd(dev["x"], dev["W"], dev["b"], dev["U"], act, True)
    _, ttape = Fn.lstm_layer_tfwd(dev["xd"], dev["W"], tape, dev["U"], act)
    _, _, ahd = Fn.lstm_layer_bwd_keep(dev["dHd"], tape, dev["U"], act)
    runs = [Fn.lstm_layer_tbwd1(dev["dH"], ahd, tape, ttape, dev["U"], act) for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    # and, fed by the BPTT's own a_hd, it is the pipeline's dZ: within the suite's fp32 tolerance of fp64
    _close(runs[0], ref[(False, True)])


def test_row_block_setup_over_many_tiles(cuda):
    """More 32-row tiles than workgroups (B = 256 * 32 + 45, T = 2, tanh), so every workgroup walks several
    tiles and the per-row-block set-up of the reverse kernels (HEAD row factors, descriptors, prologue loads,
    store share) runs more than once: the BPTT with HEAD and the h adjoints kept (dZ and a_hd) and the
    single-stream tangent reverse with HEAD, fed by that a_hd, against fp64 at the suite's fp32 tolerance;
    every output bitwise equal on a second run."""
    B, T, act = 256 * 32 + 45, 2, 2
    p, ref = _point(B, T, act)
    dev = {k: v.to(cuda) for k, v in p.items()}
    _, tape = Fn.lstm_layer_fwd(dev["x"], dev["W"], dev["b"], dev["U"], act, True)
    _, ttape = Fn.lstm_layer_tfwd(dev["xd"], dev["W"], tape, dev["U"], act)
    o1 = Fn.OuterAdjoint(dev["d1"], dev["w"], (B, T, H))
    o2 = Fn.OuterAdjoint(dev["d2"], dev["w"], (B, T, H))
    (dZ, _, ahd), (dZ2, _, ahd2) = (Fn.lstm_layer_bwd_keep(o2, tape, dev["U"], act) for _ in range(2))
    _close(dZ, ref[("dzd", True)])
    _close(ahd, ref[("ahd", True)])
    assert torch.equal(dZ, dZ2) and torch.equal(ahd, ahd2)
    t1, t2 = (Fn.lstm_layer_tbwd1(o1, ahd, tape, ttape, dev["U"], act) for _ in range(2))
    _close(t1, ref[(True, True)])
    assert torch.equal(t1, t2)


class _OpLog:
    """torch.ops.hfrep with every op call's name recorded (one native op = one kernel family)."""

    def __init__(self, ops, log):
        self._ops, self._log = ops, log

    def __getattr__(self, name):
        fn = getattr(self._ops, name)

        def call(*a, **k):
            self._log.append(name)
            return fn(*a, **k)
        return call


@pytest.mark.parametrize("concurrent", ["1", "0"])
def test_critic_gp_grads_reuse_on_and_off(cuda, monkeypatch, concurrent):
    """One critic_gp_grads call on the native fp32 path (B = 40, T = 3, F = 32; side-stream and sequential
    branch) with HFREP_GP_REUSE on and off: the same gradient, flat and block by block, to the fp32 tolerance of
    test_trainer_gradients_gpu_vs_cpu (relative norm 2e-4); with the switch on the call log holds no
    lstmf_tbwd (the two-stream lstmf_tbwdp launch), two lstmf_tbwd1 and one dgrad fewer."""
    from hfrep.train.gan_trainer import GANConfig, GANTrainer

    B, T, F = 40, 3, 32
    monkeypatch.setenv("HFREP_CONCURRENT", concurrent)
    cfg = GANConfig(arch="lstm", loss="wgan_gp", window=T, features=F, batch_size=B, dtype="float32")
    tr = GANTrainer(cfg, np.random.RandomState(0).rand(64, T, F).astype(np.float32), device=cuda)
    g = torch.Generator().manual_seed(13)
    real, fake, alpha = (t.to(cuda) for t in (torch.rand(B, T, F, generator=g), torch.randn(B, T, F, generator=g),
                                              torch.rand(B, generator=g)))
    log, real_ops = [], Fn._ops()
    monkeypatch.setattr(Fn, "_ops", lambda: _OpLog(real_ops, log))
    out = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("HFREP_GP_REUSE", sw)
        tr.critic.zero_grad()
        log.clear()
        with torch.no_grad():
            pack = tr.critic_gp_grads(real, fake, alpha)
        torch.cuda.synchronize()
        out[sw] = (tr.critic.flat.grad.double().cpu(), pack.double().cpu(), list(log))
    (g1, p1, l1), (g0, p0, l0) = out["1"], out["0"]
    assert l0.count("lstmf_tbwd") == 2 and l0.count("lstmf_tbwd1") == 0
    assert l1.count("lstmf_tbwd") == 0 and l1.count("lstmf_tbwd1") == 2
    assert l1.count("lstmf_dgrad") == l0.count("lstmf_dgrad") - 1
    assert l1.count("lstm_wgrad_") == l0.count("lstm_wgrad_")
    # the flat gradient and every parameter block and LSTM gate on its own; the head bias vanishes in a whole
    # update and is measured against its real-half Wasserstein term, |sum_r -1/B| = 1 (tests/_blocks.py)
    head = VANISHED["lstm", "wgan_gp"]
    assert_blocks_close(tr.critic, tr.critic, "float32", head, {head[0]: 1.0}, f"concurrent {concurrent}: reuse on vs off",
                        flat_tol=2e-4, got=g1, ref=g0)
    assert torch.equal(p1, p0)  # the loss pack never sees the tangent reverse, and the BPTT's dZ / dX are unchanged
