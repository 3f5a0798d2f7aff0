"""The optimizer kernels (``csrc/optim.hip``) against the Keras 2.7 rules in fp64 (``_keras_optim_ref``).

Tolerance.  There is no hand-picked rtol: every comparison runs three engines on the same inputs --
the kernel, the CPU fp32 ``KerasOptimizer`` and the fp64 reference -- and asks, as ``test_lstmf_*split*``
does of the split GEMMs, that the kernel's error be at most twice the fp32 twin's plus one fp32 ulp of
the compared value (of its largest magnitude).  Errors are maxima over the buffer, scaled by
``lr * steps`` (the distance a parameter can have travelled) for parameters and by the slot's magnitude
for slots; where the twin's error is exactly zero the ulp term stands alone.

Same inputs includes the hyper-parameters.  The bindings hand the kernels fp32 scalars, so every
hyper-parameter here is the fp32 value of the workload's (fl32(5e-5), fl32(0.999), ...): the kernels see
exactly what they see in training, and the twin and the fp64 reference see the same numbers.  (With
0.999 as a double the three would disagree about 1 - beta_2 by 1.3e-5 before any arithmetic is done:
1 - fl32(0.999) against fl32(1 - 0.999).)
"""
import numpy as np
import pytest
import torch

import _keras_optim_ref as K

pytestmark = pytest.mark.gpu


def f32(x):
    return float(np.float32(x))


CLIP = f32(0.01)
COMMON = dict(rho=f32(0.9), beta_2=f32(0.999), epsilon=f32(1e-7))
# the workload's optimizers: the critics' RMSprop(5e-5) with the 0.01 clip, the GAN's Adam(2e-4, 0.5), the
# autoencoder's Nadam()
HYPER = {
    "rmsprop": dict(learning_rate=f32(5e-5), beta_1=f32(0.9), **COMMON),
    "adam": dict(learning_rate=f32(2e-4), beta_1=f32(0.5), **COMMON),
    "nadam": dict(learning_rate=f32(1e-3), beta_1=f32(0.9), **COMMON),
}
GRID_CAP = 2048 * 256  # threads of the capped grid: one more element and the stride loop runs twice
STRIDE_N = {"rmsprop": 4 * GRID_CAP + 1003, "adam": GRID_CAP + 1003, "nadam": GRID_CAP + 1003}


def _ops():
    from hfrep.ops import _native

    return _native.native()


def _offset(t, device):
    """``t`` on ``device`` as ``buf[1:]``: contiguous, 4 bytes off 16-byte alignment."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    v = buf[1:]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


class Engines:
    """One optimizer three times over: the kernels, the CPU fp32 twin and the fp64 reference, fed the
    same fp32 parameters and gradients and sharing their ``iterations`` the same way."""

    def __init__(self, kind, cuda):
        from hfrep.train.optim import KerasOptimizer

        h = HYPER[kind]
        self.kind, self.cuda, self.lr = kind, cuda, h["learning_rate"]
        self.gpu = KerasOptimizer(kind, device=cuda, **h)
        self.cpu = KerasOptimizer(kind, **h)
        self.ref = K.RefOptimizer(kind, h["learning_rate"], h["rho"], h["beta_1"], h["beta_2"], h["epsilon"])
        self.flats = {}
        self.misaligned_grad = False

    def add(self, name, p0, misaligned=False):
        """A parameter buffer starting at the fp32 array ``p0``; ``misaligned``: the kernel's buffer and
        its slots are ``buf[1:]`` views."""
        p0 = np.asarray(p0, dtype=np.float32)
        pc = torch.from_numpy(p0.copy())
        pg = _offset(pc, self.cuda) if misaligned else pc.clone().to(self.cuda)
        if misaligned:
            n_slots = 1 if self.kind == "rmsprop" else 2
            self.gpu.load_slots(pg, tuple(_offset(torch.zeros_like(pc), self.cuda) for _ in range(n_slots)))
            assert all(s.data_ptr() % 16 == 4 for s in self.gpu._slots(pg))
        self.flats[name] = [pg, pc, p0.astype(np.float64)]

    def _grad(self, g):
        gc = torch.from_numpy(np.asarray(g, dtype=np.float32))
        return (_offset(gc, self.cuda) if self.misaligned_grad else gc.to(self.cuda)), gc

    def apply(self, name, g, clip=0.0, gscale=1.0):
        f = self.flats[name]
        gg, gc = self._grad(g)
        self.gpu.apply(f[0], gg, clip=clip, gscale=gscale)
        self.cpu.apply(f[1], gc, clip=clip, gscale=gscale)
        f[2] = self.ref.apply(name, f[2], np.asarray(g, dtype=np.float32), clip=clip, gscale=gscale)

    def apply_group(self, names, gs, clip=0.0, gscale=1.0):
        for name, g in zip(names, gs):
            f = self.flats[name]
            f[0].grad, f[1].grad = self._grad(g)
        self.gpu.apply_group([self.flats[n][0] for n in names], clip=clip, gscale=gscale)
        self.cpu.apply_group([self.flats[n][1] for n in names], clip=clip, gscale=gscale)
        new = self.ref.apply_group([(n, self.flats[n][2], np.asarray(g, dtype=np.float32)) for n, g in zip(names, gs)],
                                   clip=clip, gscale=gscale)
        for n, p in zip(names, new):
            self.flats[n][2] = p

    @staticmethod
    def _hold(what, got, twin, ref, scale):
        ref = np.atleast_1d(np.asarray(ref, dtype=np.float64))
        assert got.dtype == torch.float32 and twin.dtype == torch.float32
        eg = float(np.abs(got.detach().double().cpu().numpy().reshape(-1) - ref).max())
        ec = float(np.abs(twin.detach().double().numpy().reshape(-1) - ref).max())
        ulp = float(np.spacing(np.float32(np.abs(ref).max())))
        scale = scale if scale > 0 else 1.0
        print(f"{what}: kernel {eg / scale:.3e}  fp32 twin {ec / scale:.3e}  ulp {ulp / scale:.3e}  (scale {scale:.3e})")
        assert eg / scale <= 2 * ec / scale + ulp / scale, f"{what}: kernel {eg:.3e}, twin {ec:.3e}, ulp {ulp:.3e}"

    def check(self, what):
        """Parameters, every slot, ``iterations`` and the Nadam cache of all three engines, now."""
        steps = self.ref.iterations
        for name, (pg, pc, pr) in self.flats.items():
            self._hold(f"{what} {name} p", pg, pc, pr, self.lr * max(steps, 1))
            for k, (sg, sc, sr) in enumerate(zip(self.gpu._slots(pg), self.cpu._slots(pc), self.ref.slots[name])):
                self._hold(f"{what} {name} slot{k}", sg, sc, sr, float(np.abs(sr).max()))
        assert self.gpu.iterations.item() == self.cpu.iterations.item() == steps, what
        if self.kind == "nadam":
            assert self.cpu.m_cache.dtype == torch.float32
            self._hold(f"{what} m_cache", self.gpu.m_cache, self.cpu.m_cache, self.ref.m_cache, float(self.ref.m_cache))
        else:
            assert self.gpu.m_cache.item() == 1.0


def _params(rng, n, clip):
    """Start inside and outside the clip window where there is one, at unit scale otherwise."""
    return rng.uniform(-1.5 * clip, 1.5 * clip, n) if clip > 0 else rng.randn(n)


@pytest.mark.parametrize("kind,steps", [("nadam", 300), ("adam", 300), ("rmsprop", 100)])
def test_trajectory(cuda, kind, steps):
    """Long runs at the workload's hyper-parameters with fresh gradients every step: Nadam's fp32
    momentum-cache product over 300 factors, Adam with beta_1 = 0.5 past the step where beta_1^t leaves
    the fp32 range (t = 150), RMSprop under its clip.  Compared at steps 1, 2, 10 and the last."""
    clip = CLIP if kind == "rmsprop" else 0.0
    rng = np.random.RandomState(30)
    e = Engines(kind, cuda)
    e.add("w", _params(rng, 1003, clip))
    grads = rng.randn(steps, 1003).astype(np.float32)
    for step in range(1, steps + 1):
        e.apply("w", grads[step - 1], clip=clip)
        if step in (1, 2, 10, steps):
            e.check(f"{kind} step {step}")


@pytest.mark.parametrize("n", [1, 3, 5, 1003, "stride"])
@pytest.mark.parametrize("kind,clip", [("rmsprop", CLIP), ("adam", 0.0), ("nadam", 0.0), ("nadam", CLIP)])
def test_sizes(cuda, kind, clip, n):
    """Three steps at the small sizes (a lone element, less than one float4, a float4 and a tail, more
    than one block) and at the first size whose capped grid (2048 blocks) strides: 2048 * 256 + 1003 for
    the scalar kernels (Adam, Nadam, and ``clip_`` behind the clipped Nadam), four times the cap for
    RMSprop's float4 body."""
    n = STRIDE_N[kind] if n == "stride" else n
    rng = np.random.RandomState(31)
    e = Engines(kind, cuda)
    e.add("w", _params(rng, n, clip))
    for step in range(3):
        e.apply("w", rng.randn(n).astype(np.float32), clip=clip)
    e.check(f"{kind} n={n}")
    if clip > 0:
        top = e.flats["w"][0].abs().max().item()
        assert top <= CLIP and (n < 1003 or top == CLIP), "nothing lies outside the clip, and it binds somewhere"


@pytest.mark.parametrize("which", ["all", "grad_only"])
def test_rmsprop_unaligned_buffers(cuda, which):
    """RMSprop's scalar path: parameters, gradient and slot as ``buf[1:]`` views, or the gradient alone
    (one unaligned pointer is enough to leave the float4 body)."""
    rng = np.random.RandomState(32)
    e = Engines("rmsprop", cuda)
    e.misaligned_grad = True
    e.add("w", _params(rng, 1003, CLIP), misaligned=which == "all")
    assert e.flats["w"][0].data_ptr() % 16 == (4 if which == "all" else 0)
    for step in range(3):
        e.apply("w", rng.randn(1003).astype(np.float32), clip=CLIP)
    e.check(f"rmsprop unaligned {which}")


@pytest.mark.parametrize("gscale", [0.5, 0.125])
@pytest.mark.parametrize("kind", ["rmsprop", "adam", "nadam"])
def test_gscale_and_clip(cuda, kind, gscale):
    """The data-parallel average ``gscale`` on every kind, each under the 0.01 clip (inside the kernel
    for RMSprop and Adam, ``clip_`` after Nadam): nothing ends outside [-c, c], and an element sitting
    exactly on +-c with a zero gradient stays there."""
    n = 1003
    rng = np.random.RandomState(33)
    p0 = _params(rng, n, CLIP).astype(np.float32)
    p0[0], p0[1] = CLIP, -CLIP
    e = Engines(kind, cuda)
    e.add("w", p0)
    for step in range(1, 6):
        g = (rng.randn(n) / gscale).astype(np.float32)
        g[:2] = 0.0
        e.apply("w", g, clip=CLIP, gscale=gscale)
        pg = e.flats["w"][0]
        assert pg.abs().max().item() <= CLIP and pg[0].item() == CLIP and pg[1].item() == -CLIP, f"step {step}"
        if step in (1, 5):
            e.check(f"{kind} gscale={gscale} step {step}")
    assert (e.flats["w"][0].abs() == CLIP).sum().item() > 2, "the clip bound elements other than the two placed on it"


@pytest.mark.parametrize("kind", ["rmsprop", "adam", "nadam"])
def test_edge_gradients(cuda, kind):
    """Step 1 with an all-zero gradient: parameters bitwise unchanged, slots zero, the counter ticks.
    Step 2 mixes exact zeros, 1e-20, 1 and 1e4: the square of 1e-20 is below the fp32 normal range, its
    second moment vanishes against epsilon and the RMSprop update is lr g / epsilon; 1e4 squares to 1e8."""
    n = 1003
    clip = CLIP if kind == "rmsprop" else 0.0
    rng = np.random.RandomState(34)
    p0 = (rng.uniform(-CLIP, CLIP, n) if clip > 0 else rng.randn(n)).astype(np.float32)
    e = Engines(kind, cuda)
    e.add("w", p0)
    e.apply("w", np.zeros(n, dtype=np.float32), clip=clip)
    pg = e.flats["w"][0]
    assert torch.equal(pg.cpu(), torch.from_numpy(p0))
    assert all((s == 0).all().item() for s in e.gpu._slots(pg)) and e.gpu.iterations.item() == 1
    e.check(f"{kind} zero gradient")
    g = np.tile(np.array([0.0, 1e-20, 1.0, 1e4, -1e-20, -1.0, -1e4], dtype=np.float32), n // 7 + 1)[:n]
    e.apply("w", g, clip=clip)
    assert torch.isfinite(pg).all()
    e.check(f"{kind} mixed magnitudes")
    if kind == "rmsprop":  # the reference's own update of the 1e-20 lanes is lr g / eps to fp64 rounding
        h = HYPER[kind]
        moved = e.ref.slots["w"][0][1::7]
        assert np.all(np.sqrt(moved) < 1e-6 * h["epsilon"])


def test_shared_counter(cuda):
    """One Adam object on two buffers in turn (Keras compiles one optimizer into the critic and the
    combined model): ``iterations`` ticks on every apply, so each buffer sees every second bias
    correction; then one ``apply_group`` over both, a single tick."""
    n = 1003
    rng = np.random.RandomState(35)
    e = Engines("adam", cuda)
    e.add("a", rng.randn(n))
    e.add("b", rng.randn(n))
    for k in range(20):
        e.apply("ab"[k % 2], rng.randn(n).astype(np.float32))
        if k in (0, 1, 19):
            assert e.gpu.iterations.item() == k + 1
    e.check("adam shared, 20 applies")
    e.apply_group(["a", "b"], [rng.randn(n).astype(np.float32) for _ in "ab"])
    assert e.gpu.iterations.item() == 21
    e.check("adam shared, apply_group")


# ------------------------------------------------------------------------------------ binding checks
# Every rejected call is harmless even without its check: the odd tensor is the larger one.
def _adam_args(cuda, n=16):
    z = lambda k=n: torch.zeros(k, device=cuda)  # noqa: E731
    return dict(p=torch.ones(n, device=cuda), g=z(), m=z(), v=z(), step=z(1), m_cache=torch.ones(1, device=cuda))


HP = (1e-3, 0.9, 0.999, 1e-7)


@pytest.mark.parametrize("odd", ["g", "m", "v"])
def test_nadam_rejects_size_mismatch(cuda, odd):
    a = _adam_args(cuda)
    a[odd] = torch.zeros(16 + 4, device=cuda)
    with pytest.raises(RuntimeError, match="size mismatch"):
        _ops().nadam_(a["p"], a["g"], a["m"], a["v"], a["step"], a["m_cache"], *HP, 1.0)
    assert (a["p"] == 1).all()


@pytest.mark.parametrize("op,odd", [("adam_", "step"), ("nadam_", "step"), ("nadam_", "m_cache")])
def test_step_counters_must_be_scalars(cuda, op, odd):
    a = _adam_args(cuda)
    a[odd] = torch.ones(2, device=cuda)
    with pytest.raises(RuntimeError, match="one element"):
        if op == "adam_":
            _ops().adam_(a["p"], a["g"], a["m"], a["v"], a["step"], *HP, 0.0, 1.0)
        else:
            _ops().nadam_(a["p"], a["g"], a["m"], a["v"], a["step"], a["m_cache"], *HP, 1.0)
    assert (a["p"] == 1).all() and (a[odd] == 1).all()


@pytest.mark.parametrize("odd", ["step", "m_cache"])
def test_step_advance_rejects_non_scalars(cuda, odd):
    step, cache = torch.zeros(2 if odd == "step" else 1, device=cuda), torch.ones(2 if odd == "m_cache" else 1, device=cuda)
    with pytest.raises(RuntimeError, match="one element"):
        _ops().step_advance_(step, cache, 0.9)
    assert (step == 0).all() and (cache == 1).all()
    if odd == "step":
        with pytest.raises(RuntimeError, match="one element"):
            _ops().step_advance_(step, None, 0.9)
        assert (step == 0).all()
