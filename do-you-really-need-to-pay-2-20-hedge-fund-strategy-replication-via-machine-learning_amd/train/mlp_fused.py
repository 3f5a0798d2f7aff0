"""Fused MLP-GAN training steps (BASELINE configs 3 / 4, the clipped MLP WGAN and its LayerNorm critic
under the gradient penalty) on the kernels of ``csrc/mlp_*.hip``.

The layer-by-layer engine (``Sequential.efwd / ebwd / etfwd / etbwd``) runs one kernel per layer and
pass and round-trips every (B*T, 100) activation and adjoint through HBM: 607 GB per bf16 MLP WGAN-GP
iteration (``profiles/r06_mlp/baseline``).  For the four MLP models of the zoo this module replaces it
with one kernel per pass that carries a 32-row tile through every layer in registers:

* ``mlp_gen_fwd``     G(z) (GAN/WGAN_GP.py:221-236, GAN/GAN.py:127-142);
* ``mlp_wgp_norm`` + ``mlp_wgp_coef``   the gradient penalty's first-order pass: |dD/dx_hat| per
  sample and the adjoint coefficient c_b (GAN/WGAN_GP.py:201-216);
* ``mlp_wgp_critic``  a whole WGAN-GP critic update of the linear critic (GAN/WGAN_GP.py:238-253):
  W terms on real / fake and the reverse-over-tangent of the penalty, as one combined weight-gradient
  operand per weight (see the kernel's comment); ``mlp_wgp_critic_t`` also takes the three weight
  gradients in the kernel (rows walked t-major, per-t column sums in registers);
* ``mlp_gan_critic``  a vanilla-GAN discriminator update (GAN/GAN.py:144-158, 187-189);
  ``mlp_gan_critic_g`` takes its gradients in the kernel as dz-weighted column sums (the linear hidden
  layers make every adjoint of a row rank-1);
* ``mlp_critic_dx`` + ``mlp_gen_bwd``  the generator update through the frozen critic
  (GAN/WGAN_GP.py:178-189, GAN/GAN.py:195-198); in bf16 ``mlp_gen_bwd_w`` accumulates all ten
  generator parameter gradients in the kernel;
* ``mlp_wgan_critic``  one update of the clipped WGAN's LReLU + LayerNorm critic (GAN/WGAN.py:147-158,
  loop :166-205) on one batch with its label: forward, rank-1 head adjoint, both LN / LReLU reverses;
  the weight-gradient operands (u1, dz2, dz1) go to ``linear_wgrad_``, the LayerNorm and head gradients
  come from per-wave column-sum slabs; ``mlp_wgan_critic_dx`` is the generator step's dfake through that
  critic (then ``mlp_gen_bwd`` / ``mlp_gen_bwd_w`` as for the other two models);
* ``mlp_lngp_norm`` + ``mlp_lngp_critic``  the gradient penalty of that LReLU + LayerNorm critic (zoo
  ``("mlp_ln", "wgan_gp")``): g = dD/dx_hat per row with its squared norm, then (after ``mlp_wgp_coef``) the
  reverse over the tangent along v = c_b g through both LayerNorms, as two row-stacked (primal; tangent)
  weight-gradient operand pairs for ``linear_wgrad_`` and per-wave slabs for the LayerNorm, head and bias
  gradients; the W terms of that update
  are two ``mlp_wgan_critic`` launches (label -1 on real, +1 on fake);

followed by the streaming weight-gradient kernels (``linear_wgrad_``) and the fused optimizer.  The
random draws are the engine path's, in its order (real, noise, alpha per critic update), so both paths
see the same batches; ``HFREP_MLP_FUSED=0`` selects the engine path (A/B, tests).  When an MLP trainer on
a GPU does not get the fused path, one log line (logger ``hfrep.mlp_fused``) names the reason.

For the affine WGAN-GP critic the penalty's input gradient dD/dx_hat does not depend on x_hat, so
neither x_hat nor D(x_hat) is formed (alpha is still drawn: the RNG stream stays the engine's).  Going
one step further (``mlp_wgp_affine``, default): g_t = W1 W2 w3_t depends on t alone, so every sample has
the same penalty coefficient, and the W terms enter the weight gradients and the losses only through
per-t sums over the batch (sum_b (x_b W) = (sum_b x_b) W).  A critic update then reads real and fake
once (per-t column sums) and finishes in fp32 in one workgroup; the generator step's dfake is -g_t / B
for every row (``mlp_critic_dx_affine``).  ``HFREP_MLP_AFFINE=0`` keeps the per-row kernels above.
"""
from __future__ import annotations

import logging
import os

import torch

from ..models.layers import Dense, Flatten, LayerNormalization, LeakyReLU
from ..ops import _native
from ..ops import functional as Fn


log = logging.getLogger("hfrep.mlp_fused")


def _ops():
    return _native.native()


def _views(model, layer, names, grad=False):
    get = model.gview if grad else model.view
    return [get(layer, n) for n in names]


def _ln_stack_lists(M, hidden_act: int, last_ok, grad=False):
    """[W1, b1, gamma1, beta1, W2, b2, gamma2, beta2, W3, b3] of Dense -> LReLU(0.2) -> LN(1e-3) -> Dense ->
    LReLU(0.2) -> LN(1e-3) -> Dense (every Dense with bias, the first two with activation ``hidden_act``, the
    last one linear and accepted by ``last_ok``), or None if M is not that."""
    L = M.layers
    kinds = [Dense, LeakyReLU, LayerNormalization, Dense, LeakyReLU, LayerNormalization, Dense]
    if len(L) != 7 or not all(isinstance(l, k) for l, k in zip(L, kinds)):
        return None
    if not (L[0].act_code == hidden_act and L[3].act_code == hidden_act and L[6].act_code == 0
            and all(L[i].use_bias for i in (0, 3, 6)) and last_ok(L[6])):
        return None
    if abs(L[1].alpha - 0.2) > 1e-6 or abs(L[4].alpha - 0.2) > 1e-6 or L[2].eps != 1e-3 or L[5].eps != 1e-3:
        return None
    out = []
    for d, ln in ((L[0], L[2]), (L[3], L[5])):
        out += _views(M, d, ["kernel", "bias"], grad) + _views(M, ln, ["gamma", "beta"], grad)
    return out + _views(M, L[6], ["kernel", "bias"], grad)


def _gen_lists(G, grad=False):
    """The MLP generator: sigmoid Dense layers in front of each LReLU -> LN, any output width."""
    return _ln_stack_lists(G, 1, lambda last: True, grad)


def _critic_lists(C, head: int, grad=False):
    """[W1, b1, W2, b2, w3, b3] of Dense -> Dense -> (Flatten ->) Dense(1) with linear hidden layers;
    head 0 = Flatten -> Dense(1) linear, head 1 = per-row Dense(1, sigmoid)."""
    L = C.layers
    if head == 0:
        ok = len(L) == 4 and isinstance(L[2], Flatten) and L[3].act_code == 0
        last = L[3] if ok else None
    else:
        ok = len(L) == 3 and L[2].act_code == 1
        last = L[2] if ok else None
    if not ok or not all(isinstance(l, Dense) and l.use_bias for l in (L[0], L[1], last)):
        return None
    if L[0].act_code != 0 or L[1].act_code != 0 or last.units != 1:
        return None
    return (_views(C, L[0], ["kernel", "bias"], grad) + _views(C, L[1], ["kernel", "bias"], grad)
            + _views(C, last, ["kernel", "bias"], grad))


def _clip_critic_lists(C, grad=False):
    """The clipped WGAN's critic: linear Dense layers, per-row Dense(1) head (no Flatten)."""
    return _ln_stack_lists(C, 0, lambda last: last.units == 1, grad)


# 2: the clip critic (per-row LReLU + LN, W loss); 3: that critic under the gradient penalty
_HEAD = {("mlp", "wgan_gp"): 0, ("mlp", "gan"): 1, ("mlp", "wgan"): 2, ("mlp_ln", "wgan_gp"): 3}


def _critic_of(C, head: int, grad=False):
    return _clip_critic_lists(C, grad) if head in (2, 3) else _critic_lists(C, head, grad)


class FusedMLP:
    """The MLP models' training step on the fused kernels (attached to a GANTrainer)."""

    def __init__(self, tr):
        self.tr = tr
        self.head = _HEAD[(tr.cfg.arch, tr.cfg.loss)]
        self.gw, self.gg = _gen_lists(tr.generator), _gen_lists(tr.generator, grad=True)
        self.cw, self.cg = _critic_of(tr.critic, self.head), _critic_of(tr.critic, self.head, grad=True)
        self._ones = {}
        # GP critic update (both dtypes): rows walked t-major, the weight gradients as per-t column sums
        # in registers (mlp_wgp_critic_t) -- no per-row operands in HBM.  HFREP_MLP_WGRAD_INKERNEL=0 keeps
        # the operand path (mlp_wgp_critic + linear_wgrad_).  The generator reverse: mlp_gen_bwd_w (bf16).
        cfg = tr.cfg
        on = os.environ.get("HFREP_MLP_WGRAD_INKERNEL", "1") != "0"
        inkernel = tr.dtype == torch.bfloat16 and on
        self.wgrad_tsum = self.head == 0 and on
        # affine critic: the update from per-t batch sums (mlp_wgp_affine / mlp_critic_dx_affine)
        self.affine = (self.head == 0 and os.environ.get("HFREP_MLP_AFFINE", "1") != "0"
                       and bool(_ops().mlp_affine_supported(int(cfg.features), int(cfg.window))))
        self.gen_wgrad_inkernel = inkernel
        # GAN discriminator: rank-1 adjoints per row -> gradients as dz-weighted column sums in the
        # kernel (mlp_gan_critic_g, both dtypes); HFREP_MLP_WGRAD_INKERNEL=0 keeps the operand path
        self.gan_colsum = self.head == 1 and on

    @staticmethod
    def decline_reason(tr) -> str | None:
        """Why this trainer does not get the fused path (None: it does)."""
        cfg = tr.cfg
        if (cfg.arch, cfg.loss) not in _HEAD:
            return "not an MLP model of the zoo"
        if tr.device.type != "cuda":
            return "device is not a GPU"
        if os.environ.get("HFREP_MLP_FUSED", "1") == "0":
            return "env switch HFREP_MLP_FUSED=0"
        if tr.dtype not in (torch.float32, torch.bfloat16):
            return f"dtype {tr.dtype} (float32 and bfloat16 only)"
        if _native.fallback_allowed() or not _native.available():
            return "native library not in use"
        if not bool(_ops().mlp_supported(int(cfg.features), int(cfg.hidden))):
            return f"width (F, H) = ({int(cfg.features)}, {int(cfg.hidden)}) not instantiated"
        if _gen_lists(tr.generator) is None or _critic_of(tr.critic, _HEAD[(cfg.arch, cfg.loss)]) is None:
            return "structure mismatch (generator or critic is not the zoo's layer sequence)"
        return None

    @staticmethod
    def supported(tr) -> bool:
        why = FusedMLP.decline_reason(tr)
        if why is None:
            return True
        # one line per trainer, for an MLP model on a GPU only (elsewhere the engine is the expected path)
        if tr.cfg.arch.startswith("mlp") and tr.device.type == "cuda" and not getattr(tr, "_fused_decline_logged", False):
            tr._fused_decline_logged = True
            log.warning("fused MLP path declined for (%s, %s): %s; running the layer-by-layer engine",
                        tr.cfg.arch, tr.cfg.loss, why)
        return False

    def _ones_col(self, n, dtype):
        key = (n, dtype)
        t = self._ones.get(key)
        if t is None:
            t = self._ones[key] = torch.ones((n, 1), dtype=dtype, device=self.tr.device)
        return t

    # ---- generator update through the frozen critic ---------------------------------------------
    def _generator_grads(self, noise, fake):
        tr, ops = self.tr, _ops()
        B = noise.shape[0]
        if self.head == 0:
            if self.affine:
                dfake, slab = ops.mlp_critic_dx_affine(fake, self.cw)
            else:
                dfake, slab = ops.mlp_critic_dx(fake, self.cw, 0, -1.0)
            loss = ops.mlp_finish(slab, None, 1, 1.0 / B, self.cw[5], 0.0)
        elif self.head in (2, 3):
            dfake, slab = ops.mlp_wgan_critic_dx(fake, self.cw)  # slab: sum of -s over the rows
            loss = ops.mlp_finish(slab, None, 2, 1.0 / noise[..., 0].numel(), None, 0.0)
        else:
            dfake, slab = ops.mlp_critic_dx(fake, self.cw, 1, 1.0)
            loss = ops.mlp_finish(slab, None, 2, 1.0 / noise[..., 0].numel(), None, 0.0)
        if self.gen_wgrad_inkernel:
            ops.mlp_gen_bwd_w(noise, dfake, self.gw, self.gg)
            return loss[0:1]
        dz1, u1, dz2, u2, lnslab = ops.mlp_gen_bwd(noise, dfake, self.gw)
        gW1, gb1, gg1, gbe1, gW2, gb2, gg2, gbe2, gW3, gb3 = self.gg
        Fn.linear_wgrad_(noise, dz1, gW1, gb1)
        Fn.linear_wgrad_(u1, dz2, gW2, gb2)
        Fn.linear_wgrad_(u2, dfake, gW3, gb3)
        ops.mlp_slab_sum_(lnslab, int(gg1.numel()), gg1, gbe1, gg2, gbe2)
        return loss[0:1]

    # ---- WGAN-GP (config 4) -----------------------------------------------------------------------
    def _wgp_critic_grads(self, real, fake):
        tr, ops = self.tr, _ops()
        B, T = real.shape[0], real.shape[1]
        if self.affine:
            gW1, _gb1, gW2, _gb2, gw3, _gb3 = self.cg
            slab, e = ops.mlp_wgp_affine(real, fake, self.cw, float(tr.gp_weight), gW1, gW2, gw3)
            return ops.mlp_finish(slab, e, 0, 1.0 / B, self.cw[5], float(tr.gp_weight))
        gsq = ops.mlp_wgp_norm(real, self.cw)
        c, e = ops.mlp_wgp_coef(gsq, float(tr.gp_weight))
        gW1, _gb1, gW2, _gb2, gw3, _gb3 = self.cg
        if self.wgrad_tsum:
            slab = ops.mlp_wgp_critic_t(real, fake, c, self.cw, gW1, gW2, gw3)
            return ops.mlp_finish(slab, e, 0, 1.0 / B, self.cw[5], float(tr.gp_weight))
        X2c, dY2, X1c, dY1, Y3c, slab = ops.mlp_wgp_critic(real, fake, c, self.cw)
        # the W terms' bias gradients cancel (-1/B and +1/B per row pair) and the tangent has none
        Fn.linear_wgrad_(X2c, dY2, gW2, None)
        Fn.linear_wgrad_(X1c, dY1, gW1, None)
        Fn.linear_wgrad_(Y3c.reshape(B, -1), self._ones_col(B, Y3c.dtype), gw3, None)
        return ops.mlp_finish(slab, e, 0, 1.0 / B, self.cw[5], float(tr.gp_weight))

    def _step_wgan_gp(self):
        tr, ops = self.tr, _ops()
        B = tr.cfg.batch_size
        for _ in range(tr.n_critic):
            real, noise = tr._batch(B)
            tr.rng.uniform((B,))  # alpha: drawn for RNG-stream parity (the affine critic needs no x_hat)
            fake = ops.mlp_gen_fwd(noise, self.gw)
            tr._d_acc = self._wgp_critic_grads(real, fake)
            tr._apply(tr.critic)
        # the generator step trains on the last critic update's noise (GAN/WGAN_GP.py:282) with the
        # same generator weights: its fake windows are that update's
        tr._g_acc = self._generator_grads(noise, fake).to(tr._acc)
        tr._apply(tr.generator)

    # ---- clipped WGAN (GAN/WGAN.py) ---------------------------------------------------------------
    def _wgan_critic_grads(self, x, label: float):
        """Accumulate the critic gradient of mean(label * C(x)) over the B*T rows; returns the loss."""
        ops = _ops()
        u1, dz2, dz1, slab = ops.mlp_wgan_critic(x, self.cw, float(label), self.cg)
        gW1, gb1, _gg1, _gbe1, gW2, gb2 = self.cg[:6]
        Fn.linear_wgrad_(x, dz1, gW1, gb1)
        Fn.linear_wgrad_(u1, dz2, gW2, gb2)
        return ops.mlp_finish(slab, None, 2, 1.0 / x[..., 0].numel(), None, 0.0)[0]

    def _step_wgan(self):
        tr, ops = self.tr, _ops()
        B = tr.cfg.batch_size
        for _ in range(tr.n_critic):
            real, noise = tr._batch(B)
            fake = ops.mlp_gen_fwd(noise, self.gw)
            lr_ = self._wgan_critic_grads(real, -1.0).to(tr._acc)
            tr._apply(tr.critic, clip=0.0)
            lf_ = self._wgan_critic_grads(fake, 1.0).to(tr._acc)
            tr._apply(tr.critic, clip=tr.clip)
            tr._d_acc = torch.stack([0.5 * (lr_ + lf_), lr_, lf_, torch.zeros_like(lr_)])
        # the generator step trains on the last critic update's noise (GAN/WGAN.py:205) with the same
        # generator weights: its fake windows are that update's
        tr._g_acc = self._generator_grads(noise, fake).to(tr._acc)
        tr._apply(tr.generator)

    # ---- the LReLU + LayerNorm critic with the gradient penalty ((mlp_ln, wgan_gp)) --------------------
    def _lngp_critic_grads(self, real, fake, alpha):
        """Accumulate the critic gradient of W(real, -1) + W(fake, +1) + lambda GP(x_hat); returns the loss
        pack [total, W real, W fake, GP] (the W terms: means over the B*T rows, as the engine's)."""
        tr, ops = self.tr, _ops()
        B, lam = real.shape[0], float(tr.gp_weight)
        wr = self._wgan_critic_grads(real, -1.0)
        wf = self._wgan_critic_grads(fake, 1.0)
        xh = Fn.interpolate(real, fake, alpha)
        xg, gsq = ops.mlp_lngp_norm(xh, self.cw)  # xg = [x_hat; g]
        c, e = ops.mlp_wgp_coef(gsq, lam)
        # row-stacked primal / tangent operand pairs: one streaming product of 2 B T rows per weight; the bias
        # gradients (primal rows only: z' = u' W has no bias) come from the kernel's column sums
        U, DZ2, DZ1 = ops.mlp_lngp_critic(xg, c, self.cw, self.cg)
        Fn.linear_wgrad_(xg, DZ1, self.cg[0], None)
        Fn.linear_wgrad_(U, DZ2, self.cg[4], None)
        pen = ops.mlp_finish(self._zero_slab(), e, 0, 1.0 / B, None, lam)[3]  # mean_b (|g_b| - 1)^2, fixed order
        return torch.stack([wr + wf + lam * pen, wr, wf, pen])

    def _zero_slab(self):
        t = self._ones.get("zero_slab")
        if t is None:
            t = self._ones["zero_slab"] = torch.zeros((1, 2), dtype=torch.float32, device=self.tr.device)
        return t

    def _step_lngp(self):
        tr, ops = self.tr, _ops()
        B = tr.cfg.batch_size
        for _ in range(tr.n_critic):
            real, noise = tr._batch(B)
            fake = ops.mlp_gen_fwd(noise, self.gw)
            alpha = tr.rng.uniform((B,))
            tr._d_acc = self._lngp_critic_grads(real, fake, alpha).to(tr._acc)
            tr._apply(tr.critic)
        # the generator step trains on the last critic update's noise with the same generator weights: its
        # fake windows are that update's (as the clipped WGAN's step above)
        tr._g_acc = self._generator_grads(noise, fake).to(tr._acc)
        tr._apply(tr.generator)

    # ---- vanilla GAN (config 3) -------------------------------------------------------------------
    def _gan_d_grads(self, x, label: float):
        """Accumulate the discriminator gradient of BCE(D(x), label) (mean over the B*T rows); returns
        the loss."""
        ops = _ops()
        if self.gan_colsum:
            slab = ops.mlp_gan_critic_g(x, self.cw, float(label), self.cg)
            return ops.mlp_finish(slab, None, 2, 1.0 / x[..., 0].numel(), None, 0.0)[0]
        h1, dh2, dh1, h2, dz3, slab = ops.mlp_gan_critic(x, self.cw, float(label))
        gW1, gb1, gW2, gb2, gw3, gb3 = self.cg
        Fn.linear_wgrad_(h1, dh2, gW2, gb2)
        Fn.linear_wgrad_(x, dh1, gW1, gb1)
        Fn.linear_wgrad_(h2, dz3, gw3, gb3)
        return ops.mlp_finish(slab, None, 2, 1.0 / x[..., 0].numel(), None, 0.0)[0]

    def _gan_d_step(self, x, label: float):
        tr = self.tr
        loss = self._gan_d_grads(x, label)
        tr._apply(tr.critic)
        return loss.to(tr._acc)

    def _step_gan(self):
        tr, ops = self.tr, _ops()
        cfg, B = tr.cfg, tr.cfg.batch_size
        real, noise = tr._batch(B)
        fake = ops.mlp_gen_fwd(noise, self.gw)
        lr_ = self._gan_d_step(real, 1.0)
        lf_ = self._gan_d_step(fake, 0.0)
        d = 0.5 * (lr_ + lf_)
        tr._d_acc = torch.stack([d, lr_, lf_, torch.zeros_like(d)])
        noise2 = tr.rng.normal((B, cfg.window, cfg.features), dtype=tr.dtype)
        fake2 = ops.mlp_gen_fwd(noise2, self.gw)
        tr._g_acc = self._generator_grads(noise2, fake2).to(tr._acc)
        tr._apply(tr.generator)

    def train_step(self):
        if self.head == 0:
            self._step_wgan_gp()
        elif self.head == 2:
            self._step_wgan()
        elif self.head == 3:
            self._step_lngp()
        else:
            self._step_gan()
