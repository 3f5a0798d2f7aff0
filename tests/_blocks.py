"""Per-block comparison of two copies of one model's flat gradient (a plain helper module, like _spawn.py).

The flat gradient of every model here is dominated by two or three large matrices, so the relative L2 error
of the whole buffer says nothing about the biases, the LayerNorm gamma / beta or one LSTM gate: a block
whose norm is 3 % of the flat norm may be halved under a flat bound of 3e-2.  ``assert_blocks_close`` holds
every parameter tensor, and every gate of every LSTM tensor, to the tolerance on its own.

Blocks are named by position, ``"<layer index>.<layer kind>.<parameter>"`` (``"2.layer_normalization.gamma"``),
gate blocks ``"0.lstm.bias[f]"``: the Keras weight names carry process-wide counters and so differ between
two trainers of one process.

Tolerances (docs/TEST_TOLERANCES.md holds the measurements behind them):

* fp32: 2e-4 per block, the project's fp32-kernel-against-fp64 bound.  The CPU fp32 engine meets it with
  room to spare (per-block errors 7e-8 .. 1e-5, tests/test_blocks.py).
* bf16: ``BF16_BLOCK`` = 5e-2 per block, ``BF16_GLOBAL`` = 1.5e-2 for the flat gradient of the LSTM models.
  Measured on MI355X (r02, profiles/r02_tests/bf16_errors.txt): global 2.7e-3 .. 5.9e-3, worst block
  4.0e-3 .. 2.3e-2 (the generator's first LSTM kernel at T = 168).  The compute is bf16 MFMA with bf16
  activations / tapes against an fp64 reference of the same inputs, so ~1e-2 is the bf16 noise floor; a stale
  or wrong row tile moves these by O(0.1 .. 1).  Where the caller passes the CPU bf16 engine's gradient of
  the same weights and batch (``model_cpu``), a block's bound is max(5e-2, 2 e_cpu), e_cpu that engine's own
  error on the block: the factor 2 covers two bf16 implementations rounding at different points, and is
  never a multiple of the error of the path under test.
* A block whose exact gradient vanishes by cancellation is named by the caller (``vanished``; the complete
  lists per zoo key are in ``VANISHED``) and held to ``tol * scales[name]``, the scale being the norm of the
  block's fp64 gradient from the real half's Wasserstein term alone (``wasserstein_half_scales``): the
  magnitude of the terms that cancel.  No block leaves the relative check by a threshold.
"""
import dataclasses

import numpy as np
import torch

BF16_GLOBAL, BF16_BLOCK = 1.5e-2, 5e-2
TOL_BLOCK = {"float32": 2e-4, "bfloat16": BF16_BLOCK}
GATES = "ifco"

_LN_CRITIC = ("5.layer_normalization.beta", "6.dense.bias")
# critic blocks whose exact gradient in one whole update is zero (tests/test_blocks.py pins the lists against
# the fp64 engine).  (mlp, wgan_gp): the critic is affine in x, so the penalty sees no bias, and the
# Wasserstein terms' score gradients (-1/B on the real rows, +1/B on the fake rows) sum to zero on every
# bias.  The other heads: the score is h . w + b, so b gets sum_r ds_r = 0; the last LayerNorm's beta enters
# the score the same way (s = (gamma xh + beta) . w + b).  No generator block and no gan / wgan critic
# block (one label per update) vanishes.
VANISHED = {
    ("mlp", "wgan_gp"): ("0.dense.bias", "1.dense.bias", "3.dense.bias"),
    ("lstm", "wgan_gp"): ("3.dense.bias",),
    ("conv", "wgan_gp"): ("3.dense.bias",),
    ("lstm_ln", "wgan_gp"): _LN_CRITIC,
    ("mlp_ln", "wgan_gp"): _LN_CRITIC,
}


def _dtype_name(dtype):
    return dtype if isinstance(dtype, str) else {torch.float32: "float32", torch.bfloat16: "bfloat16"}[dtype]


def blocks(model):
    """[(name, offset, shape, column slice or None)]: every parameter spec of every layer, then the four
    gate column blocks of each LSTM parameter."""
    out = []
    for li, lay in enumerate(model.layers):
        for sp in lay.specs:
            name = f"{li}.{lay.kind}.{sp.name}"
            out.append((name, sp.offset, tuple(sp.shape), None))
            if lay.kind == "lstm":
                H = sp.shape[-1] // 4
                out += [(f"{name}[{g}]", sp.offset, tuple(sp.shape), slice(k * H, (k + 1) * H))
                        for k, g in enumerate(GATES)]
    return out


def _flat(model, grad):
    g = model.flat.grad if grad is None else grad
    return g.detach().double().cpu().reshape(-1)


def _take(flat, off, shape, cols):
    v = flat[off:off + int(np.prod(shape))].view(shape)
    return v if cols is None else v[..., cols]


def block_norms(model, grad=None):
    """{block name: L2 norm of the block of ``grad`` (default: the model's flat gradient)}."""
    flat = _flat(model, grad)
    return {name: _take(flat, off, shape, cols).norm().item() for name, off, shape, cols in blocks(model)}


def block_errors(model_got, model_ref, got=None, ref=None):
    """(flat relative L2 error, [(name, ||got - ref||, ||ref||)] per block) of two flat gradients of one
    model: the models' own ``flat.grad`` or the flat tensors ``got`` / ``ref``."""
    a, b = _flat(model_got, got), _flat(model_ref, ref)
    assert a.shape == b.shape and [x[:3] for x in blocks(model_got)] == [x[:3] for x in blocks(model_ref)]
    rows = [(name, (_take(a, off, shape, cols) - _take(b, off, shape, cols)).norm().item(),
             _take(b, off, shape, cols).norm().item()) for name, off, shape, cols in blocks(model_ref)]
    return ((a - b).norm() / max(b.norm().item(), 1e-300)).item(), rows


def wasserstein_half_scales(trainer, real, names):
    """{name: norm of the block's gradient from the real half's Wasserstein term alone} on ``trainer`` (the
    fp64 engine): efwd, gan_loss(kind 0, label -1), ebwd.  The critic's flat gradient is left as found."""
    from hfrep.ops import functional as Fn

    C = trainer.critic
    keep = C.flat.grad.clone()
    with torch.no_grad():
        C.zero_grad()
        s, tape = C.efwd(real, save=True)
        _, ds = Fn.gan_loss(s, s.numel(), -1.0, -1.0, 0)
        C.ebwd(tape, ds)
        norms = block_norms(C)
        C.flat.grad.copy_(keep)
    return {n: norms[n] for n in names}


def cpu_twin(trainer, dtype):
    """A CPU trainer of ``trainer``'s configuration in ``dtype`` with its weights: "float64" is the reference
    engine, "bfloat16" the CPU bf16 engine whose per-block error e_cpu sets the max(5e-2, 2 e_cpu) bound."""
    from hfrep.train.gan_trainer import GANTrainer

    pd = torch.float64 if dtype == "float64" else torch.float32
    tw = GANTrainer(dataclasses.replace(trainer.cfg, dtype=dtype), trainer.dataset.cpu(), param_dtype=pd)
    with torch.no_grad():
        tw.generator.flat.copy_(trainer.generator.flat.detach().to("cpu", pd))
        tw.critic.flat.copy_(trainer.critic.flat.detach().to("cpu", pd))
    return tw


def _table(flat, flat_tol, rows, total):
    lines = [f"flat rel {flat:.3e} (bound {flat_tol:.3e})" if flat_tol is not None else f"flat rel {flat:.3e}",
             f"{'block':<44}{'|got-ref|':>11}{'bound':>11}{'of bound':>10}{'|ref|/flat':>12}  rule"]
    for name, err, bound, share, rule in sorted(rows, key=lambda r: -r[1] / max(r[2], 1e-300)):
        lines.append(f"{name:<44}{err:>11.3e}{bound:>11.3e}{err / max(bound, 1e-300):>10.2f}"
                     f"{share / max(total, 1e-300):>12.3e}  {rule}")
    return "\n".join(lines)


def assert_blocks_close(model_got, model_ref, dtype, vanished=(), scales=None, label="", *, flat_tol=None,
                        tol_block=None, model_cpu=None, got=None, ref=None, cpu=None, verbose=True):
    """Every block of ``model_got``'s flat gradient against ``model_ref``'s (fp64).

    Ordinary block: ||got - ref|| <= bound ||ref||, bound = ``tol_block`` (default by ``dtype``: 2e-4 fp32,
    5e-2 bf16), raised to 2 e_cpu where ``model_cpu`` (the CPU bf16 engine's gradient of the same weights
    and batch) is given and its own error e_cpu on the block is larger than half of it.  A block named in
    ``vanished``: ||got - ref|| <= tol_block * scales[name] (see ``wasserstein_half_scales``).  ``flat_tol``:
    the calling test's bound on the flat relative error, asserted (strictly) as before.  ``got`` / ``ref`` /
    ``cpu``: flat gradients to read instead of the models' own ``flat.grad``.  On failure the message lists
    every block, the worst first: absolute error, the bound on it, the block's share of the flat norm and
    the rule applied.  Returns (flat relative error, {name: error relative to its scale})."""
    tol = TOL_BLOCK[_dtype_name(dtype)] if tol_block is None else tol_block
    flat, rows = block_errors(model_got, model_ref, got, ref)
    names = [r[0] for r in rows]
    vanished, scales = tuple(vanished), dict(scales or {})
    unknown = [n for n in vanished if n not in names]
    assert not unknown, f"vanished blocks not in the model: {unknown}"
    missing = [n for n in vanished if n not in scales]
    assert not missing, f"vanished blocks without a scale: {missing}"
    e_cpu = {}
    if model_cpu is not None:
        e_cpu = {n: e / max(r, 1e-300) for n, e, r in block_errors(model_cpu, model_ref, cpu, ref)[1]}
    total = _flat(model_ref, ref).norm().item()
    out, rel, bad = [], {}, []
    for name, err, rn in rows:
        if name in vanished or any(name.startswith(v + "[") for v in vanished):
            base = name.split("[")[0]
            bound, rule = tol * scales[base], f"vanished: {tol:.1e} x |g_half| {scales[base]:.3e}"
            rel[name] = err / max(scales[base], 1e-300)
        else:
            t, rule = tol, f"{tol:.1e} x |ref|"
            if 2.0 * e_cpu.get(name, 0.0) > tol:
                t, rule = 2.0 * e_cpu[name], f"2 e_cpu, e_cpu {e_cpu[name]:.3e}"
            bound = t * rn
            rel[name] = err / max(rn, 1e-300)
        out.append((name, err, bound, rn, rule))
        if not err <= bound:
            bad.append(name)
    flat_bad = flat_tol is not None and not flat < flat_tol
    text = _table(flat, flat_tol, out, total)
    if verbose:
        worst = max(out, key=lambda r: r[1] / max(r[2], 1e-300))
        print(f"[{label}] flat rel {flat:.3e}; worst block {worst[0]}: rel {rel[worst[0]]:.3e}, "
              f"{worst[1] / max(worst[2], 1e-300):.2f} of its bound ({worst[4]})")
        for name, err, bound, rn, rule in out:
            if rule.startswith(("2 e_cpu", "vanished")):
                print(f"    {name}: rel {rel[name]:.3e}, {err / max(bound, 1e-300):.2f} of its bound ({rule})")
    assert not bad and not flat_bad, f"{label}: blocks over their bound: {bad}; flat over its bound: {flat_bad}\n{text}"
    return flat, rel
