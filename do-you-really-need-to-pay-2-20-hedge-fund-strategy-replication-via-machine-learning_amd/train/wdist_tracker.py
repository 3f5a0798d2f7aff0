"""W-dist of a fixed generated sample against fixed held-out real windows, tracked on the device
during training, with a device-side copy of the best generator so far.

The project's quality metric (``GAN_eval.wasserstein``) exists in the reference only
after a run, on the CPU; GAN training is not monotone, and the reference author picked one of many
timestamped generators by hand (GAN/trained_generator/old/*.h5).  :class:`WDistTracker` evaluates the
metric inside the loop without stalling it:

* set-up sorts the real sample once (``torch.sort``, outside the loop) and draws the evaluation noise
  once from its OWN random stream -- the draw ``GANTrainer.generate(N, seed=cfg.seed + 7)`` makes on
  rank 0 for ``N <= 4096`` -- so the training stream does not move (bitwise resume and determinism are
  unaffected) and a tracked value at the last iteration is ``hfrep parity``'s ``w_fake_vs_real``;
* :meth:`update` runs the generator forward on that noise and ``ops.functional.wdist`` (the native
  sort-and-pair kernel on the GPU), then selects best-so-far value / iteration / weights with
  ``torch.where``: stream-ordered, no ``.item()``, no host synchronise;
* :meth:`tensors` rides on the runner's deferred snapshots (``utils.logger.AsyncScalars``).

Under data parallelism every rank evaluates the same noise (stream 10 000) with the same
parameters, so all ranks hold the same values and no collective is needed.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import functional as Fn
from ..utils.rng import DeviceRNG

MAX_WINDOWS = 4096  # GANTrainer.generate draws larger samples in several batches


class _BestWeights:
    """The generator's layout over another flat buffer: what ``utils.checkpoint.save_generator`` reads."""

    def __init__(self, model, flat):
        self.model, self.flat = model, flat

    def named_weights(self):
        out = []
        for layer in self.model.layers:
            for s in layer.specs:
                n = int(np.prod(s.shape))
                out.append((s.keras, self.flat[s.offset:s.offset + n].view(s.shape)))
        return out

    def get_weights(self):
        return [v.detach().cpu().numpy().copy() for _, v in self.named_weights()]


class WDistTracker:
    def __init__(self, trainer, real, n: int | None = None, noise_seed: int | None = None):
        if isinstance(real, np.ndarray):
            real = torch.from_numpy(np.ascontiguousarray(real, dtype=np.float32))
        cfg = trainer.cfg
        if real.dim() != 3 or tuple(real.shape[1:]) != (cfg.window, cfg.features):
            raise ValueError(f"real windows {tuple(real.shape)} are not (N, {cfg.window}, {cfg.features})")
        N = int(real.shape[0] if n is None else n)
        if not 1 <= N <= real.shape[0]:
            raise ValueError(f"n = {N} outside 1 .. {real.shape[0]} (the real windows given)")
        if N > MAX_WINDOWS:
            raise ValueError(f"n = {N} > {MAX_WINDOWS}: GANTrainer.generate batches its noise differently there, "
                             "and the tracked value would not be the one it reproduces")
        self.trainer, self.N, self.T, self.F = trainer, N, cfg.window, cfg.features
        dev = trainer.device
        self.ref_sorted = Fn.wdist_ref(real[:N].to(dev, torch.float32).reshape(N * self.T, self.F))  # (F, N T), once
        self.noise_seed = cfg.seed + 7 if noise_seed is None else int(noise_seed)
        self.noise = DeviceRNG(self.noise_seed, dev, stream=10_000).normal((N, self.T, self.F), dtype=trainer.dtype)
        # [w_last, best_w, best_iteration]: one tensor, so the snapshot copies it as it is
        self._w = torch.tensor([float("nan"), float("inf"), -1.0], dtype=torch.float64, device=dev)
        self._it = torch.zeros((), dtype=torch.float64, device=dev)
        self.best_flat = trainer.generator.flat.detach().clone()

    # ---- the loop's call ------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, iteration: int) -> None:
        """Evaluate the current generator and keep it if it is the best so far (NaN compares false).
        ``iteration`` is a host value: a captured update replays the one it was captured with."""
        flat = self.trainer.generator.flat.detach()
        fake = self.trainer.generator.predict(self.noise)
        w = Fn.wdist(fake.reshape(self.N * self.T, self.F), self.ref_sorted)
        cur, best_w, best_it = w[self.F], self._w[1], self._w[2]
        better = cur < best_w
        self._it.fill_(float(iteration))
        torch.where(better, flat, self.best_flat, out=self.best_flat)
        torch.where(better, self._it, best_it, out=best_it)
        torch.where(better, cur, best_w, out=best_w)
        self._w[0].copy_(cur)

    def tensors(self) -> dict:
        """For ``AsyncScalars.snapshot``: ``w`` = [w_last, best_w, best_iteration]."""
        return {"w": self._w}

    # ---- checkpoint -----------------------------------------------------------------------------
    def state_dict(self) -> dict:
        return {"w": self._w.detach().cpu(), "best_flat": self.best_flat.detach().cpu(),
                "noise_seed": torch.tensor(self.noise_seed), "n": torch.tensor(self.N)}

    def load_state_dict(self, st: dict) -> None:
        if int(st["n"]) != self.N or int(st["noise_seed"]) != self.noise_seed:
            raise ValueError(f"tracker state of (n, noise_seed) = ({int(st['n'])}, {int(st['noise_seed'])}) does not "
                             f"continue this tracker's ({self.N}, {self.noise_seed})")
        with torch.no_grad():
            self._w.copy_(st["w"].to(self._w))
            self.best_flat.copy_(st["best_flat"].to(self.best_flat))

    # ---- after training (these may synchronise) ---------------------------------------------------
    def values(self) -> dict:
        w = self._w.detach().cpu().tolist()
        return {"w_dist": w[0], "w_best": w[1], "w_best_iteration": int(w[2])}

    def best_generator_weights(self) -> list:
        """The best generator's weights in Keras ``get_weights`` order."""
        return _BestWeights(self.trainer.generator, self.best_flat).get_weights()

    def save_best(self, path: str, config: dict) -> str:
        from ..utils.checkpoint import save_generator

        return save_generator(path, _BestWeights(self.trainer.generator, self.best_flat), config)
