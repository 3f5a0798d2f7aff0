"""A/B timing of the training step of the MLP WGAN-GP with the LReLU + LayerNorm critic, zoo
("mlp_ln", "wgan_gp"): fused kernels (csrc/mlp_clip.hip mlp_lngp_norm / mlp_lngp_critic) vs the layer-by-layer engine.

bench.py has no entry for this model; this script times ``GANTrainer.train_step`` with device
events after warm-up, for each dtype the fused path first and then the engine path
(``HFREP_MLP_FUSED=0``) in the same process, and prints one JSON line per (dtype, path) plus the ratio.

    python scripts/bench_mlp_ln_gp.py                      # B = 262144, T = 24, F = 32, both dtypes
    python scripts/bench_mlp_ln_gp.py --batch 32 --window 48 --features 36 --steps 50 --warmup 5
    python scripts/bench_mlp_ln_gp.py --paths fused --dtypes bfloat16 --steps 1 --warmup 1   # for a profiler
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hfrep  # noqa: E402,F401
from hfrep.train.gan_trainer import GANConfig, GANTrainer  # noqa: E402


def time_path(dtype: str, fused: bool, a) -> dict:
    os.environ["HFREP_MLP_FUSED"] = "1" if fused else "0"
    dev = torch.device("cuda", 0)
    ds = np.random.RandomState(0).rand(1024, a.window, a.features).astype(np.float32)
    cfg = GANConfig(arch="mlp_ln", loss="wgan_gp", window=a.window, features=a.features, batch_size=a.batch, dtype=dtype)
    tr = GANTrainer(cfg, ds, device=dev)
    assert (tr._fused is not None) == fused, "path selection"
    for _ in range(a.warmup):
        tr.train_step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    ev[0].record()
    for i in range(a.steps):
        tr.train_step()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)]
    rec = tr.losses()
    assert all(np.isfinite(v) for v in rec.values()), rec
    out = {"model": "mlp_ln/wgan_gp", "dtype": dtype, "path": "fused" if fused else "engine", "batch": a.batch,
           "window": a.window, "features": a.features, "steps": a.steps, "warmup": a.warmup,
           "ms_per_iter_median": float(np.median(ms)), "ms_per_iter_min": float(min(ms)),
           "ms_per_iter_max": float(max(ms)), "ms_per_iter": ms, "d_loss": rec["d_loss"], "gp": rec["gp"],
           "g_loss": rec["g_loss"]}
    del tr
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--window", type=int, default=24)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--paths", nargs="+", default=["fused", "engine"], choices=["fused", "engine"])
    a = ap.parse_args(argv)
    for dtype in a.dtypes:
        res = {}
        for path in a.paths:
            res[path] = time_path(dtype, path == "fused", a)
            print(json.dumps(res[path]), flush=True)
        if len(res) == 2:
            print(json.dumps({"dtype": dtype, "engine_over_fused": res["engine"]["ms_per_iter_median"]
                              / res["fused"]["ms_per_iter_median"]}), flush=True)


if __name__ == "__main__":
    main()
