"""Timing of the ("conv", "wgan_gp") training step: the direct conv1d kernels vs the im2col route.

bench.py's flagship is the LSTM model; this script times ``GANTrainer.train_step`` of the temporal-conv
critic model with device events after warm-up, in fp32 and bf16, at the small preset (B = 32, T = 48, F = 36)
and at a large batch (T = 24, F = 32; B = the largest power of two, from --batch down, that fits in memory).
Every repeat builds a fresh trainer; the spread of the repeats' medians is the run-to-run noise.  One JSON
line per (preset, dtype, route).  ``HFREP_CONV_DIRECT=0`` (or a tree without the direct kernels) times
the im2col route, so the same script measures a parent checkout.

    python scripts/bench_conv1d.py                                   # both presets, both dtypes, 5 repeats
    python scripts/bench_conv1d.py --routes direct im2col             # A/B in one process
    python scripts/bench_conv1d.py --presets large --dtypes float32 --repeats 1 --steps 1 --warmup 1   # for a profiler
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hfrep  # noqa: E402,F401
from hfrep.ops import functional as Fn  # noqa: E402
from hfrep.train.gan_trainer import GANConfig, GANTrainer  # noqa: E402

HAS_DIRECT = hasattr(Fn, "conv1d_direct")


def one_repeat(dtype, B, T, F, a, steps):
    dev = torch.device("cuda", 0)
    ds = np.random.RandomState(0).rand(1024, T, F).astype(np.float32)
    tr = GANTrainer(GANConfig(arch="conv", loss="wgan_gp", window=T, features=F, batch_size=B, dtype=dtype), ds, device=dev)
    for _ in range(a.warmup):
        tr.train_step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        tr.train_step()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    rec = tr.losses()
    assert all(np.isfinite(v) for v in rec.values()), rec
    del tr
    torch.cuda.empty_cache()
    return float(np.median(ms))


def time_case(preset, dtype, route, B, T, F, a):
    if route == "direct" and not HAS_DIRECT:
        return None
    os.environ["HFREP_CONV_DIRECT"] = "1" if route == "direct" else "0"
    steps = a.steps if preset == "large" else 10 * a.steps  # (a small iteration is a few ms: more of them per repeat)
    while True:
        try:
            meds = [one_repeat(dtype, B, T, F, a, steps) for _ in range(a.repeats)]
            break
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
            if preset != "large" or B <= 1024:
                raise
            B //= 2  # the large batch: the largest power of two that runs within memory
    return {"model": "conv/wgan_gp", "preset": preset, "dtype": dtype, "route": route, "batch": B, "window": T,
            "features": F, "steps": steps, "warmup": a.warmup, "repeats": a.repeats,
            "ms_per_iter_median": float(np.median(meds)), "ms_per_iter_min": float(min(meds)),
            "ms_per_iter_max": float(max(meds)), "spread_ms": float(max(meds) - min(meds)), "ms_per_iter_repeats": meds}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=65536, help="large preset: the batch to start from")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--presets", nargs="+", default=["small", "large"], choices=["small", "large"])
    ap.add_argument("--routes", nargs="+", default=None, choices=["direct", "im2col"],
                    help="default: the route the environment selects (HFREP_CONV_DIRECT)")
    a = ap.parse_args(argv)
    env_direct = HAS_DIRECT and os.environ.get("HFREP_CONV_DIRECT", "1") != "0"
    routes = a.routes or ["direct" if env_direct else "im2col"]
    for preset in a.presets:
        B, T, F = (32, 48, 36) if preset == "small" else (a.batch, 24, 32)
        for dtype in a.dtypes:
            for route in routes:
                res = time_case(preset, dtype, route, B, T, F, a)
                if res is not None:
                    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
