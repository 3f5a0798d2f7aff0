"""What on-device W-dist tracking costs (train/wdist_tracker.py, csrc/wdist.hip), on one MI355X.

    python scripts/bench_wdist.py [--calls 200] [--iters 150] [--repeats 3] [--parts a,b,c]

One JSON line per measurement, for (N, T, F) = (1000, 48, 35), (1000, 24, 32), (1000, 168, 36) in fp32 and bf16:

* part ``a``: one ``WDistTracker.update`` (generator forward + sort-and-pair kernels + best-so-far selects) by
  device events: 20 warm-up calls, then ``--calls`` timed calls; beside it the generator forward alone and
  the ``ops.functional.wdist`` call alone;
* part ``b``: the path it replaces, by the host clock with the copy inside the timed region:
  ``fake.float().cpu()`` then ``GANEval.wasserstein`` (scipy, one column at a time);
* part ``c``: the reference preset (B = 32, T = 48, F = 35, the iteration replayed by ``GraphedStep`` as in
  scripts/bench_small.py): ms per iteration with ``wdist_every`` in {0, 50, 10}, the three settings
  alternated in one process and repeated ``--repeats`` times so the run-to-run spread is visible.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = [(1000, 48, 35), (1000, 24, 32), (1000, 168, 36)]


def _event_ms(fn, warmup: int, calls: int) -> float:
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--cpu-calls", type=int, default=5)
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--parts", default="a,b,c")
    a = ap.parse_args()
    parts = a.parts.split(",")

    import torch

    import hfrep  # noqa: F401
    from hfrep.data.windows import synthetic_windows
    from hfrep.eval.gan_eval import GANEval
    from hfrep.ops import functional as Fn
    from hfrep.train.gan_trainer import GANConfig, GANTrainer
    from hfrep.train.runner import GraphedStep
    from hfrep.train.wdist_tracker import WDistTracker

    dev = torch.device("cuda", 0)

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    for N, T, F in SHAPES:
        ds = synthetic_windows(N, T, F, seed=7)
        hold = synthetic_windows(N, T, F, seed=1007)
        for dt in a.dtypes.split(","):
            if not ("a" in parts or "b" in parts):
                break
            cfg = GANConfig(arch="lstm", loss="wgan_gp", window=T, features=F, batch_size=32, dtype=dt, seed=123)
            tr = GANTrainer(cfg, ds, device=dev)
            tk = WDistTracker(tr, hold)
            it = [0]

            def update():
                it[0] += 1
                tk.update(it[0])

            if "a" in parts:
                with torch.no_grad():
                    fake = tr.generator.predict(tk.noise).reshape(N * T, F)
                    ms_up = _event_ms(update, 20, a.calls)
                    ms_fw = _event_ms(lambda: tr.generator.predict(tk.noise), 20, a.calls)
                    ms_op = _event_ms(lambda: Fn.wdist(fake, tk.ref_sorted), 20, a.calls)
                emit(part="a", N=N, T=T, F=F, dtype=dt, calls=a.calls, update_ms=round(ms_up, 4),
                     generator_forward_ms=round(ms_fw, 4), wdist_op_ms=round(ms_op, 4), w_dist=tk.values()["w_dist"])
            if "b" in parts:
                names = [f"f{i}" for i in range(F)]
                with torch.no_grad():
                    fake = tr.generator.predict(tk.noise)
                torch.cuda.synchronize()
                times = []
                for _ in range(a.cpu_calls + 1):
                    t0 = time.perf_counter()
                    host = fake.float().cpu().numpy()
                    w = GANEval(hold, host, hold, names, ["m"]).wasserstein()
                    times.append((time.perf_counter() - t0) * 1e3)
                times = times[1:]  # the first call pays the imports' lazy set-up
                emit(part="b", N=N, T=T, F=F, dtype=dt, calls=len(times), cpu_path_ms=round(sum(times) / len(times), 3),
                     cpu_path_ms_min=round(min(times), 3), cpu_path_ms_max=round(max(times), 3), w_dist=w)
            del tr, tk
            torch.cuda.empty_cache()

    if "c" in parts:
        N, T, F = SHAPES[0]
        ds = synthetic_windows(N, T, F, seed=7)
        hold = synthetic_windows(N, T, F, seed=1007)
        for dt in a.dtypes.split(","):
            cfg = GANConfig(arch="lstm", loss="wgan_gp", window=T, features=F, batch_size=32, dtype=dt, seed=123)
            tr = GANTrainer(cfg, ds, device=dev)
            tk = WDistTracker(tr, hold)
            step = GraphedStep(tr, warmup=2)
            for _ in range(5):
                step()
            tk.update(tr.iteration)
            torch.cuda.synchronize()
            for rep in range(a.repeats):
                for every in (0, 50, 10):
                    t0 = time.perf_counter()
                    for k in range(1, a.iters + 1):
                        step()
                        if every and k % every == 0:
                            tk.update(tr.iteration)
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) / a.iters * 1e3
                    emit(part="c", dtype=dt, batch=32, window=T, features=F, graph=True, repeat=rep, wdist_every=every,
                         iters=a.iters, ms_per_iter=round(ms, 3))
            del tr, tk, step
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
