"""GANEval's six device metrics (csrc/evalm.hip) against the host path, on one MI355X.

    python scripts/bench_eval.py [--n 32768] [--n-large 262144] [--calls 3] [--out profiles/eval_device/README.md]

ks_test, ACF, lp_dist, kl_div, js_div and Inception_score at (N, T, F) = (--n, 24, 32) on the host path
(``GANEval()``: scipy / numpy / sklearn) and on the device path (``GANEval(device='cuda')``), then the device
path alone at --n-large.  Wall time by the host clock, the device path bracketed by ``torch.cuda.synchronize()``:

* ``host``: one call at the timed size, after a warm-up call at N = 512 (lazy imports; the host formulas have
  no size-dependent set-up);
* ``device, fresh``: a new ``GANEval`` per call, so the time includes the upload of ``real`` and ``fake`` and,
  for the NB metrics, the ``GaussianNB.fit`` on the host; one warm-up call at the timed size, then the mean
  of --calls calls;
* ``device, shared``: the six metrics on ONE instance in run_all's order (one upload per array, one
  ``nb_divergences`` pass for the three NB metrics), beside the sum of the six host times;
* ``op``: the native op alone on resident tensors, by device events (its launches back to back).

``dataset`` is 1000 windows (the reference's size).  The table goes to --out as markdown, one JSON line per
measurement to stdout (kept as ``profiles/eval_device/bench.jsonl``).  A run without a GPU fails.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T, F = 24, 32
METRICS = ["ACF", "Inception_score", "js_div", "kl_div", "ks_test", "lp_dist"]  # run_all's order


def _data(n, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    real = rng.random((n, T, F), dtype=np.float32)  # uniform
    fake = rng.standard_normal((n, T, F), dtype=np.float32)
    np.negative(fake, out=fake)
    np.exp(fake, out=fake)
    fake += 1.0
    np.reciprocal(fake, out=fake)  # sigmoid of a normal
    return real, fake


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--n-large", type=int, default=262144)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "eval_device", "README.md"))
    ap.add_argument("--skip-host", action="store_true", help="device path only (no table of ratios)")
    a = ap.parse_args()

    import numpy as np
    import torch

    import hfrep  # noqa: F401
    from hfrep.eval.gan_eval import GANEval
    from hfrep.ops import functional as Fn

    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on a GPU: none is visible")
    dev = torch.device("cuda", 0)
    names = [f"f{i}" for i in range(F)]
    dataset = np.random.RandomState(3).rand(1000, T, F).astype(np.float32)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    def event_ms(fn, calls):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def on_device(n, m):
        return not (m == "ks_test" and n * T > Fn.KS_MAX_ROWS)

    def ops_alone(real, fake, n):
        """The native ops on resident tensors (ms per call, device events)."""
        from sklearn.naive_bayes import GaussianNB

        r, f = (torch.as_tensor(x, device=dev) for x in (real, fake))
        gnb = GaussianNB().fit(np.transpose(dataset, (0, 2, 1)).reshape(-1, T), np.repeat(np.arange(F), len(dataset)))
        par = [torch.as_tensor(np.ascontiguousarray(p, dtype=np.float64), device=dev)
               for p in (gnb.theta_, gnb.var_, np.log(gnb.class_prior_))]
        out = {"acf_mean": event_ms(lambda: (Fn.acf_mean(r, 17), Fn.acf_mean(f, 17)), a.calls),
               "nb_divergences": event_ms(lambda: Fn.nb_divergences(r, f, *par), a.calls),
               "lp_cols": event_ms(lambda: Fn.lp_cols(r.view(-1, F), f.view(-1, F)), a.calls)}
        if on_device(n, "ks_test"):
            ref = Fn.wdist_ref(r.view(-1, F))
            out["ks_stat"] = event_ms(lambda: Fn.ks_stat(f.view(-1, F), ref), a.calls)
            out["wdist_ref (torch.sort of real)"] = event_ms(lambda: Fn.wdist_ref(r.view(-1, F)), a.calls)
        return out

    def device_side(real, fake, n):
        res = {}
        for m in METRICS:
            if not on_device(n, m):
                res[m] = None
                emit(kind="device_fresh", N=n, metric=m, ms=None, note=f"{n * T} rows > 2^24: the host path runs")
                continue
            call = lambda: getattr(GANEval(real, fake, dataset, names, ["m"], device=dev), m)()  # noqa: E731
            wall(call)
            ts = [wall(call) for _ in range(a.calls)]
            res[m] = (sum(t for t, _ in ts) / len(ts), min(t for t, _ in ts), ts[0][1])
            emit(kind="device_fresh", N=n, metric=m, ms=round(res[m][0], 3), ms_min=round(res[m][1], 3), value=res[m][2])
        todo = [m for m in METRICS if on_device(n, m)]

        def shared():
            ev = GANEval(real, fake, dataset, names, ["m"], device=dev)
            return [getattr(ev, m)() for m in todo]

        wall(shared)
        ts = [wall(shared)[0] for _ in range(a.calls)]
        emit(kind="device_shared", N=n, metrics=todo, ms=round(sum(ts) / len(ts), 3), ms_min=round(min(ts), 3))
        ops = ops_alone(real, fake, n)
        for k, v in ops.items():
            emit(kind="op", N=n, op=k, ms=round(v, 4))
        return res, sum(ts) / len(ts), ops

    real, fake = _data(a.n, 11)
    dres, dshared, dops = device_side(real, fake, a.n)
    hres = {}
    if not a.skip_host:
        small = GANEval(real[:512], fake[:512], dataset, names, ["m"])
        for m in METRICS:
            getattr(small, m)()
            hres[m] = wall(lambda: getattr(GANEval(real, fake, dataset, names, ["m"]), m)())
            emit(kind="host", N=a.n, metric=m, ms=round(hres[m][0], 1), value=hres[m][1])
    del real, fake
    lres = lshared = lops = None
    if a.n_large > 0:
        real, fake = _data(a.n_large, 12)
        lres, lshared, lops = device_side(real, fake, a.n_large)
        del real, fake

    def fmt(v, nd=1):
        return "not on the device" if v is None else f"{v:.{nd}f}"

    lines = ["# GANEval's KS, ACF, Lp and KL / JS / IS metrics on the device", "",
             f"Written by `scripts/bench_eval.py` (its docstring has the method): one MI355X, (T, F) = ({T}, {F}), "
             f"`dataset` 1000 windows, wall time in ms, device times the mean of {a.calls} calls after one warm-up call.",
             "", f"## N = {a.n}: host path against device path", "",
             "| metric | host ms | device ms (fresh instance: upload + metric) | host / device | device value | host value |",
             "|---|---|---|---|---|---|"]
    findings = []
    for m in METRICS:
        h, d = hres.get(m), dres[m]
        ratio = "" if (h is None or d is None) else f"{h[0] / d[0]:.1f}x"
        lines.append(f"| {m} | {fmt(h[0] if h else None)} | {fmt(d[0] if d else None, 2)} | {ratio} | "
                     f"{d[2] if d else ''} | {h[1] if h else ''} |")
        if h is not None and d is not None and d[0] >= h[0]:
            findings.append(f"`{m}` does NOT beat the host path at N = {a.n}: {d[0]:.2f} ms against {h[0]:.2f} ms.")
    if hres:
        lines += ["", f"The six metrics on one instance (one upload per array, one `nb_divergences` pass): "
                  f"{dshared:.1f} ms on the device; the six host calls sum to {sum(v[0] for v in hres.values()):.0f} ms."]
    lines += ["", "Native ops alone on resident tensors (device events, ms per call; `acf_mean` is the pair of calls "
              "for real and fake):", "", "| op | ms |", "|---|---|"] + [f"| {k} | {v:.3f} |" for k, v in dops.items()]
    if lres is not None:
        lines += ["", f"## N = {a.n_large}: device path alone", "", "| metric | device ms (fresh instance) | value |",
                  "|---|---|---|"]
        for m in METRICS:
            d = lres[m]
            lines.append(f"| {m} | {fmt(d[0] if d else None, 2)} | {d[2] if d else ''} |")
            if d is None:
                findings.append(f"`{m}` is not on the device at N = {a.n_large}: {a.n_large * T} rows exceed `ks_stat`'s "
                                "2^24; `GANEval.ks_test` runs the host path there, which this script does not time.")
        lines += ["", f"The metrics that are on the device, on one instance: {lshared:.1f} ms.", "",
                  "| op | ms |", "|---|---|"] + [f"| {k} | {v:.3f} |" for k, v in lops.items()]
    lines += ["", "## Findings", ""] + ([f"- {f}" for f in findings] or ["- Every device metric beats the host path."])
    out = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
