"""Time AE.metrics_many: the device evaluation (csrc/ae_eval.hip) against the host path.

The host path (``HFREP_AE_METRICS_DEVICE=0``: host windows with refit scalers, one batched
``autoencoder.predict`` on the GPU, numpy metrics per window) is what every AE's ``model_*`` methods do.
Both variants run alternated in this one process, after a warm-up of each, with a device synchronise
around every timed region; the device variant runs three times in a row per repetition (see ``ab``).

* daily ETF panel, test half, latents 1..21, fp32 and bf16, ``oos_stride`` 21 and 1.  At stride 1 the
  host path is timed on the k = 7 autoencoder alone unless ``--host-full`` (it builds ~1.2 GB of scaled
  windows per autoencoder);
* the 30-seed monthly sweep (630 autoencoders, 167 windows each).

Writes ``ae_metrics_bench.json`` into ``--out`` (default profiles/ae_metrics_device).  ``--device-only``
runs nothing but the daily stride-1 fp32 device evaluation (a profiler's target).
"""
import argparse
import json
import lzma
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stage_golden():
    """The reference dataset from tests/golden/reference (xz-packed CSVs unpacked), unless one is staged."""
    if os.environ.get("HFREP_DATA_ROOT"):
        return
    golden = os.path.join(ROOT, "tests", "golden", "reference")
    root = tempfile.mkdtemp(prefix="hfrep_ref_")
    for d, _, files in os.walk(golden):
        out = os.path.join(root, os.path.relpath(d, golden))
        os.makedirs(out, exist_ok=True)
        for f in files:
            src = os.path.join(d, f)
            if f.endswith(".xz"):
                with lzma.open(src) as fh, open(os.path.join(out, f[:-3]), "wb") as oh:
                    oh.write(fh.read())
            else:
                os.symlink(src, os.path.join(out, f))
    os.environ["HFREP_DATA_ROOT"] = root


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ae_metrics_device"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-full", action="store_true", help="time the host path on all 21 latents at stride 1")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--skip-monthly", action="store_true")
    a = ap.parse_args()
    _stage_golden()
    import numpy as np
    import torch

    import hfrep  # noqa: F401
    from hfrep.data.io import load_cleaned, load_daily_etf
    from hfrep.finance.autoencoder_replication import AE

    import hfrep.finance.autoencoder_replication as ar

    dev = torch.device("cuda", 0)

    class TimedOps:
        """torch.ops.hfrep with every op call timed to completion (synchronise before and after): splits a
        device call's wall time into its kernels (``ae_window_table``, ``ae_recon_metrics``) and the rest
        (hashing and uploading the panels, the work list, the download)."""

        def __init__(self, ops):
            self.ops, self.t = ops, {}

        def __getattr__(self, name):
            f = getattr(self.ops, name)

            def g(*args, **kw):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = f(*args, **kw)
                torch.cuda.synchronize()
                self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0
                return r
            return g

    ops = TimedOps(ar._native.native())
    real_native = ar._native.native
    split = []  # per device call: (wall seconds, seconds inside each op)

    def timed(aes, device_path: bool):
        os.environ["HFREP_AE_METRICS_DEVICE"] = "1" if device_path else "0"
        for x in aes:
            x._oos_cache = None  # (the host path's cached predictions)
            x._metrics_cache = None
        ops.t = {}
        ar._native.native = (lambda: ops) if device_path else real_native
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            res = AE.metrics_many(aes)
        finally:
            ar._native.native = real_native
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if device_path:
            split.append((dt, {k: v for k, v in ops.t.items() if k.startswith("ae_") and k != "ae_fit_supported"}))
        return dt, res

    def ab(aes_dev, aes_host, reps):
        """Alternated timings (seconds, minimum and all) after one warm-up of each variant."""
        td, th = [], []
        del split[:]
        _, rd = timed(aes_dev, True)
        _, rh = timed(aes_host, False)
        for _ in range(reps):
            # three device calls back to back: the first follows the host variant's seconds of host-side
            # work, during which the GPU sat idle; the next two show the call on a busy device, which is
            # how a study meets it (right after the fits)
            td.append([timed(aes_dev, True)[0] for _ in range(3)])
            th.append(timed(aes_host, False)[0])
        slow = max(split[1:], key=lambda s: s[0])  # (the warm-up aside) the slowest device call and where it went
        return {"device_s": min(min(t) for t in td), "device_first_after_host_s": min(t[0] for t in td),
                "device_first_after_host_max_s": max(t[0] for t in td), "host_s": min(th), "device_all": td,
                "host_all": th, "slowest_device_call": {"wall_s": slow[0], "in_ops_s": slow[1]}}, rd, rh

    def fmas(aes):
        return float(sum(2 * x._x_train.shape[1] * x._latent_dim * (len(x._x_train) + sum(x._oos_ends())) for x in aes))

    def gap(rd, rh):
        """Largest |device - host| over the AEs' mean OOS r2 and IS r2."""
        return {"max_abs_diff_mean_OOS_r2": max(abs(np.mean(d["OOS_r2"]) - np.mean(h["OOS_r2"])) for d, h in zip(rd, rh)),
                "max_abs_diff_IS_r2": max(abs(d["IS_r2"] - h["IS_r2"]) for d, h in zip(rd, rh))}

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "daily": [], "monthly": None}
    daily = load_daily_etf()[0].to_numpy(np.float64)
    n = len(daily) // 2
    x_tr, x_te = daily[:n], daily[n:]
    for dt in (torch.float32,) if a.device_only else (torch.float32, torch.bfloat16):
        aes = [AE(x_tr, x_tr, x_te, x_te, k, device=dev, dtype=dt, seed=123, oos_stride=1) for k in range(1, 22)]
        AE.train_many(aes)
        if a.device_only:
            timed(aes, True)
            t, _ = timed(aes, True)
            print(json.dumps({"daily_stride1_fp32_device_s": t, "fma": fmas(aes)}))
            return
        for stride in (21, 1):
            for x in aes:
                x.oos_stride = stride
            host = aes if (stride > 1 or a.host_full) else [x for x in aes if x._latent_dim == 7]
            r, rd, rh = ab(aes, host, a.reps)
            r.update(dtype=str(dt), stride=stride, test_rows=len(x_te), windows=len(aes[0]._oos_ends()), aes_device=len(aes),
                     aes_host=len(host), fma_device=fmas(aes))
            if len(host) != len(aes):  # the like-for-like pair: the device path on the host's AEs
                r["device_s_on_host_aes"] = min(timed(host, True)[0] for _ in range(a.reps))
                rd = [d for d, x in zip(rd, aes) if x._latent_dim == 7]
            r.update(gap(rd, rh))
            print(json.dumps(r), flush=True)
            out["daily"].append(r)
    if not a.skip_monthly:
        c = load_cleaned()
        etf, hfd = c["factor_etf_data"], c["hfd"]
        h = len(etf) // 2
        aes = [AE(etf.iloc[:h].to_numpy(), hfd.iloc[:h].to_numpy(), etf.iloc[h:], hfd.iloc[h:], k, device=dev, seed=s)
               for s in range(1, 31) for k in range(1, 22)]
        AE.train_many(aes)
        r, rd, rh = ab(aes, aes, a.reps)
        r.update(dtype="torch.float32", aes=len(aes), windows=len(aes[0]._oos_ends()), fma_device=fmas(aes))
        r.update(gap(rd, rh))
        print(json.dumps(r), flush=True)
        out["monthly"] = r
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ae_metrics_bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
