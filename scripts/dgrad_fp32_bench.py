"""fp32 LSTM input gradient dX = dZ W^T (csrc/lstmf_grad.hip), per call: the A/B tool of the op's impls.

impl 1 = lstmf_dgrad_kernel (exact fp32 MFMA), 3 = lstmf_dgrad_s4_kernel (split, every wave every job),
4 = lstmf_dgrad_roles_kernel (split, MFMA / staging wave roles; bitwise equal to 3).  Each case (M, KO, impl)
is timed `--repeats` times (`--iters` calls per repeat between two events) and gives one JSON line with the
minimum, the range of the repeats and the max |difference| against impl 3.  For a library that predates an
impl pass `--impls` without it (an unknown impl runs the default kernel); HFREP_NATIVE_LIB picks the library.

usage: python scripts/dgrad_fp32_bench.py [--M 6291456 12582912] [--KO 100] [--impls 1 3 4] [--repeats 3]
(GPU only)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hfrep  # noqa: E402,F401
from hfrep.ops import _native  # noqa: E402


def timeit(fn, iters):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--M", type=int, nargs="+", default=[6291456, 12582912])
    ap.add_argument("--KO", type=int, nargs="+", default=[100])
    ap.add_argument("--impls", type=int, nargs="+", default=[1, 3, 4])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--label", default=os.environ.get("HFREP_NATIVE_LIB", "default"))
    a = ap.parse_args()
    ops = _native.native()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    for M in a.M:
        dz = torch.randn(M, 400, device=dev, generator=g)
        for KO in a.KO:
            W = torch.randn(KO, 400, device=dev, generator=g) * 0.1
            ref = ops.lstmf_dgrad(dz, W, 3)
            for impl in a.impls:
                x = ops.lstmf_dgrad(dz, W, impl)  # (also the warm-up call)
                diff = (x - ref).abs().max().item()
                del x
                ts = [timeit(lambda: ops.lstmf_dgrad(dz, W, impl), a.iters) for _ in range(a.repeats)]
                t = min(ts)
                print(json.dumps({"op": "lstmf_dgrad", "lib": a.label, "M": M, "KO": KO, "impl": impl,
                                  "min_ms": round(t, 4), "range_ms": [round(min(ts), 4), round(max(ts), 4)],
                                  "repeats_ms": [round(v, 4) for v in ts], "iters": a.iters,
                                  "tflops": round(2.0 * M * 400 * KO / t / 1e9, 1),
                                  "GBs": round(M * (400 + KO) * 4 / t / 1e6, 0),
                                  "maxdiff_vs_impl3": diff}), flush=True)
            del ref
        del dz
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
