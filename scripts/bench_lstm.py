"""Microbenchmark of the LSTM v2 recurrent kernels (fwd / tangent fwd / BPTT / tangent reverse).

Times each layer-level op at the flagship shape (H=100, T=24, bf16) and prints one JSON line per op.
Usage: python scripts/bench_lstm.py [--batch 16384] [--K 100] [--iters 10] [--repeats 1] [--only fwd,bwd,tbwd1,...]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hfrep  # noqa: E402,F401
from hfrep.ops import functional as Fn  # noqa: E402


def timeit(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--T", type=int, default=24)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--act", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=1, help="timed repeats per op (one JSON line each)")
    ap.add_argument("--only", default="fwd,tfwd,bwd,tbwd,bwd_dx,tbwd_dx,dgrad")
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    ap.add_argument("--fwd-impl", type=int, default=0, help="fp32: set_lstmf_fwd_impl value (0: the library default)")
    ap.add_argument("--fwd100-impl", type=int, default=0,
                    help="fp32, K = 100: set_lstmf_fwd100_impl value (1 four waves, 2 eight waves; 0: the library default)")
    ap.add_argument("--bwd-impl", type=int, default=0,
                    help="fp32: set_lstmf_bwd_impl value (2 exact, 3 split on four waves, 4 split on eight waves; "
                         "0: the library default)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.bwd_impl:
        from hfrep.ops import _native

        _native.native().set_lstmf_bwd_impl(a.bwd_impl)
    if a.fwd_impl:
        from hfrep.ops import _native

        _native.native().set_lstmf_fwd_impl(a.fwd_impl)
    if a.fwd100_impl:
        from hfrep.ops import _native

        _native.native().set_lstmf_fwd100_impl(a.fwd100_impl)
    B, T, K, H = a.batch, a.T, a.K, 100
    g = torch.Generator(device=dev).manual_seed(0)
    dt = getattr(torch, a.dtype)
    mk = lambda *s, sc=0.5: (torch.randn(*s, device=dev, generator=g) * sc).to(dt)
    x, xd = mk(B, T, K), mk(B, T, K)
    W = torch.randn(K, 4 * H, device=dev, generator=g) * 0.1
    U = torch.randn(H, 4 * H, device=dev, generator=g) * 0.1
    b = torch.zeros(4 * H, device=dev)
    dH, dHd = mk(B, T, H), mk(B, T, H)
    hs, tape = Fn.lstm_layer_fwd(x, W, b, U, a.act, True)
    hds, ttape = Fn.lstm_layer_tfwd(xd, W, tape, U, a.act)
    dZ_ = Fn.lstm_layer_bwd(dH, tape, U, a.act)
    gW, gU, gb = torch.zeros(K, 4 * H, device=dev), torch.zeros(H, 4 * H, device=dev), torch.zeros(4 * H, device=dev)
    ops = {
        "fwd": lambda: Fn.lstm_layer_fwd(x, W, b, U, a.act, True),
        "fwd_notape": lambda: Fn.lstm_layer_fwd(x, W, b, U, a.act, False),
        "tfwd": lambda: Fn.lstm_layer_tfwd(xd, W, tape, U, a.act),
        "bwd": lambda: Fn.lstm_layer_bwd(dH, tape, U, a.act),
        "tbwd": lambda: Fn.lstm_layer_tbwd(dH, dHd, tape, ttape, U, a.act),
        "bwd_dx": lambda: Fn.lstm_layer_bwd(dH, tape, U, a.act, W=W),
        "tbwd_dx": lambda: Fn.lstm_layer_tbwd(dH, dHd, tape, ttape, U, a.act, W=W),
        "dgrad": lambda: Fn.linear_dgrad(dZ_, W),
        "wgrad": lambda: Fn.lstm_wgrad_(x, hs, dZ_, gW, gU, gb),
        "wgrad_tan": lambda: Fn.lstm_wgrad_(x, hs, dZ_, gW, gU, gb, xd, hds, dZ_),
    }
    if a.dtype == "float32":  # the BPTT's other instantiations: in-kernel head adjoint (HEAD), kept h adjoints (AHD)
        hd, hw = torch.randn(B, 1, device=dev, generator=g), torch.randn(T * H, 1, device=dev, generator=g)
        oa = Fn.OuterAdjoint(hd, hw, (B, T, H))
        ops["bwd_head"] = lambda: Fn.lstm_layer_bwd(oa, tape, U, a.act)
        ops["bwd_ah"] = lambda: Fn.lstm_layer_bwd_keep(dH, tape, U, a.act)
        ops["bwd_head_ah"] = lambda: Fn.lstm_layer_bwd_keep(oa, tape, U, a.act)
    if "tbwd1" in a.only.split(","):  # fp32 only: the single-stream tangent reverse, a_hd from a kept BPTT
        ahd = Fn.lstm_layer_bwd_keep(dHd, tape, U, a.act)[2]
        ops["tbwd1"] = lambda: Fn.lstm_layer_tbwd1(dH, ahd, tape, ttape, U, a.act)
    for name in a.only.split(","):
        for _ in range(a.repeats):
            ms = timeit(ops[name], a.iters)
            print(json.dumps({"op": name, "dtype": a.dtype, "B": B, "T": T, "K": K, "act": a.act, "fwd_impl": a.fwd_impl, "fwd100_impl": a.fwd100_impl,
                              "bwd_impl": a.bwd_impl, "ms": round(ms, 4),
                              "us_per_step": round(ms * 1e3 / T, 2)}), flush=True)


if __name__ == "__main__":
    main()
