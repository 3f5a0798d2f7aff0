"""Bitwise A/B of the fp32 LSTM reverse kernels (csrc/lstm_f32.hip) between two builds of the native library.

    python scripts/ab_reverse_f32.py --parent PARENT.so --new NEW.so [--new OTHER.so ...] [--out ab_compare.txt]

Each library is loaded through HFREP_NATIVE_LIB in a fresh child process per (library, (B, T)); the children are
fed the same seeded inputs (CPU generator, seed 77 B + 5 T + act) and run lstmf_bwd (impl 2: with / without dH;
impl 3: plain, HEAD, aH out, HEAD + aH, dH null with / without aH), lstmf_tbwd (plain, HEAD primal / tangent /
both, dH null) and lstmf_tbwd1 (plain, HEAD, HEAD without a factor, seed null) for act 0, 1, 2 at H = 100,
K = 32; the tapes are compared too.  Arrays above 2 M elements travel as the SHA-256 of their bytes.  Stops at
the first child that does not exit cleanly; exit status 0 only if every array is bitwise equal and finite.
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPES = [(1, 1), (33, 1), (41, 5), (70, 24), (256 * 32 + 45, 2)]


def run_case(B, T, out):
    import hfrep  # noqa: F401
    from hfrep.ops import _native
    from hfrep.ops import functional as Fn

    H, K = 100, 32
    dev = torch.device("cuda:0")
    ops = _native.native()
    res = {}
    for act in (0, 1, 2):
        g = torch.Generator().manual_seed(77 * B + 5 * T + act)
        rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        p = dict(x=rn(B, T, K) * 0.5, xd=rn(B, T, K) * 0.3, W=rn(K, 4 * H) * K ** -0.5, b=rn(4 * H) * 0.1,
                 U=rn(H, 4 * H) * H ** -0.5, dH=rn(B, T, H), dHd=rn(B, T, H), d1=rn(B, 1), d2=rn(B, 1), w=rn(T * H))
        d = {k: v.to(dev).contiguous() for k, v in p.items()}
        _, tape = Fn.lstm_layer_fwd(d["x"], d["W"], d["b"], d["U"], act, True)
        _, ttape = Fn.lstm_layer_tfwd(d["xd"], d["W"], tape, d["U"], act)
        assert isinstance(tape, Fn.FTape)
        U, tp, tt = d["U"], tape.t, ttape.t
        res[f"a{act}/tape"], res[f"a{act}/ttape"] = tp, tt
        zah = lambda: torch.zeros(B, T, H, device=dev)  # noqa: E731
        prev = ops.set_lstmf_bwd_impl(2)
        res[f"a{act}/bwd/exact"] = ops.lstmf_bwd(d["dH"], tp, U, act, B, T)
        res[f"a{act}/bwd/exact_null"] = ops.lstmf_bwd(None, tp, U, act, B, T)
        ops.set_lstmf_bwd_impl(3)
        res[f"a{act}/bwd/split"] = ops.lstmf_bwd(d["dH"], tp, U, act, B, T)
        res[f"a{act}/bwd/split_head"] = ops.lstmf_bwd(None, tp, U, act, B, T, d["d1"], d["w"])
        ah = zah()
        res[f"a{act}/bwd/split_ah"] = ops.lstmf_bwd(d["dH"], tp, U, act, B, T, None, None, ah)
        res[f"a{act}/bwd/split_ah.aH"] = ah
        ah2 = zah()
        res[f"a{act}/bwd/split_head_ah"] = ops.lstmf_bwd(None, tp, U, act, B, T, d["d1"], d["w"], ah2)
        res[f"a{act}/bwd/split_head_ah.aH"] = ah2
        res[f"a{act}/bwd/split_null"] = ops.lstmf_bwd(None, tp, U, act, B, T)
        ah3 = zah()
        res[f"a{act}/bwd/split_null_ah"] = ops.lstmf_bwd(None, tp, U, act, B, T, None, None, ah3)
        res[f"a{act}/bwd/split_null_ah.aH"] = ah3
        ops.set_lstmf_bwd_impl(prev)

        def two(name, r):
            res[name + ".dZ"], res[name + ".dZd"] = r

        two(f"a{act}/tbwd/plain", ops.lstmf_tbwd(d["dH"], d["dHd"], tp, tt, U, act, B, T))
        two(f"a{act}/tbwd/head_primal", ops.lstmf_tbwd(None, None, tp, tt, U, act, B, T, d["d1"], None, d["w"]))
        two(f"a{act}/tbwd/head_tangent", ops.lstmf_tbwd(None, None, tp, tt, U, act, B, T, None, d["d2"], d["w"]))
        two(f"a{act}/tbwd/head_both", ops.lstmf_tbwd(None, None, tp, tt, U, act, B, T, d["d1"], d["d2"], d["w"]))
        two(f"a{act}/tbwd/dH_null", ops.lstmf_tbwd(None, d["dHd"], tp, tt, U, act, B, T))
        res[f"a{act}/tbwd1/plain"] = ops.lstmf_tbwd1(d["dH"], ah, tp, tt, U, act, B, T)
        res[f"a{act}/tbwd1/head"] = ops.lstmf_tbwd1(None, ah, tp, tt, U, act, B, T, d["d1"], d["w"])
        res[f"a{act}/tbwd1/head_nofactor"] = ops.lstmf_tbwd1(None, ah, tp, tt, U, act, B, T, None, d["w"])
        res[f"a{act}/tbwd1/seed_null"] = ops.lstmf_tbwd1(None, ah, tp, tt, U, act, B, T)
        torch.cuda.synchronize()

    def pack(v):
        v = v.cpu().contiguous()
        if v.numel() <= 2_000_000:
            return v
        # large arrays travel as a digest of their bytes (equal digests = bitwise equal) + finiteness
        return ("sha256", hashlib.sha256(v.numpy().tobytes()).hexdigest(), bool(torch.isfinite(v).all()), tuple(v.shape))

    torch.save({k: pack(v) for k, v in res.items()}, out)
    print("saved", len(res), "arrays", out, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", nargs=3, metavar=("B", "T", "OUT"), help="child mode: one (B, T) with the loaded library")
    ap.add_argument("--parent")
    ap.add_argument("--new", action="append", default=[])
    ap.add_argument("--out", default="ab_compare.txt")
    a = ap.parse_args()
    if a.case:
        run_case(int(a.case[0]), int(a.case[1]), a.case[2])
        return 0
    libs = {"parent": os.path.abspath(a.parent)}
    for i, p in enumerate(a.new):
        libs["new" if len(a.new) == 1 else f"new{i + 1}"] = os.path.abspath(p)
    for v in libs.values():
        assert os.path.exists(v), v
    log = open(a.out, "w")

    def say(*x):
        s = " ".join(str(y) for y in x)
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    tot = same = 0
    bad, per = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        for B, T in SHAPES:
            got = {}
            for tag, lib in libs.items():
                f = os.path.join(tmp, f"{tag}.pt")
                r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--case", str(B), str(T), f],
                                   env=dict(os.environ, HFREP_NATIVE_LIB=lib), timeout=280, capture_output=True, text=True)
                if r.returncode != 0:
                    say(f"child {tag} B {B} T {T} exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                    return 1
                got[tag] = torch.load(f)
                os.remove(f)
            ref = got["parent"]
            for tag in [t for t in libs if t != "parent"]:
                b = got[tag]
                assert ref.keys() == b.keys()
                n_eq = 0
                for k in sorted(ref):
                    if isinstance(ref[k], tuple):
                        eq = ref[k] == b[k] and ref[k][2]
                    else:
                        eq = torch.equal(ref[k], b[k]) and bool(torch.isfinite(ref[k]).all())
                    tot += 1
                    n_eq += eq
                    same += eq
                    if not eq:
                        bad.append((tag, B, T, k))
                        per.setdefault(tag, {}).setdefault(k.split("/")[1], 0)
                        per[tag][k.split("/")[1]] += 1
                say(f"{tag}: B {B} T {T}: {len(ref)} arrays, {n_eq} bitwise equal and finite")
    say(f"compared {tot} arrays: {same} bitwise equal, {tot - same} different")
    say("different arrays per library and op:", per)
    for x in bad[:60]:
        say("DIFFERENT", x)
    return 0 if tot == same else 2


if __name__ == "__main__":
    sys.exit(main())
