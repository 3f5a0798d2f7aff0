"""Inputs, per-element error budgets and shape tables of the Dense kernels, shared by
tests/test_dense_routes_gpu.py (the kernels) and tests/test_dense_shapes.py (the CPU-only check that these
inputs can see an edge error).

Conventions (those of the tensor-free op ``dense_route(op, bf16, M, K, N, shiftT)``):

* ``linear``:        y (M, N) = act(x (M, K) W (K, N) + b)
* ``linear_dgrad``:  dx (M, N) = dz (M, K) W^T, W stored (N, K): K is the reduction length here too
* ``linear_wgrad_``: gW (K, N) += xe (M, K)^T dz (M, N), gb (N) += colsum dz; xe = x, or with shiftT > 0
  row m - 1 of x, and zeros where m % shiftT == 0
* ``linear_head_cs``: y (M, 1) = x (M, K) W + b, gW += x^T d, gb += sum d with d_r = wa (r < split) / wb

Budgets.  u16 = 2^-8, u32 = 2^-24; the reference is fp64 from the operands as the kernel receives them.

* forward / dgrad, fp32:  (K + 2) u32 S + floor,  S = |x| @ |W| + |b|: K products, K - 1 adds, the bias add
  and the activation, each one rounding of a partial sum that S bounds.
* forward / dgrad, bf16:  u16 S + u16 |y_ref| + (K + 2) u32 S + floor: the MFMA routes round W to bf16
  (first term), every route rounds the stored output (second term); every activation is 1-Lipschitz.
* weight gradient, both dtypes:  (2 M + 8) u32 S + 2 u32 |g_ref|,  S = |xe|^T |d|: products of bf16 operands
  are exact in fp32, so only the fp32 accumulation over M rows (slab sums and their reduce: at most 2 M
  roundings), the three dropped cross terms of the fp32 three-term split and the product rounding of the
  exact kernels (the + 8), and the final add into the accumulator (the |g_ref| term) contribute.
  gb: the same with xe = 1.
* floor: 0 for act = 0, TOL[float32]["atol"] otherwise (the activations' fast exp / divide).

These are worst-case bounds without a slack factor.
"""
import numpy as np
import torch

U16, U32 = 2.0 ** -8, 2.0 ** -24
ACT_FLOOR = 2e-5  # == test_kernels_gpu.TOL[torch.float32]["atol"] (asserted in tests/test_dense_shapes.py)
F32, BF = torch.float32, torch.bfloat16
MI355X_CUS = 256

# the k step of each forward / dgrad route: the granularity at which it could lose a partial k-group
K_STEP = {"skinny": 8, "narrowf": 4, "widef": 16, "narrow": 16, "linear2": 32, "linear": 32}


def family(route):
    return route.split("<")[0]


# ------------------------------------------------------------------------------------------ inputs
def _push(t, by=0.5):
    """Push values away from zero by ``by``, sign kept."""
    return t + torch.where(t >= 0, by, -by)


def dense_inputs(M, K, N, seed=0):
    """x (M, K), W (K, N), b (N) in fp32 with heavy reduction edges: rows 0 and K - 1 of W are pushed away
    from zero and scaled by (K - 1) / 2, so that each edge column of the reduction carries about as much
    of S = |x| @ |W| as all the columns between them together (the bf16 budget is proportional to S, which
    grows like K, not sqrt(K)); the matching columns of x are pushed away from zero, and the bias of the last
    output column is pushed away from zero and scaled with sqrt(K).  The input gradient uses W^T (N, K) and no bias."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(M, K, generator=g) * 0.5
    W = torch.randn(K, N, generator=g) * (1.0 / K ** 0.5)
    b = torch.randn(N, generator=g) * 0.1
    for k in {0, K - 1}:
        x[:, k] = _push(x[:, k])
        W[k] = _push(W[k], 0.5 / K ** 0.5) * max(1.0, (K - 1) / 2)
    b[N - 1] = _push(b[N - 1], 1.0) * max(1.0, K ** 0.5 / 4)  # (the bf16 budget grows with S ~ sqrt(K) here)
    return x, W, b


def wgrad_split_starts(route, M, K, N, cus=MI355X_CUS):
    """First rows of the M-splits (all but the first) of the weight-gradient route: mirrors the launchers'
    split arithmetic (gemm.hip wgrad_splits / wgrad_f32s_splits, skinny.hip launch_skinny_wgrad).  Only used
    to put heavy rows there."""
    fam = family(route)
    if fam == "skinny":
        splits = max(1, min(512, (M + 63) // 64))
        rps = (M + splits - 1) // splits
    elif fam == "wgrad_f32s":
        p = max(1, min((M + 1023) // 1024, 2 * cus))
        rps = ((M + p - 1) // p + 31) // 32 * 32
    else:
        tiles = ((K + 1 + 63) // 64) * ((N + 63) // 64)
        splits = max(1, min((M + 2047) // 2048, max(1, 2048 // tiles)))
        rps = ((M + splits - 1) // splits + 31) // 32 * 32
    return list(range(rps, M, rps))


def heavy_rows(route, M, K, N, shiftT, cus=MI355X_CUS):
    rows = {0, M - 1}
    if (M // 32) * 32 < M:
        rows.add((M // 32) * 32)  # the first row after the last full 32-row chunk
    rows.update(wgrad_split_starts(route, M, K, N, cus))
    if 1 < shiftT:
        rows.update(range(0, M, shiftT))  # (shiftT = 1: every row is a window start, nothing to single out)
    return sorted(rows)


def heavy_factor(M):
    """A dropped heavy row moves an element by ~h against a budget of ~2 M u32 (M + n h): h = 8 + M / 64
    keeps that above 3x for the M of the weight-gradient table (<= 2113 rows; tests/test_dense_shapes.py)."""
    return 8.0 + M / 64.0


def wgrad_inputs(route, M, K, N, shiftT, seed=0, cus=MI355X_CUS):
    """x (M, K), dz (M, N), and non-zero accumulators gW0 (K, N), gb0 (N); the heavy rows of dz are scaled."""
    g = torch.Generator().manual_seed(2000 + seed)
    x = _push(torch.randn(M, K, generator=g), 0.25)
    dz = _push(torch.randn(M, N, generator=g) * 0.1, 0.05)
    gW0 = torch.randn(K, N, generator=g)
    gb0 = torch.randn(N, generator=g)
    dz[heavy_rows(route, M, K, N, shiftT, cus)] *= heavy_factor(M)
    return x, dz, gW0, gb0


def head_inputs(M, K, split, seed=0):
    """x (M, K), W (K, 1), b (1), accumulators gW0 (K, 1), gb0 (1) and the two row weights.  The forward's
    reduction edges are heavy as in ``dense_inputs``; the rows on both sides of the split and rows 0 and
    M - 1 of x are scaled (the loss gradient itself is a constant per segment)."""
    x, W, b = dense_inputs(M, K, 1, seed + 500)
    g = torch.Generator().manual_seed(3000 + seed)
    gW0 = torch.randn(K, 1, generator=g)
    gb0 = torch.randn(1, generator=g)
    rows = sorted({0, M - 1, min(max(split - 1, 0), M - 1), min(split, M - 1)})
    x[rows] *= 8.0 + M / 16.0
    wa, wb = 0.0625, -16.0  # exact in fp32; far apart so that a row on the wrong side of the split shows
    return x, W, b, gW0, gb0, wa, wb


# ------------------------------------------------------------------------------ references and budgets
def apply_act(z, act):
    from hfrep.ops import reference as R

    return R.apply_act(z, act)


def fwd_reference(x, W, b, act, dt):
    """fp64 reference and per-element budget of y = act(x W + b); x as the kernel receives it (dtype dt),
    W (K, N) and b fp32 (b may be None).  Runs on the tensors' device."""
    xd, Wd = x.double(), W.double()
    K = xd.shape[1]
    z, S = xd @ Wd, xd.abs() @ Wd.abs()
    if b is not None:
        z, S = z + b.double(), S + b.double().abs()
    ref = apply_act(z, act)
    budget = (K + 2) * U32 * S + (ACT_FLOOR if act else 0.0)
    if dt == BF:
        budget = budget + U16 * S + U16 * ref.abs()
    return ref, budget


def shifted(x, shiftT):
    """The weight gradient's row operand xe."""
    if shiftT <= 0:
        return x
    xe = torch.zeros_like(x)
    xe[1:] = x[:-1]
    xe[torch.arange(0, x.shape[0], shiftT, device=x.device)] = 0
    return xe


def wgrad_reference(x, dz, gW0, gb0, shiftT):
    """fp64 references and per-element budgets of gW and gb (x, dz as the kernel receives them)."""
    M = x.shape[0]
    xe, d = shifted(x.double(), shiftT), dz.double()
    rW = gW0.double() + xe.t() @ d
    rb = gb0.double() + d.sum(0)
    c = (2 * M + 8) * U32
    return rW, c * (xe.abs().t() @ d.abs()) + 2 * U32 * rW.abs(), rb, c * d.abs().sum(0) + 2 * U32 * rb.abs()


def head_d(M, split, wa, wb, device=None):
    d = torch.full((M, 1), wb, dtype=torch.float64, device=device)
    d[:split] = wa
    return d


def worst(got, ref, budget):
    """(ratio, index) of the element with the largest error / budget."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / budget.clamp_min(1e-300))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))  # a NaN output (poison: never written) is a miss
    ratio = torch.where(torch.isnan(got.double()), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    return ratio.flatten()[i].item(), tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))


# ------------------------------------------------------------------------------------------ tables
def _nf(K, N):
    return f"narrowf<{(N + 15) // 16},{K // 16},{K % 16 // 4}>"


def _wf(K):
    return f"widef<{(K + 15) // 16}>"


def _cyc(seq, i):
    return seq[i % len(seq)]


def forward_table(cus=MI355X_CUS):
    """Rows (op, dt, M, K, N, act, route) of ``linear`` and ``linear_dgrad``.  ``cus``: the device's compute
    units, for the rows just past one grid pass of each persistent kernel."""
    rows = []

    def add(op, dt, M, K, N, act, route):
        if M == 1 and act in (1, 2):
            act = 3  # one row of a saturated sigmoid / tanh (the heavy edges) shows no mutation at 3x
        rows.append((op, dt, M, K, N, act if op == "linear" else 0, route))

    # (M, the activation and the dtype cycle at different rates, so that none fixes another within a block)
    # narrowf (fp32, 16-row chunks): every K x N in {5, 16, 17, 112}, both stride orders; every NT at K = 36
    i = 0
    for K in (32, 36, 64, 100, 128):
        for N in (5, 16, 17, 112):
            add("linear", F32, _cyc((1, 16, 17, 33), i), K, N, _cyc((0, 3, 1, 2), i + i // 4), _nf(K, N))
            add("linear_dgrad", F32, _cyc((17, 1, 33, 16), i), K, N, 0, _nf(K, N))
            i += 1
    for N in (5, 17, 33, 49, 65, 81, 97):
        add("linear", F32, 35, 36, N, 3, _nf(36, N))
    add("linear", F32, 64 * 4 * cus + 21, 32, 5, 0, _nf(32, 5))
    # widef (fp32, 16-row chunks, K % 4 == 0, K <= 320): NQ in {1, 2, 9, 19, 20}, ncb 1 -> 2 -> 3, k tails
    for j, (K, N) in enumerate([(4, 5), (16, 17), (20, 112), (20, 113), (20, 225), (132, 7), (144, 33), (128, 113),
                                (300, 100), (320, 5)]):
        add("linear", F32, _cyc((1, 16, 17, 33), j), K, N, _cyc((3, 0, 2, 1), j + j // 4), _wf(K))
        add("linear_dgrad", F32, _cyc((17, 33, 1, 16), j), K, N, 0, _wf(K))
    add("linear", F32, 64 * cus + 21, 4, 5, 0, _wf(4))
    # bf16 narrow (32-row tiles, forward only)
    i = 0
    for K in (2, 14, 16, 18, 126, 128):
        for N in (5, 31, 32, 33, 64):
            add("linear", BF, _cyc((1, 32, 33, 65), i), K, N, _cyc((0, 3), i // 4), "narrow")
            i += 1
    add("linear", BF, 32 * 4 * 8 * cus + 21, 2, 5, 0, "narrow")
    # bf16 linear2 (128-row tiles), both w_trans values
    i = 0
    for N in (65, 128, 129):
        for K in (1, 31, 32, 33):
            add("linear", BF, _cyc((1, 128, 129), i), K, N, _cyc((3, 0), i), "linear2")
            # (a 1-column dz with N % 8 == 0 outputs is the skinny input gradient's)
            add("linear_dgrad", BF, _cyc((129, 1, 128), i), K, N, 0, "skinny" if (K, N) == (1, 128) else "linear2")
            i += 1
    # generic linear_kernel (128-row tiles): K odd, K < 32, K = 321; the skinny decline (N <= 4, K % 8 != 0);
    # N = 63, 64, 65
    for j, (dt, K, N) in enumerate([(F32, 3, 63), (F32, 31, 64), (F32, 321, 65), (F32, 12, 3), (F32, 7, 1), (F32, 33, 5),
                                    (BF, 3, 63), (BF, 31, 64), (BF, 321, 5), (BF, 12, 3), (BF, 7, 1), (BF, 129, 33)]):
        add("linear", dt, _cyc((1, 128, 129), j), K, N, _cyc((0, 3), j) if dt == BF else _cyc((0, 1, 2, 3), j), "linear")
    for j, (dt, K, N) in enumerate([(F32, 3, 63), (F32, 321, 65), (F32, 31, 3), (BF, 3, 63), (BF, 321, 64), (BF, 32, 33),
                                    (BF, 12, 3)]):
        add("linear_dgrad", dt, _cyc((129, 1, 128), j), K, N, 0, "linear")
    # skinny (N <= 4, K % 8 == 0, 4 waves x SK_ROWS = 16 rows per block): K in {8, 512, 520, the largest}
    i = 0
    for n in (1, 2, 3, 4):
        kmax = min(8192, 16384 // n // 8 * 8)
        for kb in (8, 512, 520, kmax):
            dt = _cyc((F32, BF), i + n)
            add("linear", dt, _cyc((1, 16, 17), i), kb, n, _cyc((0, 3), i // 2), "skinny")
            add("linear_dgrad", dt, _cyc((17, 1, 16), i), n, kb, 0, "skinny")
            i += 1
    add("linear", BF, 16 * 8 * cus + 21, 8, 1, 0, "skinny")
    # the skinny input gradient is a grid-stride kernel of its own: 16 cus blocks of 256 threads, one 8-wide
    # output chunk per thread, so M N / 8 just past 256 * 16 cus re-enters its loop
    add("linear_dgrad", BF, 512 * cus + 21, 1, 64, 0, "skinny")
    return rows


def wgrad_table():
    """Rows (dt, M, K, N, shiftT, route) of ``linear_wgrad_`` (each runs with gb and with gb = None)."""
    rows = []
    # fp32 three-term split: all 16 (NI, NJ) = (ceil((K + 1) / 32), ceil(N / 32)); N = 1 only at odd K
    # (N <= 4 with K % 8 == 0 is the skinny kernel's)
    i = 0
    for K in (31, 32, 63, 64, 95, 96, 127):
        for N in (1, 32, 33, 64, 65, 96, 97, 128):
            if N == 1 and K % 8 == 0:
                continue
            rows.append((F32, _cyc((1, 31, 32, 33, 1025), i), K, N, 0, f"wgrad_f32s<{(K + 32) // 32},{(N + 31) // 32}>"))
            i += 1
    # bf16 narrow (K % 4 == 0, K + 1 <= 128, N <= 32; N % 4 != 0 tail)
    for j, (K, N) in enumerate([(4, 1), (4, 7), (4, 32), (124, 1), (124, 7), (124, 32)]):
        rows.append((BF, _cyc((2049, 33), j), K, N, 0, "wgrad_narrow"))
    # generic wgrad_kernel: bf16 at N = 33 and at K % 4 != 0, fp32 past the split kernel's 128
    rows += [(BF, 33, 100, 33, 0, "wgrad"), (BF, 65, 6, 7, 0, "wgrad"), (BF, 2049, 130, 5, 0, "wgrad"),
             (F32, 33, 128, 129, 0, "wgrad"), (F32, 2049, 128, 5, 0, "wgrad")]
    # the time shift (generic kernel in both dtypes): two splits at M >= 2049 (boundary 1056 is a window
    # start of shiftT = 3 and 24, 1088 at M = 2113 is inside a window of both); shiftT = M is one window
    for dt in (BF, F32):
        for M, sh in ((2049, 1), (2049, 3), (2049, 24), (2113, 3), (2113, 24), (33, 33), (31, 5)):
            rows.append((dt, M, 36 if dt == BF else 100, 20, sh, "wgrad"))
    # skinny (shiftT = 0 only; with a shift the same shape is the generic kernel's)
    i = 0
    for n in (1, 2, 3, 4):
        kmax = min(8192, 16384 // n // 8 * 8)
        for kb in (8, 512, 520, kmax):
            rows.append((_cyc((BF, F32), i + n), _cyc((1, 17, 65, 2049), i) if kb <= 520 else 65, kb, n, 0, "skinny"))
            i += 1
    rows.append((BF, 48, 8, 1, 24, "wgrad"))
    return rows


def head_table(cus=MI355X_CUS):
    """Rows (dt, M, K, split, has_b, has_gb, route) of ``linear_head_cs``."""
    rows = []
    # the full cross of dtype, K, M and split.  The four (b, gb) given / None combinations rotate with the
    # split, the dtype and K, so that every (dtype, NC, M) sees b given and None and gb given and None
    # (M = 1 has two splits and each NC two K: together the four combinations)
    for ki, (K, nc) in enumerate(((8, 5), (2560, 5), (2568, 8), (4096, 8))):
        for M in (1, 15, 16, 17):
            for si, split in enumerate(sorted({0, 1, M // 2, M})):
                for di, dt in enumerate((F32, BF)):
                    c = (si + di + 2 * ki) % 4
                    rows.append((dt, M, K, split, c % 2 == 0, c < 2, f"head_cs<{nc}>"))
    m = 16 * 2 * cus + 21
    rows.append((BF, m, 8, m - 1, True, True, "head_cs<5>"))
    rows.append((F32, m, 8, m - 1, False, True, "head_cs<5>"))
    return rows


def row_id(row):
    return "-".join(str(v).replace("torch.", "") for v in row)
