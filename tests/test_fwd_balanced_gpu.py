"""The eight-wave fp32 LSTM forwards (lstmf_fwd2_kernel at K = 100, set_lstmf_fwd100_impl 2; lstmf_fwds2_kernel at
K = 32, set_lstmf_fwd_impl 3) against their four-wave references (values 1 and 2), at shapes chosen for a tile that
is split between two waves by row half.  At K = 100 the tiles are balanced across the SIMDs that way: wave v owns
tiles 3 v .. 3 v + 2, and tile 24 (units 96..99) is held by waves 0 and 1, wave 0 running it for rows 0-15 of a
32-row block and wave 1 for rows 16-31.  (At K = 32 the same ownership measured no clear gain and the kernel kept
its ownership by whole columns, profiles/fwd_balanced/README.md; the cases run there too, so a later re-balancing
meets them.)  The arithmetic per tile is the reference's, so hs with and without a tape, the tangent forward's hds
and both tapes (padding-tile slots masked, and through the BPTT and the tangent reverse) are bitwise equal, and
three launches agree.  The shapes aim at the split tile: a
block whose second row half is empty, one with a single row there, a full block, a partial third block at the
workload's T, and more row blocks than CUs (a workgroup re-enters with tile 24's cell state reset).  Units 96..99
are also asserted per row half, so a failure names the owning wave."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 100
FNT, SLOT = 7, 320  # tiles per wave of the 4-wave layout; floats per tape slot (64 lanes x (4 gates + 1 cell))

# K: (switch, reference value, eight-wave value)
KERNELS = {100: ("set_lstmf_fwd100_impl", 1, 2), 32: ("set_lstmf_fwd_impl", 2, 3)}
SHAPES = [(16, 1), (17, 2), (32, 3), (69, 24)]
CASES = [(K, act, B, T) for K in KERNELS for act in (0, 1, 2) for B, T in SHAPES]
CASES += [(K, 2, 8192 + 45, 3) for K in KERNELS]


def _ops():
    from hfrep.ops import _native

    return _native.native()


def _tape_view(t, B, T):
    """(row block, step, wave, row half, tile, slot) view of a flat fp32 tape, padding tiles dropped."""
    v = t.view((B + 31) // 32, T, 4, 2, FNT, SLOT)
    return v[:, :, :3], v[:, :, 3, :, :4]


def _tapes_equal(a, b, B, T):
    return all(torch.equal(p, q) for p, q in zip(_tape_view(a, B, T), _tape_view(b, B, T)))


def _tile24_halves(t):
    """Units 96..99 of a (B, T, H) tensor, split into rows 0-15 and rows 16-31 of every 32-row block."""
    rows = torch.arange(t.shape[0], device=t.device) % 32
    u = t[:, :, 96:]
    return u[rows < 16], u[rows >= 16]


@pytest.mark.parametrize("K,act,B,T", CASES)
def test_balanced_forward_bitwise(cuda, K, act, B, T):
    from hfrep.ops import functional as Fn

    g = torch.Generator().manual_seed(85)
    x = torch.randn(B, T, K, generator=g) * 0.5
    xd = torch.randn(B, T, K, generator=g) * 0.3
    W = torch.randn(K, 4 * H, generator=g) * (1.0 / K ** 0.5)
    b = torch.randn(4 * H, generator=g) * 0.1
    U = torch.randn(H, 4 * H, generator=g) * (1.0 / H ** 0.5)
    dH, dHd = torch.randn(B, T, H, generator=g), torch.randn(B, T, H, generator=g)
    xg, xdg, Wg, bg, Ug, dHg, dHdg = (t_.to(cuda) for t_ in (x, xd, W, b, U, dH, dHd))
    ops = _ops()
    switch, v_ref, v_new = KERNELS[K]
    set_impl = getattr(ops, switch)

    def run(impl, ptape):
        set_impl(impl)
        hs, tape = Fn.lstm_layer_fwd(xg, Wg, bg, Ug, act, True)
        hs0, _ = Fn.lstm_layer_fwd(xg, Wg, bg, Ug, act, False)
        hds, ttape = Fn.lstm_layer_tfwd(xdg, Wg, ptape if ptape is not None else tape, Ug, act)
        return hs, hs0, hds, tape, ttape

    prev = set_impl(v_ref)
    try:
        ref = run(v_ref, None)
        new = [run(v_new, ref[3]) for _ in range(3)]  # (the tangent forwards all read the reference primal tape)
    finally:
        set_impl(prev)
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[2]).all()
    dz_ref = Fn.lstm_layer_bwd(dHg, ref[3], Ug, act)
    tb_ref = Fn.lstm_layer_tbwd(dHg, dHdg, ref[3], ref[4], Ug, act)
    for i, out in enumerate(new):
        # tile 24 on its own first: at K = 100 row half 0 is wave 0's, row half 1 is wave 1's
        for name, j in (("hs (tape)", 0), ("hs (no tape)", 1), ("hds", 2)):
            for half, (a_, r_) in enumerate(zip(_tile24_halves(out[j]), _tile24_halves(ref[j]))):
                assert torch.equal(a_, r_), (
                    f"{name} launch {i}: tile 24 (units 96..99), row half {half} "
                    f"(rows {16 * half}-{16 * half + 15} of a block; at K = 100 wave {half} runs it)")
        assert torch.equal(out[0], ref[0]), f"hs (tape) launch {i}"
        assert torch.equal(out[1], ref[1]), f"hs (no tape) launch {i}"
        assert torch.equal(out[2], ref[2]), f"hds launch {i}"
        assert _tapes_equal(out[3].t, ref[3].t, B, T), f"primal tape launch {i}"
        assert _tapes_equal(out[4].t, ref[4].t, B, T), f"tangent tape launch {i}"
    # the tapes through their consumers
    assert torch.equal(Fn.lstm_layer_bwd(dHg, new[0][3], Ug, act), dz_ref)
    tb_new = Fn.lstm_layer_tbwd(dHg, dHdg, new[0][3], new[0][4], Ug, act)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(tb_new, tb_ref))
