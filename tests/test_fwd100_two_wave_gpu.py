"""The exact fp32 K = 100 LSTM forward on two waves per SIMD (lstmf_fwd2_kernel, set_lstmf_fwd100_impl 2)
against the four-wave exact forward (lstmf_fwd_kernel, value 1): the eight-wave kernel regroups the same 25
gate-interleaved tiles over more waves and runs the same arithmetic per tile, so every output is bitwise
equal -- hs with and without a tape, the tangent forward's hds, and every tape value a consumer reads (the
slots of the four-wave layout's three padding tiles are never written; they are masked here, and the tapes
are also compared through their consumers, the BPTT and the tangent reverse).  Three launches of value 2 are
bitwise equal (this family's races have shown up as run-to-run drift)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, K = 100, 100
FNT, SLOT = 7, 320  # tiles per wave of the 4-wave layout; floats per tape slot (64 lanes x (4 gates + 1 cell))


def _ops():
    from hfrep.ops import _native

    return _native.native()


def _tape_view(t, B, T):
    """(row block, step, wave, row half, tile, slot) view of a flat fp32 tape, padding tiles dropped."""
    v = t.view((B + 31) // 32, T, 4, 2, FNT, SLOT)
    return v[:, :, :3], v[:, :, 3, :, :4]


def _tapes_equal(a, b, B, T):
    return all(torch.equal(p, q) for p, q in zip(_tape_view(a, B, T), _tape_view(b, B, T)))


def test_switch_returns_previous_and_defaults_to_eight_waves(cuda):
    ops = _ops()
    first = ops.set_lstmf_fwd100_impl(1)
    try:
        assert first == 2  # the library default
        assert ops.set_lstmf_fwd100_impl(2) == 1
        assert ops.set_lstmf_fwd100_impl(1) == 2
    finally:
        ops.set_lstmf_fwd100_impl(first)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("B,T", [(1, 1), (33, 2), (70, 24), (8192 + 45, 3)])
def test_two_wave_exact_forward_bitwise(cuda, act, B, T):
    from hfrep.ops import functional as Fn

    g = torch.Generator().manual_seed(84)
    x = torch.randn(B, T, K, generator=g) * 0.5
    xd = torch.randn(B, T, K, generator=g) * 0.3
    W = torch.randn(K, 4 * H, generator=g) * (1.0 / K ** 0.5)
    b = torch.randn(4 * H, generator=g) * 0.1
    U = torch.randn(H, 4 * H, generator=g) * (1.0 / H ** 0.5)
    dH, dHd = torch.randn(B, T, H, generator=g), torch.randn(B, T, H, generator=g)
    xg, xdg, Wg, bg, Ug, dHg, dHdg = (t_.to(cuda) for t_ in (x, xd, W, b, U, dH, dHd))
    ops = _ops()

    def run(impl, ptape):
        ops.set_lstmf_fwd100_impl(impl)
        hs, tape = Fn.lstm_layer_fwd(xg, Wg, bg, Ug, act, True)
        hs0, _ = Fn.lstm_layer_fwd(xg, Wg, bg, Ug, act, False)
        hds, ttape = Fn.lstm_layer_tfwd(xdg, Wg, ptape if ptape is not None else tape, Ug, act)
        return hs, hs0, hds, tape, ttape

    prev = ops.set_lstmf_fwd100_impl(1)
    try:
        ref = run(1, None)
        new = [run(2, ref[3]) for _ in range(3)]  # (the tangent forwards all read the four-wave primal tape)
    finally:
        ops.set_lstmf_fwd100_impl(prev)
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[2]).all()
    dz_ref = Fn.lstm_layer_bwd(dHg, ref[3], Ug, act)
    tb_ref = Fn.lstm_layer_tbwd(dHg, dHdg, ref[3], ref[4], Ug, act)
    for i, out in enumerate(new):
        assert torch.equal(out[0], ref[0]), f"hs (tape) launch {i}"
        assert torch.equal(out[1], ref[1]), f"hs (no tape) launch {i}"
        assert torch.equal(out[2], ref[2]), f"hds launch {i}"
        assert _tapes_equal(out[3].t, ref[3].t, B, T), f"primal tape launch {i}"
        assert _tapes_equal(out[4].t, ref[4].t, B, T), f"tangent tape launch {i}"
    # the tapes through their consumers
    assert torch.equal(Fn.lstm_layer_bwd(dHg, new[0][3], Ug, act), dz_ref)
    tb_new = Fn.lstm_layer_tbwd(dHg, dHdg, new[0][3], new[0][4], Ug, act)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(tb_new, tb_ref))
