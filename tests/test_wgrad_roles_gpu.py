"""The role-split fp32 LSTM weight gradient (csrc/lstm_f32.hip lstmf_wgrad_roles_kernel: MFMA waves 0-3,
staging waves 4-7; the default at K in {32, 100}) against the kernels whose arithmetic it keeps: the
column-pair split (``impl=2``) at K = 32 and the column-quad split (``impl=3``) at K = 100.  Same work
partition, same six products per tile in the same order into a zeroed accumulator that is added to the
running sum once per chunk: the outputs must be BITWISE equal, and bitwise equal run to run.

Shapes (B, T, K, tangent):
  (1, 5, 100, F)                        one partial chunk; rows 5..31 staged as zeros
  (3, 24, 32, T)                        72 rows: two full chunks plus a partial one, both LDS buffers; the
                                        tangent segment rewrites the bias column
  (41, 5, 100, T), (41, 5, 32, F)       T does not divide 32: the ``t == 0`` mask of the shifted H rows moves
                                        inside chunks and across row-range starts
  (700, 24, 100, T), (700, 24, 32, F)   9 / 5 chunks per row range on 256 CUs: odd chunk count, ragged last range
  (1000, 24, 100, F), (1000, 24, 32, T) 12 / 6 chunks per row range: even chunk count
  (120000, 25, 100, F)                  more than 4 GiB of dZ: the per-workgroup buffer descriptors
"""
import pytest
import torch

from hfrep.ops import functional as Fn

pytestmark = pytest.mark.gpu

H, N = 100, 400
CASES = [(1, 5, 100, False), (3, 24, 32, True), (41, 5, 100, True), (41, 5, 32, False), (700, 24, 100, True),
         (700, 24, 32, False), (1000, 24, 100, False), (1000, 24, 32, True), (120000, 25, 100, False)]


@pytest.mark.parametrize("B,T,K,tangent", CASES)
def test_wgrad_roles_bitwise(cuda, B, T, K, tangent):
    """Default path twice and the reference impl once, from the same random non-zero gW / gU / gb (the op
    accumulates): torch.equal on all three outputs."""
    g = torch.Generator(device=cuda).manual_seed(4100 + 7 * B + T + K)
    rn = lambda *s: torch.randn(*s, device=cuda, generator=g)  # noqa: E731
    x, hs, dz = rn(B, T, K), rn(B, T, H), rn(B, T, N)
    xd, hds, dzd = (rn(B, T, K), rn(B, T, H), rn(B, T, N)) if tangent else (None, None, None)
    g0 = (rn(K, N), rn(H, N), rn(N))
    assert all(bool((t != 0).any()) for t in g0)

    def run(impl):
        out = tuple(t.clone() for t in g0)
        Fn.lstm_wgrad_(x, hs, dz, *out, xd, hds, dzd, impl=impl)
        return out

    a, b, ref, r4 = run(0), run(0), run(2 if K == 32 else 3), run(4)
    for name, ta, tb, tr, t4, t0 in zip(("gW", "gU", "gb"), a, b, ref, r4, g0):
        assert not torch.equal(ta, t0), f"{name}: nothing accumulated"
        assert torch.equal(ta, tb), f"{name}: default path not bitwise run-to-run"
        assert torch.equal(t4, tr), f"{name}: the role kernel (impl 4) differs from impl {2 if K == 32 else 3}"
        ndiff, dmax = int((ta != tr).sum()), float((ta - tr).abs().max())
        print(f"{name}: {ndiff} of {ta.numel()} elements differ from the reference impl (max |diff| {dmax:.3e})")
        assert torch.equal(ta, tr), f"{name}: default path differs from impl {2 if K == 32 else 3}"
