"""The role-split fp32 input gradient dX = dZ W^T (csrc/lstmf_grad.hip lstmf_dgrad_roles_kernel: MFMA waves
0-6 with one 16-column output tile each, staging wave 7; ``impl=4`` of ``lstmf_dgrad`` and the default for
fp32 operands at KO > 64) against the kernel whose arithmetic it keeps, lstmf_dgrad_s4_kernel (``impl=3``):
per output element k-steps 0..12 in order, the six split products of each chained onto an accumulator that
starts at zero.  The outputs must be BITWISE equal, and bitwise equal run to run.

Shapes (M, KO), chosen at 256 CUs:
  (1, 100)         one partial chunk; rows 1..15 staged as zeros; no row past M written
  (17, 100)        second chunk holds one row
  (1000, 112)      63 chunks (< CUs, one per workgroup); all seven tiles full; last chunk 8 rows
  (1000, 65)       five tiles, the fifth with one live column; the two MFMA waves with no live column store nothing
  (8200, 100)      513 chunks: workgroup 0 gets three (odd count, buffer reuse), the others two; last chunk 8 rows
  (20000, 97)      4-5 chunks per workgroup, ragged; partial last tile
  (2700000, 100)   dZ is 4.32 GB: per-chunk descriptors past 4 GiB
"""
import pytest
import torch

from hfrep.ops import _native
from hfrep.ops import functional as Fn

pytestmark = pytest.mark.gpu

N = 400
CASES = [(1, 100), (17, 100), (1000, 112), (1000, 65), (8200, 100), (20000, 97), (2700000, 100)]


def _operands(cuda, M, KO):
    g = torch.Generator(device=cuda).manual_seed(5200 + 3 * KO + M % 1009)
    dz = torch.randn(M, N, device=cuda, generator=g)
    W = torch.randn(KO, N, device=cuda, generator=g) * 0.1
    return dz, W


@pytest.mark.parametrize("M,KO", CASES)
def test_dgrad_roles_bitwise(cuda, M, KO):
    """impl 4 twice, impl 3 once and the default path once: torch.equal among all four, and not all zero."""
    ops = _native.native()
    dz, W = _operands(cuda, M, KO)
    a, b = ops.lstmf_dgrad(dz, W, 4), ops.lstmf_dgrad(dz, W, 4)
    ref = ops.lstmf_dgrad(dz, W, 3)
    d = Fn.linear_dgrad(dz, W)
    assert a.shape == (M, KO) and d.shape == (M, KO)
    assert bool((a != 0).any()), "impl 4: all zero"
    ndiff = int((a != ref).sum())
    print(f"M={M} KO={KO}: {ndiff} of {a.numel()} elements differ from impl 3"
          f" (max |diff| {float((a - ref).abs().max()):.3e})")
    assert torch.equal(a, b), "the role kernel (impl 4) is not bitwise run-to-run"
    assert torch.equal(a, ref), "the role kernel (impl 4) differs from impl 3"
    assert torch.equal(d, ref), "the default path differs from impl 3"


@pytest.mark.parametrize("KO", [32, 64])
def test_dgrad_default_below_65_is_exact_kernel(cuda, KO):
    """KO <= 64 keeps the exact kernel as the default: Fn.linear_dgrad equals impl 1 bitwise."""
    ops = _native.native()
    dz, W = _operands(cuda, 5000, KO)
    d, e = Fn.linear_dgrad(dz, W), ops.lstmf_dgrad(dz, W, 1)
    assert bool((d != 0).any())
    assert torch.equal(d, e), "the default path at KO <= 64 differs from impl 1"
