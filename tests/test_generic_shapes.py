"""CPU-only: the inputs of tests/test_generic_shapes_gpu.py can see an edge-column error.

With the plain inputs of test_lstm2_fused_layer, zeroing the last input column moves h by only
0.7x .. 2.6x of what the bf16 tolerance allows, so a forward kernel that dropped that column would pass
at some widths.  ``lstm_inputs`` scales the first and the last row of W; this test holds the scaled
inputs to: zeroing column 0 or column K - 1 of x changes h by at least 3x the allowance of ``_close``
(a condition on the inputs, evaluated on the fp64 reference alone).
"""
import pytest
import torch

from _generic_shapes import ACTS, LSTM_SHAPES, lstm_inputs
from hfrep.ops import reference as R
from test_kernels_gpu import TOL


def _allowed(ref, dt):
    """The largest elementwise error ``_close(got, ref, dt)`` accepts."""
    s = max(ref.abs().max().item(), 1e-3)
    return TOL[dt]["atol"] * max(1.0, s) + TOL[dt]["rtol"] * s


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B,T,K", LSTM_SHAPES)
def test_lstm_inputs_expose_edge_columns(act, B, T, K):
    x, W, b, U, _ = lstm_inputs(B, T, K)
    xd, Wd = x.double(), W.double()
    rh = R.lstm_seq_fwd(xd @ Wd + b.double(), U.double(), act, False)[0]
    allowed = _allowed(rh, torch.bfloat16)
    for col in sorted({0, K - 1}):
        x0 = xd.clone()
        x0[:, :, col] = 0
        rh0 = R.lstm_seq_fwd(x0 @ Wd + b.double(), U.double(), act, False)[0]
        moved = (rh0 - rh).abs().max().item()
        print(f"act {act} (B, T, K) = ({B}, {T}, {K}) column {col}: {moved / allowed:.2f}x the allowance")
        assert moved >= 3 * allowed, (col, moved, allowed)
