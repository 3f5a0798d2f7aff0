"""Shapes and inputs shared by tests/test_generic_shapes_gpu.py (the kernels) and
tests/test_generic_shapes.py (the CPU-only check that these inputs can see an edge-column error).

The fused bf16 LSTM kernels (csrc/lstm2.hip) are specialised for the input widths K in
{32, 35, 36, 100}; every other K <= 128 takes the runtime-K path.  The shapes cover every k-step
count of that path (K <= 32, 64, 96, 128), odd / even K and K % 4 != 0, the 16-column owner boundaries of
the fused input gradient and both sides of its last one (112), T = 1 and T = 2 (degenerate prefetch /
double buffers), and B = 1, B = 32 exactly and a partial second row block.
"""
import torch

H = 100
LSTM_SHAPES = [(33, 5, 1), (70, 2, 20), (33, 5, 31), (40, 3, 33), (64, 5, 64), (33, 2, 97),
               (33, 5, 112), (33, 5, 113), (70, 3, 128),
               (1, 1, 20), (32, 1, 100), (33, 2, 35)]
ACTS = [0, 1, 2]


def lstm_inputs(B, T, K):
    """The inputs of test_lstm2_fused_layer (x bf16; W, b, U fp32) with rows 0 and K - 1 of W scaled by
    sqrt(K - 1): the first and the last input column then each carry as much of the pre-activation as all
    the other columns together, so a kernel that drops (or misplaces) an edge column of x is far outside
    the bf16 tolerance on h (tests/test_generic_shapes.py holds that to >= 3x).  The two edge columns of x
    are also pushed away from zero (|x| + 0.5, sign kept): the W scaling alone leaves the single row of
    (B, T, K) = (1, 1, 20), whose x[0, 0, 0] = 0.245 is half a standard deviation, at 1.3x (2.6x at three
    times the scaling), and the lone row of a partial second row block at the mercy of its own sample."""
    g = torch.Generator().manual_seed(20)
    x = torch.randn(B, T, K, generator=g) * 0.5
    for col in {0, K - 1}:
        x[:, :, col] += torch.where(x[:, :, col] >= 0, 0.5, -0.5)
    x = x.to(torch.bfloat16)
    W = torch.randn(K, 4 * H, generator=g) * (1.0 / K ** 0.5)
    b = torch.randn(4 * H, generator=g) * 0.1
    U = torch.randn(H, 4 * H, generator=g) * (1.0 / H ** 0.5)
    if K > 1:
        W[0] *= (K - 1) ** 0.5
        W[K - 1] *= (K - 1) ** 0.5
    return x, W, b, U, g
