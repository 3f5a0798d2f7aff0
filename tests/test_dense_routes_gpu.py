"""Every Dense kernel route vs an fp64 reference, element by element (run on an MI355X with -m gpu).

tests/test_kernels_gpu.py compares the largest error of a whole output with an allowance set by its
largest element, which a dropped edge row or reduction column stays under at most of its shapes.  Here
every row of the tables in tests/_dense_shapes.py (tile edges of every route of ``linear``, ``linear_dgrad``,
``linear_wgrad_`` and ``linear_head_cs``; tests/test_dense_shapes.py holds their inputs to showing an edge
error at >= 3x) first asserts the kernel it runs on (``dense_route``), then holds EVERY output element to its
own derived worst-case budget (see tests/_dense_shapes.py; a failure names the worst element and its ratio),
and runs twice for bitwise equality.  References are fp64 on the device, from the operands as the kernel
receives them.  The debug poison is on: an element no kernel wrote is NaN and fails.
"""
import pytest
import torch

import _dense_shapes as D
from test_kernels_gpu import _ops

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def poison(cuda):
    """Every op output and workspace starts as NaN for the duration of a test."""
    ops = _ops()
    prev = ops.set_debug_poison(True)
    try:
        yield
    finally:
        ops.set_debug_poison(prev)


# The ids come from the tables at an MI355X's 256 compute units; a test takes its row from the tables at
# the device's own count (only the rows just past one grid pass differ), so collecting touches no GPU.
FWD, WGRAD, HEAD = D.forward_table(), D.wgrad_table(), D.head_table()
_TABLES = {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _row(name, i):
    if not _TABLES:
        _TABLES.update(fwd=D.forward_table(_cus()), head=D.head_table(_cus()))
    return _TABLES[name][i]


def _ids(table):
    return [D.row_id(r) for r in table]


def _hold(what, got, ref, budget):
    ratio, idx = D.worst(got, ref, budget)
    print(f"  {what}: worst element {idx} at {ratio:.3f}x its budget")
    assert ratio <= 1.0, f"{what}: element {idx} is {ratio:.3f}x its budget (got {got[idx].item()!r}, ref {ref[idx].item()!r})"


def _route(op, dt, M, K, N, sh=0):
    return _ops().dense_route(op, dt == D.BF, M, K, N, sh)


def _run_fwd(op, xc, Wc, WTc, bc, act, out=None):
    """W is handed over (K, N) to ``linear`` and (N, K) to ``linear_dgrad``."""
    if op == "linear":
        return _ops().linear(xc, Wc, bc, act) if out is None else _ops().linear(xc, Wc, bc, act, out)
    return _ops().linear_dgrad(xc, WTc)


@pytest.mark.parametrize("i", range(len(FWD)), ids=_ids(FWD))
def test_forward_and_dgrad_routes(cuda, i):
    op, dt, M, K, N, act, route = _row("fwd", i)
    assert _route(op, dt, M, K, N) == route
    x, W, b = D.dense_inputs(M, K, N)
    xc, Wc, bc = x.to(cuda, dt), W.to(cuda), b.to(cuda)
    WTc = Wc.t().contiguous()
    biases = (bc, None) if op == "linear" else (None,)
    for bias in biases:
        y = _run_fwd(op, xc, Wc, WTc, bias, act)
        assert y.shape == (M, N) and y.dtype == dt
        ref, budget = D.fwd_reference(xc, Wc, bias, act, dt)
        _hold(f"{route} {'with' if bias is not None else 'without'} bias", y, ref, budget)
        assert torch.equal(y, _run_fwd(op, xc, Wc, WTc, bias, act)), "repeat run differs"


def _one_per_route(table, op):
    seen, rows = set(), []
    for r in table:
        key = (D.family(r[6]), r[1])
        if r[0] == op and key not in seen and 1 < r[2] <= 4096:
            seen.add(key)
            rows.append(r)
    return rows


@pytest.mark.parametrize("row", _one_per_route(FWD, "linear"), ids=D.row_id)
def test_linear_out_slice(cuda, row):
    """``out=``: a row slice in the middle of a larger buffer gets exactly the plain result, and the rows
    before and after it keep every bit."""
    op, dt, M, K, N, act, route = row
    assert _route(op, dt, M, K, N) == route
    x, W, b = D.dense_inputs(M, K, N)
    xc, Wc, bc = x.to(cuda, dt), W.to(cuda), b.to(cuda)
    plain = _ops().linear(xc, Wc, bc, act)
    g = torch.Generator().manual_seed(7)
    buf0 = torch.randn(M + 7, N, generator=g).to(cuda, dt)
    buf = buf0.clone()
    y = _ops().linear(xc, Wc, bc, act, buf[3:3 + M])
    assert y.data_ptr() == buf[3:3 + M].data_ptr()
    assert torch.equal(buf[3:3 + M], plain)
    assert torch.equal(buf[:3], buf0[:3]) and torch.equal(buf[3 + M:], buf0[3 + M:])


@pytest.mark.parametrize("row", WGRAD, ids=D.row_id)
def test_wgrad_routes(cuda, row):
    dt, M, K, N, sh, route = row
    assert _route("linear_wgrad_", dt, M, K, N, sh) == route
    x, dz, gW0, gb0 = D.wgrad_inputs(route, M, K, N, sh, cus=_cus())
    xc, dc, gW0c, gb0c = x.to(cuda, dt), dz.to(cuda, dt), gW0.to(cuda), gb0.to(cuda)
    rW, bW, rb, bb = D.wgrad_reference(xc, dc, gW0c, gb0c, sh)
    for with_gb in (True, False):
        runs = []
        for _ in range(2):
            gW, gb = gW0c.clone(), gb0c.clone()
            _ops().linear_wgrad_(xc, dc, gW, gb if with_gb else None, sh)
            runs.append((gW, gb))
        gW, gb = runs[0]
        _hold(f"{route} gW ({'with' if with_gb else 'without'} gb)", gW, rW, bW)
        if with_gb:
            _hold(f"{route} gb", gb, rb, bb)
        else:
            # gb = None changes Kr and has_bias in the kernels: the check that matters is gW's budget above.
            # The sentinel is not handed to the op, so this only catches a stray write past the workspace
            assert torch.equal(gb, gb0c), "gb = None: a gb-sized tensor next to the operands changed"
        assert torch.equal(gW, runs[1][0]) and torch.equal(gb, runs[1][1]), "repeat run differs"


@pytest.mark.parametrize("i", range(len(HEAD)), ids=_ids(HEAD))
def test_head_cs_routes(cuda, i):
    """``linear_head_cs``: y to the skinny forward's budget, gW and gb to the weight gradient's with
    d_r = wa (r < split) / wb."""
    dt, M, K, split, has_b, has_gb, route = _row("head", i)
    assert _route("linear_head_cs", dt, M, K, 1) == route
    x, W, b, gW0, gb0, wa, wb = D.head_inputs(M, K, split)
    xc, Wc, bc, gW0c, gb0c = x.to(cuda, dt), W.to(cuda), b.to(cuda) if has_b else None, gW0.to(cuda), gb0.to(cuda)
    ref, budget = D.fwd_reference(xc, Wc, bc, 0, dt)
    rW, bW, rb, bb = D.wgrad_reference(xc, D.head_d(M, split, wa, wb, cuda), gW0c, gb0c, 0)
    runs = []
    for _ in range(2):
        gW, gb = gW0c.clone(), gb0c.clone()
        y = _ops().linear_head_cs(xc, Wc, bc, split, wa, wb, gW, gb if has_gb else None)
        runs.append((y, gW, gb))
    y, gW, gb = runs[0]
    assert y.shape == (M, 1) and y.dtype == dt
    _hold(f"{route} y", y, ref, budget)
    _hold(f"{route} gW", gW, rW, bW)
    if has_gb:
        _hold(f"{route} gb", gb, rb, bb)
    else:
        assert torch.equal(gb, gb0c), "gb = None: the sentinel changed"
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c), "repeat run differs"
