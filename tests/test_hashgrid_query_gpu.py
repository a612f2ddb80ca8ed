"""HashGrid.query on the device against brute force (hashgrid_query_cases):
count, offset, query_idx and sample_idx bit for bit on every case group, the
cell cap, and the refusals that come before a launch."""
import numpy as np
import pytest

import hashgrid_query_cases as hq

pytestmark = pytest.mark.gpu


def _run(case):
    import torch

    from mtx.primitives import HashGrid

    dev = torch.device("cuda", 0)
    p = torch.as_tensor(case["p"], device=dev)
    q = torch.as_tensor(case["q"], device=dev)
    r = case["r"]
    r = float(r) if np.ndim(r) == 0 else torch.as_tensor(r, device=dev)
    grid = HashGrid(p, case["res"], case["n_cells"])
    return grid, [t.cpu().numpy().astype(np.int64) for t in grid.query(q, r)]


def _check(case):
    grid, got = _run(case)
    ref = hq.brute_force(case["p"], case["q"], case["r"], case["res"])
    for name, g, e in zip(("count", "offset", "query_idx", "sample_idx"), got, ref):
        assert np.array_equal(g, e), (case["name"], name)
    return grid


@pytest.mark.parametrize("n", hq.NS)
def test_query_random_points(n):
    """Group (a): n x every m, resolution, n_cells in {1, 2, n, 4n + 1}, scalar and per-query radius."""
    for case in hq.cases_random(n):
        _check(case)


@pytest.mark.parametrize("group", ["lattice", "outside", "degenerate"])
def test_query_groups(group):
    """(b) exact lattice distances at d2 = r^2, duplicates, boundary queries
    and the one-float-beyond samples; (c) queries outside the bounds, r = 0,
    negative / NaN r, NaN / inf q; (d) one sample and equal coordinates."""
    for case in getattr(hq, "cases_" + group)():
        grid = _check(case)
        bb = hq.bounds(case["p"])
        assert (np.float32(grid.bbmin), np.float32(grid.bbmax)) == bb


def test_query_cell_cap():
    """(e) A box of 17 cells per axis is refused with the count of such
    queries and the advice; the context stays usable; 16 per axis is accepted."""
    from mtx._lib import MtxError

    ok, over = hq.cases_cap()
    with pytest.raises(MtxError, match=r"1 queries whose cell box holds more than 4096 cells.*resolution"):
        _run(over)
    _check(ok)
    two = dict(over, q=np.concatenate([over["q"], ok["q"], over["q"]], 1),
               r=np.array([over["r"], ok["r"], over["r"]], np.float32))
    with pytest.raises(MtxError, match=r"2 queries"):
        _run(two)
    _check(ok)


def test_query_empty_and_host_grid():
    import torch

    from mtx._lib import MtxError
    from mtx.primitives import HashGrid

    case = hq.cases_outside()[0]
    grid = HashGrid(torch.as_tensor(case["p"], device="cuda:0"), case["res"], case["n_cells"])
    count, offset, qi, si = grid.query(torch.empty((3, 0), device="cuda:0"), 0.1)
    assert [tuple(t.shape) for t in (count, offset, qi, si)] == [(0,)] * 4
    assert all(t.dtype == torch.int32 for t in (count, offset, qi, si))
    host = HashGrid(case["p"], case["res"], case["n_cells"])
    assert (np.float32(host.bbmin), np.float32(host.bbmax)) == hq.bounds(case["p"])
    with pytest.raises(MtxError, match="query needs torch CUDA tensors"):
        host.query(case["q"], 0.1)


def test_query_refusals_before_a_launch():
    """(f) A host tensor, the wrong dtype, a non-contiguous q and a radius
    tensor of the wrong length each raise naming the argument."""
    import torch

    from mtx._lib import MtxError
    from mtx.primitives import HashGrid

    case = hq.cases_outside()[0]
    dev = torch.device("cuda", 0)
    grid = HashGrid(torch.as_tensor(case["p"], device=dev), case["res"], case["n_cells"])
    q = torch.as_tensor(case["q"], device=dev)
    m = q.shape[1]
    with pytest.raises(MtxError, match="q: expected a torch CUDA tensor"):
        grid.query(q.cpu(), 0.1)
    with pytest.raises(MtxError, match="q: expected a torch CUDA tensor"):
        grid.query(case["q"], 0.1)
    with pytest.raises(MtxError, match="q: dtype"):
        grid.query(q.double(), 0.1)
    with pytest.raises(MtxError, match="q: not contiguous"):
        grid.query(q.t().contiguous().t(), 0.1)
    with pytest.raises(MtxError, match="q: shape"):
        grid.query(q[:2].contiguous(), 0.1)
    with pytest.raises(MtxError, match="radius: shape"):
        grid.query(q, torch.full((m + 1,), 0.1, device=dev))
    with pytest.raises(MtxError, match="radius: dtype"):
        grid.query(q, torch.full((m,), 0.1, device=dev, dtype=torch.float64))
    with pytest.raises(MtxError, match="radius: on"):
        grid.query(q, torch.full((m,), 0.1))
    count, *_ = grid.query(q, 0.1)  # and the grid still answers
    assert np.array_equal(count.cpu().numpy(), hq.brute_force(case["p"], case["q"], 0.1, case["res"])[0])
