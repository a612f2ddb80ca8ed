"""Reference and cases of the hash grid's fixed-radius query (numpy only).

The reference is brute force: the float32 distance test of include/mtx.h over
all n x m pairs, then each query's neighbours sorted by (cz, cy, cx, j) with
the cell coordinates c from the build's formula in float32. It shares no code
with the walk and knows nothing about hashing.

`walk` restates the walk itself (cell box, hash, filter by own cell) over a
grid built here in numpy, with the box either widened as the kernels widen it
or taken from the plain q -+ r. tests/test_hashgrid_query.py shows on the CPU
that the first equals brute force on every case and that the second does not
on group (b), so group (b) can tell a box that is too tight.

Shared by test_hashgrid_query.py (no GPU) and test_hashgrid_query_gpu.py.
"""
import numpy as np

F = np.float32
MAX_CELLS = 4096


# -------------------------------------------------------------- reference --
def coord(x, bbmin, bbmax, res):
    """c(x) = (uint32)((x - bbmin) / ext * (float)res) in float32: negative or
    NaN -> 0, clamped to res, all 0 without a positive extent."""
    x = np.asarray(x, F)
    ext = F(bbmax) - F(bbmin)
    if not ext > 0:
        return np.zeros(x.shape, np.int64)
    with np.errstate(all="ignore"):
        a = (x - F(bbmin)) / ext * F(res)
        a = np.where(a > 0, a, F(0))
        return np.minimum(a, F(res)).astype(np.int64)


def bounds(p):
    p = np.asarray(p, F)
    return F(p.min()), F(p.max())


def brute_force(p, q, r, res):
    """(count (m,), offset (m,), query_idx, sample_idx), all int64."""
    p, q = np.asarray(p, F).reshape(3, -1), np.asarray(q, F).reshape(3, -1)
    n, m = p.shape[1], q.shape[1]
    r = np.broadcast_to(np.asarray(r, F), (m,))
    bbmin, bbmax = bounds(p)
    with np.errstate(all="ignore"):
        dx = p[0][None, :] - q[0][:, None]
        dy = p[1][None, :] - q[1][:, None]
        dz = p[2][None, :] - q[2][:, None]
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = (d2 <= (r * r)[:, None]) & (r >= 0)[:, None]
    c = [coord(p[a], bbmin, bbmax, res) for a in range(3)]
    count = ok.sum(1).astype(np.int64)
    qi, si = [], []
    for i in range(m):
        js = np.flatnonzero(ok[i])
        js = js[np.lexsort((js, c[0][js], c[1][js], c[2][js]))]
        qi.append(np.full(len(js), i, np.int64))
        si.append(js)
    offset = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64) if m else np.zeros(0, np.int64)
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int64)  # noqa: E731
    return count, offset, cat(qi), cat(si)


# ------------------------------------------------- the walk, restated --
def hash_cell(cx, cy, cz, n_cells):
    m = np.uint64(0xffffffff)
    h = ((np.uint64(cx) * np.uint64(73856093)) & m) ^ ((np.uint64(cy) * np.uint64(19349663)) & m) \
        ^ ((np.uint64(cz) * np.uint64(83492791)) & m)
    return h % np.uint64(n_cells)


def build(p, res, n_cells):
    """The hash grid of hashgrid.py in numpy: (cell_size, cell_offset, sample_idx)."""
    p = np.asarray(p, F).reshape(3, -1)
    bbmin, bbmax = bounds(p)
    c = [coord(p[a], bbmin, bbmax, res).astype(np.uint64) for a in range(3)]
    cell = hash_cell(c[0], c[1], c[2], n_cells).astype(np.int64)
    size = np.bincount(cell, minlength=n_cells)
    return size, np.concatenate([[0], np.cumsum(size)[:-1]]), np.argsort(cell, kind="stable")


def cell_box(q, r, bbmin, bbmax, res, widen=True):
    """(lo (3,), hi (3,)) cell coordinates of one query's box, or None when
    nothing can be a neighbour. widen=False: the box of the plain q -+ r."""
    q, r = np.asarray(q, F), F(r)
    if not r >= 0 or np.isnan(q).any():
        return None
    with np.errstate(all="ignore"):
        if widen:
            wf = F(F(r * F(1 + 2.0 ** -20)) + F(2.0 ** -60))
            lo = np.nextafter(F(q - wf), F(-np.inf))
            hi = np.nextafter(F(q + wf), F(np.inf))
        else:
            lo, hi = F(q - r), F(q + r)
    lo = np.where(np.isnan(lo), F(-np.inf), lo)
    hi = np.where(np.isnan(hi), F(np.inf), hi)
    return coord(lo, bbmin, bbmax, res), coord(hi, bbmin, bbmax, res)


def walk(p, q, r, res, n_cells, widen=True):
    """The kernels' walk in numpy. Returns brute_force's tuple, or the number
    of queries over the cell cap as an int."""
    p, q = np.asarray(p, F).reshape(3, -1), np.asarray(q, F).reshape(3, -1)
    m = q.shape[1]
    r = np.broadcast_to(np.asarray(r, F), (m,))
    bbmin, bbmax = bounds(p)
    size, off, order = build(p, res, n_cells)
    c = np.stack([coord(p[a], bbmin, bbmax, res) for a in range(3)])
    count, qi, si, over = np.zeros(m, np.int64), [], [], 0
    for i in range(m):
        box = cell_box(q[:, i], r[i], bbmin, bbmax, res, widen)
        if box is None:
            continue
        lo, hi = box
        if int(np.prod((hi - lo + 1).astype(object))) > MAX_CELLS:
            over += 1
            continue
        r2 = r[i] * r[i]
        for cz in range(lo[2], hi[2] + 1):
            for cy in range(lo[1], hi[1] + 1):
                for cx in range(lo[0], hi[0] + 1):
                    h = int(hash_cell(cx, cy, cz, n_cells))
                    js = order[off[h]: off[h] + size[h]]
                    js = js[(c[0][js] == cx) & (c[1][js] == cy) & (c[2][js] == cz)]
                    if not len(js):
                        continue
                    with np.errstate(all="ignore"):
                        dx, dy, dz = p[0][js] - q[0, i], p[1][js] - q[1, i], p[2][js] - q[2, i]
                        d2 = (dx * dx + dy * dy) + dz * dz
                        js = js[d2 <= r2]
                    count[i] += len(js)
                    qi.append(np.full(len(js), i, np.int64))
                    si.append(js)
    if over:
        return over
    offset = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64) if m else np.zeros(0, np.int64)
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int64)  # noqa: E731
    return count, offset, cat(qi), cat(si)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ cases --
# A case: dict(name, p (3, n), q (3, m), r (float or (m,)), res, n_cells).
def _case(name, p, q, r, res, n_cells):
    p, q = np.ascontiguousarray(p, F).reshape(3, -1), np.ascontiguousarray(q, F).reshape(3, -1)
    r = F(r) if np.ndim(r) == 0 else np.ascontiguousarray(r, F)
    return dict(name=name, p=p, q=q, r=r, res=int(res), n_cells=int(n_cells))


NS, MS, RESOLUTIONS = (1, 63, 64, 65, 257, 4096), (1, 63, 64, 65, 257), (1, 2, 7, 16)


def cases_random(n):
    """Group (a) for one n: random points in [0, 1]^3, every m, resolution and
    n_cells in {1, 2, n, 4n + 1} (with 1 or 2 hash cells every walk meets
    colliding grid cells), a scalar and a per-query radius of about three
    quarters of a cell."""
    out = []
    for m in MS:
        rng = np.random.default_rng(1000 * n + m)
        p, q = rng.random((3, n), dtype=F), rng.random((3, m), dtype=F)
        for res in RESOLUTIONS:
            for n_cells in sorted({1, 2, n, 4 * n + 1}):
                r = F(0.75 / res)
                out.append(_case(f"a-n{n}-m{m}-res{res}-c{n_cells}-scalar", p, q, r, res, n_cells))
                out.append(_case(f"a-n{n}-m{m}-res{res}-c{n_cells}-per-query", p, q,
                                 r * (F(2) * rng.random(m, dtype=F)), res, n_cells))
    return out


def _lattice(lo, hi, step):
    g = np.arange(lo, hi + step / 2, step)
    return np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)


def cases_lattice():
    """Group (b). Multiples of 1/4 in [0, 3]^3 with r = 1.25: every distance
    is exact, and the 3-4-5 offsets (0.75, 1, 0) and (1.25, 0, 0) with their
    permutations and signs lie exactly at d2 = r^2, which is included. At
    resolution 12 (cells of 1/4) and 6 (cells of 1/2) the samples at q -+ 1.25
    sit on the lower edge of the box's outermost cells on every axis. Four
    samples are repeated at the end (coincident duplicates come back twice in
    index order). Queries: the corners bbmin and bbmax, cell boundaries and
    cell centres.

    The `ulp` cases hold what the exact ones cannot: a sample one float
    beyond q -+ r whose fl(p - q) rounds to r, so it passes the fp32 test, in
    the cell next to the one q -+ r falls into -- on the low side the cell
    below (p - bbmin is exact and just under a cell edge), on the high side
    the cell `res` that the point at bbmax has to itself -- on each axis."""
    out = []
    p = _lattice(0.0, 3.0, 0.25)
    p = np.concatenate([p, p[:, [0, 700, 1100, p.shape[1] - 1]]], 1)
    q = np.array([[0, 0, 0], [3, 3, 3], [1.5, 1.5, 1.5], [1.25, 1.5, 1.75], [0, 3, 1.5], [1.75, 1.25, 3],
                  [0.25, 2.75, 1.0], [1.5, 0, 3], [2.0, 2.0, 2.0]]).T
    for res in (12, 6):
        for n_cells in (2, p.shape[1]):
            out.append(_case(f"b-exact-res{res}-c{n_cells}", p, q, 1.25, res, n_cells))
    e = 2.0 ** -25
    for axis in range(3):
        base = _lattice(-0.5, 1.5, 0.25)
        extra, qq = np.array([0.5, 0.75, 0.25]), np.array([0.5, 0.75, 0.25])
        extra[axis], qq[axis] = -0.25 - e, 1.0
        out.append(_case(f"b-ulp-low-axis{axis}", np.concatenate([base, extra[:, None]], 1), qq[:, None], 1.25, 8, 64))
        base = _lattice(0.0, 0.25, 0.0625)
        extra, qq = np.array([0.125, 0.0625, 0.1875]), np.array([0.125, 0.0625, 0.1875])
        extra[axis], qq[axis] = 0.25 + e, -1.0
        out.append(_case(f"b-ulp-high-axis{axis}", np.concatenate([base, extra[:, None]], 1), qq[:, None], 1.25, 4, 64))
    return out


def cases_outside():
    """Group (c): queries just outside the bounds that still reach in, far
    outside (1e6 away: no neighbours), r = 0 at sample positions (coincident
    samples only), negative and NaN r, NaN and +-inf q."""
    rng = np.random.default_rng(7)
    p = rng.random((3, 257), dtype=F)
    p[:, 100] = p[:, 3]  # a coincident pair
    near = np.array([[-0.01, 0.5, 0.5], [1.01, 0.5, 0.5], [0.5, -0.02, 1.02], [1.03, 1.03, 1.03]]).T
    far = np.array([[1e6, 0.5, 0.5], [-1e6, -1e6, -1e6], [0.5, 0.5, 1e6]]).T
    odd = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.inf, np.inf, np.inf]]).T
    at = p[:, [3, 5, 100]]
    out = []
    for res, n_cells in ((7, 257), (16, 2)):
        out.append(_case(f"c-near-res{res}", p, near, 0.1, res, n_cells))
        out.append(_case(f"c-far-res{res}", p, far, 0.1, res, n_cells))
        out.append(_case(f"c-r0-res{res}", p, at, 0.0, res, n_cells))
        out.append(_case(f"c-r0-mixed-res{res}", p, np.concatenate([at, near], 1),
                         np.array([0, 0, 0, 0.1, 0.1, 0, 0.05]), res, n_cells))
        out.append(_case(f"c-negative-r-res{res}", p, at, -0.5, res, n_cells))
        out.append(_case(f"c-nan-r-res{res}", p, at, np.nan, res, n_cells))
        out.append(_case(f"c-odd-r-res{res}", p, np.concatenate([at, at], 1),
                         np.array([-1.0, np.nan, 0.1, 0.2, -0.0, np.nan]), res, n_cells))
        out.append(_case(f"c-odd-q-res{res}", p, odd, 0.1, res, n_cells))
    return out


def cases_degenerate():
    """Group (d): one sample, and samples whose coordinates are all equal:
    no extent, every cell coordinate is 0."""
    q = np.array([[0.3, 0.3, 0.3], [0.3, 0.3, 0.35], [5.0, -2.0, 0.3], [0.0, 0.0, 0.0]]).T
    out = []
    for res in (1, 16):
        out.append(_case(f"d-one-res{res}", np.array([[0.3], [0.3], [0.3]]), q, 0.1, res, 1))
        out.append(_case(f"d-one-offaxis-res{res}", np.array([[0.15], [0.45], [0.3]]), q, 0.25, min(res, 4), 3))
        out.append(_case(f"d-equal-res{res}", np.full((3, 5), 0.3), q, 0.1, res, 5))
    return out


def cases_cap():
    """Group (e): resolution 64 over [0, 1]^3. (accepted: a box of 16 cells
    per axis = 4096, refused: 17 per axis = 4913)."""
    rng = np.random.default_rng(11)
    p = rng.random((3, 300), dtype=F)
    p[:, 0], p[:, 1] = 0.0, 1.0
    ok = _case("e-16", p, np.full((3, 1), 32.25 / 64), 7.5 / 64, 64, 300)
    over = _case("e-17", p, np.full((3, 1), 32.5 / 64), 8.0 / 64, 64, 300)
    return ok, over


def all_cases(ns=NS):
    out = []
    for n in ns:
        out += cases_random(n)
    return out + cases_lattice() + cases_outside() + cases_degenerate() + [cases_cap()[0]]
