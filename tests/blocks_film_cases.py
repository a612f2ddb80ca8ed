"""Shared by tests/test_blocks_film.py (CPU) and tests/test_blocks_film_gpu.py:
a numpy float32 restatement of ``blocks.Film.put`` / ``raw`` for ragged
per-pixel sample counts, and the oracle's samples of the band the tests use.

The restatement follows include/mtx.h (mtx_blocks_film_put_dev): per source
pixel the kept samples are ranked in the order given, sample r falls into slot
film_slot(sample_offset + r, T) with T = spp_total or the pixel's own count,
every slot's K = (2n+1)^2 accumulators add ``L * w`` and ``w`` one float32
operation at a time, a film pixel gathers its K neighbours in (dy, dx) order
and the 8 slots combine by the fixed tree. The weights, the gather and the
tree are tests/test_rfilter_gpu.py's (anchored there to the oracle's film).
"""
import numpy as np
from test_rfilter_gpu import REACH, _gather, _weight

F32 = np.float32
Y0, Y1 = 3, 9          # the band of the 64x36 small scene
SPPS = (1, 3, 8, 9)    # fewer samples than slots, exactly 8, uneven slots


def film_slots(g, T):
    """film_slot (mtx_core/common.h) on arrays: the k < 7 with slot_end(k) <= g counted."""
    g, T = np.asarray(g, np.uint64), np.asarray(T, np.uint64)
    k = np.zeros(g.shape, np.int64)
    for j in range(7):
        k += (((j + 1) * T) >> np.uint64(3)) <= g
    return k


def planes_np(oracle, fid, width, y0, y1, pix, L, pos, spp_total=None, sample_offset=0, planes=None):
    """The contribution planes [8, D, D, rows, W, 4] after putting the samples
    (pix: band pixel index (y - y0) * W + x, L (n, 3), pos (n, 2)), which are
    given in the order they rank in within a pixel. `planes`: continue from these."""
    n = REACH[fid]
    D = 2 * n + 1
    rows, W = y1 - y0, width
    pix = np.asarray(pix, np.int64)
    L, pos = np.asarray(L, F32).reshape(-1, 3), np.asarray(pos, F32).reshape(-1, 2)
    acc = np.zeros((8, D, D, rows, W, 4), F32) if planes is None else planes.copy()
    count = np.bincount(pix, minlength=rows * W)
    order = np.argsort(pix, kind="stable")
    start = np.cumsum(count) - count
    rank = np.empty(len(pix), np.int64)
    rank[order] = np.arange(len(pix)) - start[pix[order]]
    T = count[pix] if spp_total is None else np.full(len(pix), spp_total)
    slot = film_slots(sample_offset + rank, T)
    py, px = pix // W, pix % W
    for r in range(int(rank.max()) + 1 if len(pix) else 0):
        m = rank == r  # at most one sample per pixel: the updates of a round do not collide
        sx, sy = pos[m, 0], pos[m, 1]
        x, y, s = px[m], py[m], slot[m]
        wx = [_weight(oracle, fid, sx - ((x + dx - n).astype(F32) + F32(0.5))) for dx in range(D)]
        wy = [_weight(oracle, fid, sy - ((y + y0 + dy - n).astype(F32) + F32(0.5))) for dy in range(D)]
        for dy in range(D):
            for dx in range(D):
                w = wx[dx] * wy[dy]
                for c in range(3):
                    acc[s, dy, dx, y, x, c] = acc[s, dy, dx, y, x, c] + L[m, c] * w
                acc[s, dy, dx, y, x, 3] = acc[s, dy, dx, y, x, 3] + w
    assert acc.dtype == F32
    return acc


def raw_np(planes):
    """The raw film of planes [8, D, D, rows, W, 4]."""
    n = (planes.shape[1] - 1) // 2
    sl = [_gather(planes[s], n) for s in range(8)]
    return ((sl[0] + sl[1]) + (sl[2] + sl[3])) + ((sl[4] + sl[5]) + (sl[6] + sl[7]))


def device_layout(planes):
    """[8, D, D, rows, W, 4] -> blocks.Film.planes' (8, K, band_px, 4)."""
    s, D, _, rows, W, _ = planes.shape
    return planes.reshape(s, D * D, rows * W, 4)


_SAMPLES = {}


def band_samples(scene, oracle, spp, spp_total=None, sample_offset=0, name="path_test", seed=3):
    """(args, L (n, 3), pos (n, 2), pix (n,)) of the oracle's samples on the
    band, in (pixel, sample) order; computed once and left read-only."""
    key = (id(scene), name, seed, spp, spp_total, sample_offset)
    if key not in _SAMPLES:
        from mtx import load_dict

        a = load_dict({"type": name}).render_args(scene, seed, spp, y0=Y0, y1=Y1, spp_total=spp_total,
                                                  sample_offset=sample_offset)
        L, pos = oracle.render_samples(scene, a)
        pix = np.repeat(np.arange((Y1 - Y0) * scene.width), spp)
        # floor(pos) is the pixel that drew the sample (no jitter rounded up to the next pixel in this data),
        # so the source pixel the film takes from the position is the oracle's
        assert (np.floor(pos[:, 0]) == pix % scene.width).all() and (np.floor(pos[:, 1]) == Y0 + pix // scene.width).all()
        for x in (L, pos, pix):
            x.setflags(write=False)
        _SAMPLES[key] = (a, L, pos, pix)
    return _SAMPLES[key]
