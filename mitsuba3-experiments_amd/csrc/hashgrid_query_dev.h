// hashgrid_query_dev.h — the fixed-radius neighbour walk over a built hash
// grid (prims.hip hashgrid_build), one per-lane function templated on a
// visitor. photon.hip's kernels are its three visitors.
//
// Walk order (part of the interface: every consumer's summation order rests
// on it): grid cells ascend in cz, then cy, then cx; inside a grid cell the
// samples follow the grid's own order, ascending sample index. Several grid
// cells share a hash cell, so every candidate's own cell coordinates are
// recomputed and compared with the grid cell being walked: a sample belongs
// to exactly one grid cell and is visited exactly once per query.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mtx.h"

namespace mtxd {

// mtx_hashgrid_view with the sample count narrowed (the entries refuse n >= 2^31).
struct HgView {
  const float *p;  // (3, n)
  uint32_t n;
  float bbmin, bbmax;
  uint32_t res, n_cells;
  const uint32_t *cell_size, *cell_offset, *sample_idx;
};

// Cell coordinate of a value: the build's formula (prims.hip hg_cell,
// hashgrid.py:86-90), (uint32)((x - bbmin) / ext * (float)res). A negative or
// NaN argument gives 0 (what the device conversion gives the build for 0 / 0),
// the argument is clamped to res from above (the point at bbmax has
// coordinate res), and without a positive extent every coordinate is 0.
// Monotone in x: every operation is a correctly rounded monotone function of
// x with its other operand fixed.
__device__ __forceinline__ uint32_t hg_coord(float x, float bbmin, float ext, float fres) {
  if (!(ext > 0.f)) return 0u;
  const float a = (x - bbmin) / ext * fres;
  if (!(a > 0.f)) return 0u;
  return (uint32_t)(a > fres ? fres : a);
}
__device__ __forceinline__ uint32_t hg_hash(uint32_t x, uint32_t y, uint32_t z, uint32_t n_cells) {
  return ((x * 73856093u) ^ (y * 19349663u) ^ (z * 83492791u)) % n_cells;
}

// The neighbouring float towards -inf / +inf (NaN and that infinity stay).
__device__ __forceinline__ float hg_next_down(float x) {
  if (!(x > -__builtin_inff())) return x;
  if (x == 0.f) return -__uint_as_float(1u);
  const uint32_t b = __float_as_uint(x);
  return __uint_as_float(x > 0.f ? b - 1u : b + 1u);
}
__device__ __forceinline__ float hg_next_up(float x) { return -hg_next_down(-x); }

struct HgBox {
  uint32_t lo[3], hi[3];
};

// The cell box of a query: c(lo) .. c(hi) per axis, conservative with respect
// to the fp32 distance test of hg_walk. Returns 0: walk it; 1: no neighbour
// can exist (NaN in q or r, or r < 0); 2: more than MTX_HG_MAX_QUERY_CELLS.
//
// Why the box is conservative. Let u = 2^-24. A sample coordinate p passes
// only if fl(dx dx) <= d2 <= fl(r r) with dx = fl(p - q): adding the other
// axes' non-negative squares and rounding never decreases a partial sum.
// fl(r r) <= r^2 (1 + u), and fl(dx dx) >= dx^2 (1 - u) unless the square
// underflows, which needs |dx| < 2^-63. So |dx| <= r (1 + 2u) + 2^-63. The
// subtraction rounds once and cannot underflow: |p - q| <= |dx| / (1 - u) <=
// r (1 + 5u) + 2^-62 =: w. The code forms wf = fl(fl(r * (1 + 16u)) + 2^-60)
// >= r (1 + 16u)(1 - u)^2 + 2^-60 (1 - u) >= w, then fl(q -+ wf), which is
// within half an ulp of q -+ wf, and steps one float outward: the result is
// <= q - wf <= q - w on the low side and >= q + w on the high side whatever
// the magnitudes of q and r. c is monotone, so c(lo) <= c(p) <= c(hi) for
// every p that can pass. A NaN bound (inf - inf) opens the whole axis.
__device__ __forceinline__ int hg_box(const HgView &g, float qx, float qy, float qz, float r, HgBox *b) {
  if (!(r >= 0.f) || qx != qx || qy != qy || qz != qz) return 1;
  const float ext = g.bbmax - g.bbmin, fres = (float)g.res;
  const float wf = r * 1.00000095367431640625f + 8.673617379884035e-19f;  // 1 + 2^-20, 2^-60
  const float q[3] = {qx, qy, qz};
  uint64_t cells = 1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = hg_next_down(q[a] - wf), hi = hg_next_up(q[a] + wf);
    b->lo[a] = lo != lo ? 0u : hg_coord(lo, g.bbmin, ext, fres);
    b->hi[a] = hi != hi ? hg_coord(__builtin_inff(), g.bbmin, ext, fres) : hg_coord(hi, g.bbmin, ext, fres);
    const uint32_t span = b->hi[a] - b->lo[a] + 1u;  // hi >= lo: c is monotone and hi >= lo as floats
    if (span > MTX_HG_MAX_QUERY_CELLS) return 2;
    cells *= span;
  }
  return cells > MTX_HG_MAX_QUERY_CELLS ? 2 : 0;
}

// Calls visit(j, px, py, pz) for every sample j within r of q, in walk order.
// The distance test, fp32 without contraction: d2 = (dx dx + dy dy) + dz dz
// with dx = p.x - q.x, ...; a neighbour iff d2 <= r r. Nothing is loaded
// through an unchecked index: a slot past the grid's n samples ends the cell,
// and a sample index >= n is skipped before p is read through it.
template <class Visit>
__device__ __forceinline__ void hg_walk(const HgView &g, const HgBox &b, float qx, float qy, float qz, float r,
                                        Visit &&visit) {
  const float ext = g.bbmax - g.bbmin, fres = (float)g.res, r2 = r * r;
  const size_t n = g.n;
  for (uint32_t cz = b.lo[2]; cz <= b.hi[2]; ++cz)
    for (uint32_t cy = b.lo[1]; cy <= b.hi[1]; ++cy)
      for (uint32_t cx = b.lo[0]; cx <= b.hi[0]; ++cx) {
        const uint32_t h = hg_hash(cx, cy, cz, g.n_cells);
        const uint32_t size = g.cell_size[h], off = g.cell_offset[h];
        for (uint32_t k = 0; k < size; ++k) {
          const uint64_t slot = (uint64_t)off + k;
          if (slot >= n) break;
          const uint32_t j = g.sample_idx[slot];
          if (j >= g.n) continue;
          const float px = g.p[j], py = g.p[n + j], pz = g.p[2 * n + j];
          if (hg_coord(px, g.bbmin, ext, fres) != cx || hg_coord(py, g.bbmin, ext, fres) != cy ||
              hg_coord(pz, g.bbmin, ext, fres) != cz)
            continue;
          const float dx = px - qx, dy = py - qy, dz = pz - qz;
          const float d2 = (dx * dx + dy * dy) + dz * dz;
          if (d2 <= r2) visit(j, px, py, pz);
        }
      }
}

}  // namespace mtxd
