// refit.hip — mtx_scene_update_vertices on the device: the counterpart of
// assigning vertex_positions and calling params.update() on mi.traverse of a
// scene, for a scene that lives in HBM. A pre-pass that only reads (extents,
// the vertices' box, refusals), one pass over the triangles, then one launch
// per tree level from the deepest to the root. The node arithmetic is
// mtx_core/refit.h, shared with the host refit, so the device's nodes equal
// the host's bit for bit.
//
// A level launch has no dependencies inside it: a node reads its children's
// boxes, written by the previous (deeper) launch on the same stream, and
// writes its own. One thread per node: the per-child loop keeps the shared
// host/device code in one piece; the passes are bound by the triangle pass's
// traffic, not by the levels.
//
// Mesh emitters move with their vertices: their tables in `tables` (mtx.h:
// pmf the fp32 triangle areas, cdf the inclusive prefix accumulated
// sequentially in double, in entry order, and stored as float) are rebuilt in
// the pre-pass into scratch and committed once every check has passed.
//   areas  one thread per entry: prim -> tri_vidx -> the new vpos ->
//          mtx::tri_area; per block (wave reductions, no atomics: the blocks
//          of a large light would all meet on four words) the bits of the
//          largest and of the smallest non-zero area, the first / last entry
//          with pmf > 0 and the double sum of its areas.
//   reduce one block per emitter folds its blocks' four words (min and max:
//          any order).
//   scan   A parallel scan adds in another order than the definition, so it
//          runs only where the order provably cannot matter
//          (mtx::prefix_order_free, mtx_core/discrete.h): with M = ilogb of
//          the largest area, m = max(ilogb(smallest non-zero area), -126) - 23
//          and n entries, every partial sum of every subset of the areas is a
//          non-negative multiple of 2^m below 2^(M + 1 + ceil(log2 n)); if
//          M + 1 + ceil(log2 n) - m <= 53 each such sum is a double, no
//          addition in any association rounds, and the block sums, the wave
//          scans and their offsets all equal the sequential prefix. An
//          emitter that fails the predicate takes the ordered fallback: one
//          wave stages 1024 entries at a time through LDS and lane 0 adds
//          them in entry order. Slow, and exactly the definition.
//   finish sum = cdf[n - 1], norm = 1 / sum (one fp32 division); no entry
//          with pmf > 0, a non-finite area, or a sum or norm that is not
//          finite and positive is RF_BAD_AREA.
#include "refit.h"

#include "mtx_core/discrete.h"
#include "mtx_core/refit.h"

namespace mtxd {

namespace {

constexpr int kBlock = 256;

// fp32 -> u32 key with the same order (negative values below positive ones).
__device__ __forceinline__ uint32_t order_key(float x) {
  const uint32_t b = mtx::f2u(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

__global__ void k_refit_state_init(uint32_t *state) {
  const uint32_t i = threadIdx.x;
  if (i < RF_WORDS) state[i] = ((i >= RF_LO && i < RF_LO + 3) || i == RF_EM) ? 0xffffffffu : 0u;
}

// All vertices: finite and within the bound; their box (the environment's
// bounding sphere). Every lane takes part in the wave reductions.
__global__ __launch_bounds__(kBlock) void k_refit_verts(const float *__restrict__ vpos, uint32_t n_verts,
                                                        uint32_t *state) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, bad = 0u;
  if (i < n_verts) {
    for (int a = 0; a < 3; ++a) {
      const float x = vpos[3 * (size_t)i + a];
      if (!(fabsf(x) <= mtx::kRefitMaxCoord)) bad = RF_BAD_COORD;  // also NaN
      lo[a] = hi[a] = order_key(x);
    }
  }
  bad = wave_or_u32(bad);
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_min_u32(lo[a]);
    hi[a] = wave_max_u32(hi[a]);
  }
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicOr(&state[RF_FLAGS], bad);
    for (int a = 0; a < 3; ++a) {
      atomicMin(&state[RF_LO + a], lo[a]);
      atomicMax(&state[RF_HI + a], hi[a]);
    }
  }
}

// Leaf-order triangles: the two extents, the occlusion points' bound, and
// that no triangle of a rectangle-emitter shape moves (its vertices against
// the position rows of its shading record; the record of a rectangle emitter
// has a non-zero normal, mtx.h).
__global__ __launch_bounds__(kBlock) void k_refit_check_tris(const float *__restrict__ vpos,
                                                             const uint32_t *__restrict__ tri_vidx,
                                                             const uint32_t *__restrict__ tri_shape,
                                                             const mtx_shape *__restrict__ shapes,
                                                             const mtx_emitter *__restrict__ emitters,
                                                             const float *__restrict__ shade_rec, uint32_t n_tris,
                                                             uint32_t *state) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  uint32_t ext = 0u, occ_ext = 0u, bad = 0u;
  if (t < n_tris) {
    float p[3][3];
    for (int k = 0; k < 3; ++k) {
      const uint32_t vi = tri_vidx[3 * (size_t)t + k];
      for (int a = 0; a < 3; ++a) {
        p[k][a] = vpos[3 * (size_t)vi + a];
        const uint32_t b = mtx::abs_bits(p[k][a]);
        ext = b > ext ? b : ext;
      }
    }
    float v0[3], e1[3], e2[3], pts[9];
    mtx::tri_record(p[0], p[1], p[2], v0, e1, e2);
    mtx::occ_points(v0, e1, e2, pts);
    for (int j = 0; j < 9; ++j) {
      if (!(fabsf(pts[j]) <= mtx::kRefitMaxPoint)) bad |= RF_BAD_COORD;
      const uint32_t b = mtx::abs_bits(pts[j]);
      occ_ext = b > occ_ext ? b : occ_ext;
    }
    const int32_t em = shapes[tri_shape[t]].emitter;
    if (em >= 0 && !(emitters[em].normal[0] == 0.f && emitters[em].normal[1] == 0.f && emitters[em].normal[2] == 0.f)) {
      const float *r = shade_rec + 32 * (size_t)t;
      for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a)
          if (mtx::f2u(r[4 * k + a]) != mtx::f2u(p[k][a])) bad |= RF_BAD_EMITTER;
    }
  }
  ext = wave_max_u32(ext);
  occ_ext = wave_max_u32(occ_ext);
  bad = wave_or_u32(bad);
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicOr(&state[RF_FLAGS], bad);
    atomicMax(&state[RF_EXTENT], ext);
    atomicMax(&state[RF_OCC_EXTENT], occ_ext);
  }
}

__global__ __launch_bounds__(kBlock) void k_refit_triangles(const float *__restrict__ vpos,
                                                            const float *__restrict__ vnormal,
                                                            const uint32_t *__restrict__ tri_vidx, uint32_t n_tris,
                                                            float *__restrict__ tri, float *__restrict__ shade_rec,
                                                            float *__restrict__ tbox) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_tris) return;
  float p[3][3];
  uint32_t vi[3];
  for (int k = 0; k < 3; ++k) {
    vi[k] = tri_vidx[3 * (size_t)t + k];
    for (int a = 0; a < 3; ++a) p[k][a] = vpos[3 * (size_t)vi[k] + a];
  }
  float *g = tri + 9 * (size_t)t;
  mtx::tri_record(p[0], p[1], p[2], g, g + 3, g + 6);
  float *r = shade_rec + 32 * (size_t)t;
  // words 3, 7, 11 (material, emitter, flags) and the uv block stay
  const uint32_t fl = mtx::f2u(r[11]);
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) r[4 * k + a] = p[k][a];
  if (vnormal && (fl & 1u))
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) r[12 + 4 * k + a] = vnormal[3 * (size_t)vi[k] + a];
  float b[6];
  mtx::box_reset(b);
  for (int k = 0; k < 3; ++k) mtx::box_grow_point(b, p[k]);
  for (int j = 0; j < 6; ++j) tbox[6 * (size_t)t + j] = b[j];
}

__global__ __launch_bounds__(kBlock) void k_refit_occ_gather(const float *__restrict__ tri,
                                                             const uint32_t *__restrict__ occ_perm, uint32_t n_tris,
                                                             float *__restrict__ occ_tri, float *__restrict__ tbox) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_tris) return;
  const uint32_t j = occ_perm[i];
  float g[9];
  for (int w = 0; w < 9; ++w) g[w] = tri[9 * (size_t)j + w];
  for (int w = 0; w < 9; ++w) occ_tri[9 * (size_t)i + w] = g[w];
  float pts[9], b[6];
  mtx::occ_points(g, g + 3, g + 6, pts);
  mtx::box_reset(b);
  for (int k = 0; k < 3; ++k) mtx::box_grow_point(b, pts + 3 * k);
  for (int w = 0; w < 6; ++w) tbox[6 * (size_t)i + w] = b[w];
}

__global__ __launch_bounds__(kBlock) void k_refit_level4(int32_t *nodes, uint32_t first, uint32_t count,
                                                         const uint32_t *__restrict__ list, const float *tbox,
                                                         float *nbox, float extent, uint32_t *state) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const uint32_t nd = list ? list[first + i] : first + i;
  int32_t W[MTX_BVH_NODE_WORDS];
  int32_t *N = nodes + MTX_BVH_NODE_WORDS * (size_t)nd;
  for (int w = 0; w < MTX_BVH_NODE_WORDS; ++w) W[w] = N[w];
  float self[6];
  const bool ok = mtx::refit_node4(W, tbox, nbox, extent, self);
  for (int w = 0; w < 4; ++w) N[w] = W[w];
  for (int w = 8; w < 14; ++w) N[w] = W[w];
  for (int w = 0; w < 6; ++w) nbox[6 * (size_t)nd + w] = self[w];
  if (!ok) atomicOr(&state[RF_FLAGS], (uint32_t)RF_BAD_QUANT);
}

__global__ __launch_bounds__(kBlock) void k_refit_level8(uint32_t *nodes, uint32_t first, uint32_t count,
                                                         const uint32_t *__restrict__ list, const float *tbox,
                                                         float *nbox, float extent, uint32_t *state) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const uint32_t nd = list ? list[first + i] : first + i;
  uint32_t W[MTX_OCC_NODE_WORDS];
  uint32_t *N = nodes + MTX_OCC_NODE_WORDS * (size_t)nd;
  for (int w = 0; w < MTX_OCC_NODE_WORDS; ++w) W[w] = N[w];
  float self[6];
  const bool ok = mtx::refit_node8(W, tbox, nbox, extent, self);
  for (int w = 0; w < 4; ++w) N[w] = W[w];
  for (int w = 8; w < MTX_OCC_NODE_WORDS; ++w) N[w] = W[w];
  for (int w = 0; w < 6; ++w) nbox[6 * (size_t)nd + w] = self[w];
  if (!ok) atomicOr(&state[RF_FLAGS], (uint32_t)RF_BAD_QUANT);
}

// ------------------------------------------------- mesh emitter tables --
static_assert(kEmBlock == 256, "four waves per block below");

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// 1: block-parallel scan, 2: ordered fallback, 0: refused (no scan).
__device__ __forceinline__ uint32_t em_path(const uint32_t *st, uint32_t n) {
  if (st[EM_MAX] >= 0x7f800000u || st[EM_LO] == 0xffffffffu) return 0u;
  return mtx::prefix_order_free(st[EM_MAX], st[EM_MIN], n) ? 1u : 2u;
}

__global__ __launch_bounds__(kEmBlock) void k_em_areas(EmTables t, const float *__restrict__ vpos,
                                                       const uint32_t *__restrict__ tri_vidx,
                                                       const float *__restrict__ tables) {
  __shared__ double wsum[4];
  __shared__ uint32_t wst[4][4];
  const EmBlock b = t.blocks[blockIdx.x];
  const EmSlot s = t.slots[b.slot];
  const uint32_t k = b.first + threadIdx.x;
  const bool in = k < s.count;
  float a = 0.f;
  if (in) {
    const uint32_t prim = mtx::f2u(tables[(size_t)s.offset + 2 * (size_t)s.count + k]);
    mtx::V3 p[3];
    for (int j = 0; j < 3; ++j) {
      const uint32_t vi = tri_vidx[3 * (size_t)prim + j];
      p[j] = mtx::v3(vpos[3 * (size_t)vi], vpos[3 * (size_t)vi + 1], vpos[3 * (size_t)vi + 2]);
    }
    a = mtx::tri_area(p[0], p[1], p[2]);
    t.pmf[(size_t)s.flat + k] = a;
  }
  const bool pos = in && a > 0.f;
  const uint32_t mx = wave_max_u32(in ? mtx::f2u(a) : 0u), mn = wave_min_u32(pos ? mtx::f2u(a) : 0xffffffffu);
  const uint32_t lo = wave_min_u32(pos ? k : 0xffffffffu), hi = wave_max_u32(pos ? k : 0u);
  const double ws = wave_sum_f64(in ? (double)a : 0.0);
  if ((threadIdx.x & 63) == 0) {
    uint32_t *w = wst[threadIdx.x >> 6];
    w[EM_MAX] = mx;
    w[EM_MIN] = mn;
    w[EM_LO] = lo;
    w[EM_HI] = hi;
    wsum[threadIdx.x >> 6] = ws;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    t.bsum[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    uint32_t *o = t.bstat + 4 * (size_t)blockIdx.x;
    o[EM_MAX] = max(max(wst[0][EM_MAX], wst[1][EM_MAX]), max(wst[2][EM_MAX], wst[3][EM_MAX]));
    o[EM_MIN] = min(min(wst[0][EM_MIN], wst[1][EM_MIN]), min(wst[2][EM_MIN], wst[3][EM_MIN]));
    o[EM_LO] = min(min(wst[0][EM_LO], wst[1][EM_LO]), min(wst[2][EM_LO], wst[3][EM_LO]));
    o[EM_HI] = max(max(wst[0][EM_HI], wst[1][EM_HI]), max(wst[2][EM_HI], wst[3][EM_HI]));
  }
}

// One block per emitter: its blocks' words into its state.
__global__ __launch_bounds__(kEmBlock) void k_em_reduce(EmTables t) {
  __shared__ uint32_t wst[4][4];
  const EmSlot s = t.slots[blockIdx.x];
  const uint32_t nb = (s.count + kEmBlock - 1) / kEmBlock;
  uint32_t mx = 0u, mn = 0xffffffffu, lo = 0xffffffffu, hi = 0u;
  for (uint32_t i = threadIdx.x; i < nb; i += kEmBlock) {
    const uint32_t *b = t.bstat + 4 * (size_t)(s.block + i);
    mx = max(mx, b[EM_MAX]);
    mn = min(mn, b[EM_MIN]);
    lo = min(lo, b[EM_LO]);
    hi = max(hi, b[EM_HI]);
  }
  mx = wave_max_u32(mx);
  mn = wave_min_u32(mn);
  lo = wave_min_u32(lo);
  hi = wave_max_u32(hi);
  if ((threadIdx.x & 63) == 0) {
    uint32_t *w = wst[threadIdx.x >> 6];
    w[EM_MAX] = mx;
    w[EM_MIN] = mn;
    w[EM_LO] = lo;
    w[EM_HI] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t *st = t.state + EM_WORDS * (size_t)blockIdx.x;
    st[EM_MAX] = max(max(wst[0][EM_MAX], wst[1][EM_MAX]), max(wst[2][EM_MAX], wst[3][EM_MAX]));
    st[EM_MIN] = min(min(wst[0][EM_MIN], wst[1][EM_MIN]), min(wst[2][EM_MIN], wst[3][EM_MIN]));
    st[EM_LO] = min(min(wst[0][EM_LO], wst[1][EM_LO]), min(wst[2][EM_LO], wst[3][EM_LO]));
    st[EM_HI] = max(max(wst[0][EM_HI], wst[1][EM_HI]), max(wst[2][EM_HI], wst[3][EM_HI]));
  }
}

// Emitters that satisfy mtx::prefix_order_free: every sum below is exact, so
// its order is free (the header comment).
__global__ __launch_bounds__(kEmBlock) void k_em_scan(EmTables t) {
  __shared__ double woff[4], wtot[4];
  const EmBlock b = t.blocks[blockIdx.x];
  const EmSlot s = t.slots[b.slot];
  if (em_path(t.state + EM_WORDS * (size_t)b.slot, s.count) != 1u) return;  // the whole block
  const uint32_t before = b.first / kEmBlock, base = blockIdx.x - before;  // this emitter's earlier blocks
  double off = 0.0;
  for (uint32_t i = threadIdx.x; i < before; i += kEmBlock) off += t.bsum[base + i];
  off = wave_sum_f64(off);
  const uint32_t k = b.first + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool in = k < s.count;
  double v = in ? (double)t.pmf[(size_t)s.flat + k] : 0.0;
  for (int o = 1; o < 64; o <<= 1) {
    const double w = __shfl_up(v, o, 64);
    if ((int)lane >= o) v += w;
  }
  if (lane == 0) woff[wv] = off;
  if (lane == 63) wtot[wv] = v;
  __syncthreads();
  double add = ((woff[0] + woff[1]) + woff[2]) + woff[3];
  for (uint32_t w = 0; w < wv; ++w) add += wtot[w];
  if (in) t.cdf[(size_t)s.flat + k] = (float)(add + v);
}

// The others: the definition itself. One wave per emitter; lane 0 adds in
// entry order, the wave moves the data.
__global__ __launch_bounds__(64) void k_em_scan_ordered(EmTables t) {
  constexpr uint32_t kChunk = 1024;
  __shared__ float buf[kChunk];
  const EmSlot s = t.slots[blockIdx.x];
  if (em_path(t.state + EM_WORDS * (size_t)blockIdx.x, s.count) != 2u) return;
  double acc = 0.0;  // lane 0's
  for (uint32_t c = 0; c < s.count; c += kChunk) {
    const uint32_t m = s.count - c < kChunk ? s.count - c : kChunk;
    for (uint32_t i = threadIdx.x; i < m; i += 64) buf[i] = t.pmf[(size_t)s.flat + c + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (uint32_t i = 0; i < m; ++i) {
        acc += (double)buf[i];
        buf[i] = (float)acc;
      }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m; i += 64) t.cdf[(size_t)s.flat + c + i] = buf[i];
    __syncthreads();
  }
}

__global__ void k_em_finish(EmTables t, uint32_t *state) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= t.n_slots) return;
  const EmSlot s = t.slots[i];
  uint32_t *st = t.state + EM_WORDS * (size_t)i;
  const uint32_t path = em_path(st, s.count);
  bool ok = path != 0u;
  if (ok) {
    const float sum = t.cdf[(size_t)s.flat + s.count - 1], norm = 1.f / sum;
    ok = sum > 0.f && mtx::isfinite_(sum) && norm > 0.f && mtx::isfinite_(norm);
    st[EM_SUM] = mtx::f2u(sum);
    st[EM_NORM] = mtx::f2u(norm);
  }
  st[EM_PATH] = ok ? path : 0u;
  if (!ok) {
    atomicOr(&state[RF_FLAGS], (uint32_t)RF_BAD_AREA);
    atomicMin(&state[RF_EM], s.emitter);
  }
}

__global__ __launch_bounds__(kEmBlock) void k_em_commit(EmTables t, float *__restrict__ tables,
                                                        mtx_emitter *__restrict__ emitters) {
  const EmBlock b = t.blocks[blockIdx.x];
  const EmSlot s = t.slots[b.slot];
  const uint32_t k = b.first + threadIdx.x;
  if (k < s.count) {
    tables[(size_t)s.offset + k] = t.pmf[(size_t)s.flat + k];
    tables[(size_t)s.offset + s.count + k] = t.cdf[(size_t)s.flat + k];
  }
  if (k == 0) {
    const uint32_t *st = t.state + EM_WORDS * (size_t)b.slot;
    mtx_emitter &e = emitters[s.emitter];
    e.mesh_valid_lo = st[EM_LO];
    e.mesh_valid_hi = st[EM_HI];
    e.mesh_sum = mtx::u2f(st[EM_SUM]);
    e.mesh_norm = mtx::u2f(st[EM_NORM]);
    e.inv_area = mtx::u2f(st[EM_NORM]);
  }
}

inline unsigned blocks(uint32_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

float refit_key_decode(uint32_t key) { return mtx::u2f((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

void refit_state_init(uint32_t *state, hipStream_t st) { hipLaunchKernelGGL(k_refit_state_init, 1, 64, 0, st, state); }

void refit_prepass(const float *vpos, uint32_t n_verts, const uint32_t *tri_vidx, const uint32_t *tri_shape,
                   const mtx_shape *shapes, const mtx_emitter *emitters, const float *shade_rec, uint32_t n_tris,
                   uint32_t *state, hipStream_t st) {
  hipLaunchKernelGGL(k_refit_verts, blocks(n_verts), kBlock, 0, st, vpos, n_verts, state);
  hipLaunchKernelGGL(k_refit_check_tris, blocks(n_tris), kBlock, 0, st, vpos, tri_vidx, tri_shape, shapes, emitters,
                     shade_rec, n_tris, state);
}

void refit_emitter_tables(const EmTables &t, const float *vpos, const uint32_t *tri_vidx, const float *tables,
                          uint32_t *state, hipStream_t st) {
  if (t.n_slots == 0) return;
  hipLaunchKernelGGL(k_em_areas, t.n_blocks, kEmBlock, 0, st, t, vpos, tri_vidx, tables);
  hipLaunchKernelGGL(k_em_reduce, t.n_slots, kEmBlock, 0, st, t);
  hipLaunchKernelGGL(k_em_scan, t.n_blocks, kEmBlock, 0, st, t);
  hipLaunchKernelGGL(k_em_scan_ordered, t.n_slots, 64, 0, st, t);
  hipLaunchKernelGGL(k_em_finish, blocks(t.n_slots), kBlock, 0, st, t, state);
}

void refit_emitter_commit(const EmTables &t, float *tables, mtx_emitter *emitters, hipStream_t st) {
  if (t.n_slots == 0) return;
  hipLaunchKernelGGL(k_em_commit, t.n_blocks, kEmBlock, 0, st, t, tables, emitters);
}

void refit_triangles(const float *vpos, const float *vnormal, const uint32_t *tri_vidx, uint32_t n_tris, float *tri,
                     float *shade_rec, float *tbox, hipStream_t st) {
  hipLaunchKernelGGL(k_refit_triangles, blocks(n_tris), kBlock, 0, st, vpos, vnormal, tri_vidx, n_tris, tri, shade_rec,
                     tbox);
}

void refit_occ_gather(const float *tri, const uint32_t *occ_perm, uint32_t n_tris, float *occ_tri, float *tbox,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_refit_occ_gather, blocks(n_tris), kBlock, 0, st, tri, occ_perm, n_tris, occ_tri, tbox);
}

void refit_level4(int32_t *nodes, uint32_t first, uint32_t count, const uint32_t *list, const float *tbox, float *nbox,
                  float extent, uint32_t *state, hipStream_t st) {
  if (count == 0) return;
  hipLaunchKernelGGL(k_refit_level4, blocks(count), kBlock, 0, st, nodes, first, count, list, tbox, nbox, extent,
                     state);
}

void refit_level8(uint32_t *occ_nodes, uint32_t first, uint32_t count, const uint32_t *list, const float *tbox,
                  float *nbox, float extent, uint32_t *state, hipStream_t st) {
  if (count == 0) return;
  hipLaunchKernelGGL(k_refit_level8, blocks(count), kBlock, 0, st, occ_nodes, first, count, list, tbox, nbox, extent,
                     state);
}

}  // namespace mtxd
