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
#include "refit.h"

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
  if (i < RF_WORDS) state[i] = (i >= RF_LO && i < RF_LO + 3) ? 0xffffffffu : 0u;
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
// that no triangle of an emitter shape moves (its vertices against the
// position rows of its shading record).
__global__ __launch_bounds__(kBlock) void k_refit_check_tris(const float *__restrict__ vpos,
                                                             const uint32_t *__restrict__ tri_vidx,
                                                             const uint32_t *__restrict__ tri_shape,
                                                             const mtx_shape *__restrict__ shapes,
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
    if (shapes[tri_shape[t]].emitter >= 0) {
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

inline unsigned blocks(uint32_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

float refit_key_decode(uint32_t key) { return mtx::u2f((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

void refit_state_init(uint32_t *state, hipStream_t st) { hipLaunchKernelGGL(k_refit_state_init, 1, 64, 0, st, state); }

void refit_prepass(const float *vpos, uint32_t n_verts, const uint32_t *tri_vidx, const uint32_t *tri_shape,
                   const mtx_shape *shapes, const float *shade_rec, uint32_t n_tris, uint32_t *state, hipStream_t st) {
  hipLaunchKernelGGL(k_refit_verts, blocks(n_verts), kBlock, 0, st, vpos, n_verts, state);
  hipLaunchKernelGGL(k_refit_check_tris, blocks(n_tris), kBlock, 0, st, vpos, tri_vidx, tri_shape, shapes, shade_rec,
                     n_tris, state);
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
