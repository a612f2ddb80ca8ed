// blocks.hip — the device-tensor building blocks (mtx.h "building blocks"):
// thin wavefront-wide kernels over the per-lane functions of mtx_core, the
// same ones the fixed integrator kernels and the oracle call. One lane
// handles one item in a grid-stride loop; nothing is persistent. Every
// quantity is a (C, N) SoA plane set, so a wave reads and writes whole 256-B
// lines per plane.
//
// Indices that arrive in caller tensors (prim, material, emitter) are
// compared against the scene's counts before any load that depends on them;
// a lane with one out of range is counted in `bad` and handled as invalid.
#include "blocks.h"

#include <algorithm>

#include "device_common.h"

namespace mtxd {

namespace {

constexpr int kBlkBlock = 256;

__device__ __forceinline__ V3 ld3(const float *a, uint32_t n, uint32_t i) {
  return V3{a[i], a[(size_t)n + i], a[2 * (size_t)n + i]};
}
__device__ __forceinline__ V2 ld2(const float *a, uint32_t n, uint32_t i) { return V2{a[i], a[(size_t)n + i]}; }
__device__ __forceinline__ void st3(float *a, uint32_t n, uint32_t i, V3 v) {
  a[i] = v.x;
  a[(size_t)n + i] = v.y;
  a[2 * (size_t)n + i] = v.z;
}
__device__ __forceinline__ void st2(float *a, uint32_t n, uint32_t i, V2 v) {
  a[i] = v.x;
  a[(size_t)n + i] = v.y;
}
__device__ __forceinline__ bool lane_on(const uint8_t *active, uint32_t i) { return !active || active[i] != 0; }

__device__ __forceinline__ void store_si(const mtx_si_planes &o, uint32_t n, uint32_t i, const SurfaceInteraction &si,
                                         float bu, float bv) {
  st3(o.p, n, i, si.p);
  st3(o.n, n, i, si.n);
  st3(o.sh_n, n, i, si.sh.n);
  st2(o.uv, n, i, si.uv);
  st3(o.wi, n, i, si.wi);
  o.t[i] = si.t;
  o.prim[i] = si.prim;
  o.material[i] = si.material;
  o.emitter[i] = si.emitter;
  if (o.bary) st2(o.bary, n, i, V2{bu, bv});
}

__global__ __launch_bounds__(kBlkBlock) void k_blk_seed(uint32_t n, uint32_t seed, const uint32_t *lanes,
                                                        uint32_t skip, ulonglong2 *state) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    Pcg32 rng = sampler_lane(seed, lanes[i]);
    rng.advance(skip);
    state[i] = make_ulonglong2(rng.state, (unsigned long long)rng.seq);
  }
}

template <int DIMS>
__global__ __launch_bounds__(kBlkBlock) void k_blk_next(uint32_t n, ulonglong2 *state, float *out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const ulonglong2 w = state[i];
    Pcg32 rng;
    rng.state = w.x;
    rng.seq = (uint32_t)w.y;
    if (DIMS == 1) {
      out[i] = rng.next_1d();
    } else {
      st2(out, n, i, rng.next_2d());
    }
    state[i] = make_ulonglong2(rng.state, w.y);
  }
}

// ray_intersect (TRACE: the traversal of mtx_trace, device_common.h
// traverse_closest, on this thread's LDS stack column) and / or the
// interaction of a hit record (compute_si_dev).
template <bool TRACE>
__global__ __launch_bounds__(kTraceBlock) void k_blk_interact(DevScene s, uint32_t n, const float *o, const float *d,
                                                              const float *maxt, const float *ht,
                                                              const uint32_t *hprim, const float *hu, const float *hv,
                                                              const uint8_t *active, mtx_si_planes out,
                                                              uint32_t *bad) {
  extern __shared__ int4 blk_lds[];  // one stack column per thread (device_common.h stack_bytes)
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const V3 rd = ld3(d, n, i);
    if (!lane_on(active, i)) {
      store_si(out, n, i, si_invalid(kInf, 0xffffffffu, rd), 0.f, 0.f);
      continue;
    }
    float t, bu = 0.f, bv = 0.f;
    uint32_t prim = 0xffffffffu;
    if (TRACE) {
      const float tmax = maxt ? maxt[i] : kLargest;
      const TraceRay r = make_trace_ray(ld3(o, n, i), rd, tmax);
      uint32_t nv = 0, tv = 0;
      t = tmax;
      traverse_closest(s, reinterpret_cast<int32_t *>(blk_lds) + threadIdx.x, r, t, prim, bu, bv, nv, tv);
      if (prim == 0xffffffffu) t = kInf;
    } else {
      t = ht[i];
      prim = hprim[i];
      bu = hu[i];
      bv = hv[i];
      if (prim != 0xffffffffu && prim >= s.n_tris) {  // not a triangle of this scene: a miss, and reported
        atomicAdd(bad, 1u);
        prim = 0xffffffffu;
      }
    }
    store_si(out, n, i, compute_si_dev(s, t, prim, bu, bv, rd), bu, bv);
  }
}

__global__ __launch_bounds__(kTraceBlock) void k_blk_ray_test(DevScene s, uint32_t n, const float *o, const float *d,
                                                              const float *maxt, const uint8_t *active,
                                                              uint8_t *out) {
  extern __shared__ int4 blk_lds[];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    bool occ = false;
    if (lane_on(active, i)) {
      const float tmax = maxt[i];
      const TraceRay r = make_trace_ray(ld3(o, n, i), ld3(d, n, i), tmax);
      uint32_t nv = 0, tv = 0;
      occ = traverse_occ(s, reinterpret_cast<uint32_t *>(blk_lds) + threadIdx.x, r, tmax, nv, tv);
    }
    out[i] = occ ? 1 : 0;
  }
}

__global__ __launch_bounds__(kBlkBlock) void k_blk_spawn(uint32_t n, const float *p, const float *nrm, const float *x,
                                                         int to, float *o, float *d, float *maxt) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const V3 pp = ld3(p, n, i), nn = ld3(nrm, n, i), xx = ld3(x, n, i);
    const Ray r = to ? spawn_ray_to(pp, nn, xx) : spawn_ray(pp, nn, xx);
    st3(o, n, i, r.o);
    st3(d, n, i, r.d);
    maxt[i] = r.maxt;
  }
}

// sample_emitter_direction, and with VIS the oracle's sample_emitter_visible:
// the shadow ray of spawn_ray_to through the any-hit tree in the same lane.
template <bool VIS>
__global__ __launch_bounds__(kTraceBlock) void k_blk_sample_emitter(DevScene s, uint32_t n, const float *p,
                                                                    const float *nrm, const float *u,
                                                                    const uint8_t *active, mtx_ds_planes out,
                                                                    float *weight) {
  extern __shared__ int4 blk_lds[];
  const SceneView view = make_view(s);
  const bool any_emitter = emitter_count(view) != 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    DirectionSample ds;
    ds.p = ds.n = ds.d = v3s(0.f);
    ds.dist = ds.pdf = 0.f;
    ds.emitter = -1;
    V3 w = v3s(0.f);
    if (any_emitter && lane_on(active, i)) {
      const V3 ref = ld3(p, n, i);
      w = sample_emitter_direction(view, ref, ld2(u, n, i), &ds);
      if (VIS) {
        const Ray sr = spawn_ray_to(ref, ld3(nrm, n, i), ds.p);
        const TraceRay r = make_trace_ray(sr.o, sr.d, sr.maxt);
        uint32_t nv = 0, tv = 0;
        if (traverse_occ(s, reinterpret_cast<uint32_t *>(blk_lds) + threadIdx.x, r, sr.maxt, nv, tv)) w = v3s(0.f);
      }
    }
    st3(out.p, n, i, ds.p);
    st3(out.n, n, i, ds.n);
    st3(out.d, n, i, ds.d);
    out.dist[i] = ds.dist;
    out.pdf[i] = ds.pdf;
    out.emitter[i] = ds.emitter;
    st3(weight, n, i, w);
  }
}

__global__ __launch_bounds__(kBlkBlock) void k_blk_emitter(DevScene s, uint32_t n, const int32_t *emitter,
                                                           const float *d, const float *dist, const float *nrm,
                                                           const float *wi, const uint8_t *active, float *pdf,
                                                           float *le, uint32_t *bad) {
  const SceneView view = make_view(s);
  const int32_t count = (int32_t)emitter_count(view);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int32_t e = lane_on(active, i) ? emitter[i] : -1;
    if (e >= count) {  // past the emitter table (and the environment): no emitter, and reported
      atomicAdd(bad, 1u);
      e = -1;
    }
    if (pdf) pdf[i] = pdf_emitter_direction(view, e, ld3(d, n, i), dist[i], ld3(nrm, n, i));
    if (le) st3(le, n, i, emitter_eval(view, e, ld3(wi, n, i)));
  }
}

// eval_pdf_sample (oracle.cpp): lanes of one wave carry different materials;
// the switch of mtx_core/bsdf.h is the dispatch.
template <bool EVAL>
__global__ __launch_bounds__(kBlkBlock) void k_blk_bsdf(DevScene s, uint32_t n_materials, uint32_t n,
                                                        const int32_t *material, const float *uv, const float *wi,
                                                        const float *wo, const float *u1, const float *u2,
                                                        const uint8_t *active, mtx_bsdf_planes out, uint32_t *flags,
                                                        uint32_t *bad) {
  const SceneView view = make_view(s);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int32_t m = lane_on(active, i) ? material[i] : -1;
    if (m >= 0 && (uint32_t)m >= n_materials) {
      atomicAdd(bad, 1u);
      m = -1;
    }
    V3 val = v3s(0.f), weight = v3s(0.f);
    float pdf = 0.f;
    BSDFSample bs;
    bs.wo = v3s(0.f);
    bs.pdf = bs.eta = 0.f;
    bs.type = 0;
    uint32_t fl = 0;
    if (m >= 0) {
      const mtx_material mat = s.materials[m];
      fl = bsdf_flags(mat);
      if (EVAL) {
        const V2 t = ld2(uv, n, i);
        const V3 a = ld3(wi, n, i);
        bsdf_eval_pdf(view.bsdf, mat, t, a, ld3(wo, n, i), &val, &pdf);
        weight = bsdf_sample(view.bsdf, mat, t, a, u1[i], ld2(u2, n, i), &bs);
      }
    }
    if (flags) flags[i] = fl;
    if (EVAL) {
      st3(out.value, n, i, val);
      out.pdf[i] = pdf;
      st3(out.s_wo, n, i, bs.wo);
      out.s_pdf[i] = bs.pdf;
      out.s_eta[i] = bs.eta;
      out.s_type[i] = bs.type;
      st3(out.weight, n, i, weight);
    }
  }
}

__global__ __launch_bounds__(kBlkBlock) void k_blk_math(int op, uint32_t n, const float *a, const float *b,
                                                        const float *c, float *out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    switch (op) {
      case MTX_MATH_FMA: out[i] = fmaf(a[i], b[i], c[i]); break;
      case MTX_MATH_DIV: out[i] = a[i] / b[i]; break;
      case MTX_MATH_RCP: out[i] = rcp(a[i]); break;
      case MTX_MATH_SQRT: out[i] = sqrtf(a[i]); break;
      case MTX_MATH_DOT3: out[i] = dot(ld3(a, n, i), ld3(b, n, i)); break;
      case MTX_MATH_NORM3: out[i] = norm(ld3(a, n, i)); break;
      case MTX_MATH_NORMALIZE3: st3(out, n, i, normalize(ld3(a, n, i))); break;
      case MTX_MATH_TO_LOCAL: st3(out, n, i, to_local(frame_from_normal(ld3(a, n, i)), ld3(b, n, i))); break;
      case MTX_MATH_TO_WORLD: st3(out, n, i, to_world(frame_from_normal(ld3(a, n, i)), ld3(b, n, i))); break;
      case MTX_MATH_MIS_A: out[i] = mis_weight_a(a[i], b[i]); break;
      case MTX_MATH_MIS_B: out[i] = mis_weight_b(a[i], b[i]); break;
      default: break;
    }
  }
}

inline unsigned blk_grid(uint32_t n, int block) {
  // enough blocks to fill the chip several times over; the loops stride
  return std::max(1u, std::min<unsigned>((n + block - 1) / block, 256u * 32u));
}

}  // namespace

void launch_blk_seed(uint32_t n, uint32_t seed, const uint32_t *lanes, uint32_t skip, uint64_t *state,
                     hipStream_t st) {
  hipLaunchKernelGGL(k_blk_seed, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, n, seed, lanes, skip,
                     reinterpret_cast<ulonglong2 *>(state));
}
void launch_blk_next(uint32_t n, uint64_t *state, int dims, float *out, hipStream_t st) {
  ulonglong2 *w = reinterpret_cast<ulonglong2 *>(state);
  if (dims == 1)
    hipLaunchKernelGGL(k_blk_next<1>, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, n, w, out);
  else
    hipLaunchKernelGGL(k_blk_next<2>, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, n, w, out);
}
void launch_blk_interact(const DevScene &s, uint32_t n, int trace, const float *o, const float *d, const float *maxt,
                         const float *t, const uint32_t *prim, const float *u, const float *v, const uint8_t *active,
                         const mtx_si_planes &si, uint32_t *bad, hipStream_t st) {
  const dim3 grid(blk_grid(n, kTraceBlock)), block(kTraceBlock);
  if (trace)
    hipLaunchKernelGGL(k_blk_interact<true>, grid, block, stack_bytes(s), st, s, n, o, d, maxt, t, prim, u, v, active,
                       si, bad);
  else
    hipLaunchKernelGGL(k_blk_interact<false>, grid, block, 0, st, s, n, o, d, maxt, t, prim, u, v, active, si, bad);
}
void launch_blk_ray_test(const DevScene &s, uint32_t n, const float *o, const float *d, const float *maxt,
                         const uint8_t *active, uint8_t *out, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_ray_test, dim3(blk_grid(n, kTraceBlock)), dim3(kTraceBlock), stack_bytes(s), st, s, n, o,
                     d, maxt, active, out);
}
void launch_blk_spawn(uint32_t n, const float *p, const float *nrm, const float *x, int to, float *o, float *d,
                      float *maxt, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_spawn, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, n, p, nrm, x, to, o, d, maxt);
}
void launch_blk_sample_emitter(const DevScene &s, uint32_t n, const float *p, const float *nrm, const float *u,
                               const uint8_t *active, int test_visibility, const mtx_ds_planes &ds, float *weight,
                               hipStream_t st) {
  const dim3 grid(blk_grid(n, kTraceBlock)), block(kTraceBlock);
  if (test_visibility)
    hipLaunchKernelGGL(k_blk_sample_emitter<true>, grid, block, stack_bytes(s), st, s, n, p, nrm, u, active, ds,
                       weight);
  else
    hipLaunchKernelGGL(k_blk_sample_emitter<false>, grid, block, 0, st, s, n, p, nrm, u, active, ds, weight);
}
void launch_blk_emitter(const DevScene &s, uint32_t n, const int32_t *emitter, const float *d, const float *dist,
                        const float *nrm, const float *wi, const uint8_t *active, float *pdf, float *le,
                        uint32_t *bad, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_emitter, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, s, n, emitter, d, dist, nrm,
                     wi, active, pdf, le, bad);
}
void launch_blk_bsdf(const DevScene &s, uint32_t n_materials, uint32_t n, const int32_t *material, const float *uv,
                     const float *wi, const float *wo, const float *u1, const float *u2, const uint8_t *active,
                     const mtx_bsdf_planes &out, uint32_t *flags, uint32_t *bad, hipStream_t st) {
  const dim3 grid(blk_grid(n, kBlkBlock)), block(kBlkBlock);
  if (out.value)
    hipLaunchKernelGGL(k_blk_bsdf<true>, grid, block, 0, st, s, n_materials, n, material, uv, wi, wo, u1, u2, active,
                       out, flags, bad);
  else
    hipLaunchKernelGGL(k_blk_bsdf<false>, grid, block, 0, st, s, n_materials, n, material, uv, wi, wo, u1, u2, active,
                       out, flags, bad);
}
void launch_blk_math(int op, uint32_t n, const float *a, const float *b, const float *c, float *out, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_math, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, op, n, a, b, c, out);
}

}  // namespace mtxd
