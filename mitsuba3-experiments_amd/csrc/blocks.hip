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
#include "film_dev.h"
#include "mtx_core/bdpt.h"

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

// sensor.sample_ray (path.py:45-62): camera_path's two lines (camera_dev.h)
// on a film position the caller holds.
__global__ __launch_bounds__(kBlkBlock) void k_blk_sensor_ray(mtx_camera cam, uint32_t n, const float *pos,
                                                              const uint8_t *active, float *o, float *d,
                                                              float *maxt) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    Ray r;
    r.o = r.d = v3s(0.f);
    r.maxt = 0.f;
    if (lane_on(active, i)) {
      const V2 ps = ld2(pos, n, i);
      r = camera_ray(cam, V2{ps.x / (float)cam.width, ps.y / (float)cam.height});
    }
    st3(o, n, i, r.o);
    st3(d, n, i, r.d);
    if (maxt) maxt[i] = r.maxt;
  }
}

// scene.sample_emitter_ray (bdpt02.py:86-88): the start of a light path.
__global__ __launch_bounds__(kBlkBlock) void k_blk_sample_emitter_ray(DevScene s, uint32_t n, const float *u_pos,
                                                                      const float *u_dir, const uint8_t *active,
                                                                      EmitterRayPlanes out) {
  const SceneView view = make_view(s);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    EmitterRaySample es;
    if (lane_on(active, i)) {
      sample_emitter_ray(view, ld2(u_pos, n, i), ld2(u_dir, n, i), &es);
    } else {
      es.ray = Ray{v3s(0.f), v3s(0.f), 0.f};
      es.weight = es.p = es.n = v3s(0.f);
      es.emitter = -1;
    }
    st3(out.o, n, i, es.ray.o);
    st3(out.d, n, i, es.ray.d);
    out.maxt[i] = es.ray.maxt;
    st3(out.weight, n, i, es.weight);
    st3(out.p, n, i, es.p);
    st3(out.n, n, i, es.n);
    out.emitter[i] = es.emitter;
  }
}

// sensor.sample_direction: camera_sample_direction of the bound camera, and
// with VIS the connection ray spawn_ray_to(p, nrm, origin) through the
// any-hit tree in the same lane (k_blk_sample_emitter<true>'s shape).
template <bool VIS>
__global__ __launch_bounds__(kTraceBlock) void k_blk_sensor_direction(DevScene s, uint32_t n, const float *p,
                                                                      const float *nrm, const uint8_t *active,
                                                                      SensorDirPlanes out) {
  extern __shared__ int4 blk_lds[];
  const mtx_camera cam = s.camera;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    SensorDirectionSample sd;
    sd.pos = V2{0.f, 0.f};
    sd.d = v3s(0.f);
    sd.dist = sd.weight = 0.f;
    sd.valid = false;
    if (lane_on(active, i)) {
      const V3 ref = ld3(p, n, i);
      camera_sample_direction(cam, ref, &sd);
      if (VIS && sd.valid) {
        const Ray sr = spawn_ray_to(ref, ld3(nrm, n, i), V3{cam.origin[0], cam.origin[1], cam.origin[2]});
        const TraceRay r = make_trace_ray(sr.o, sr.d, sr.maxt);
        uint32_t nv = 0, tv = 0;
        if (traverse_occ(s, reinterpret_cast<uint32_t *>(blk_lds) + threadIdx.x, r, sr.maxt, nv, tv)) sd.weight = 0.f;
      }
    }
    st2(out.pos, n, i, sd.pos);
    st3(out.d, n, i, sd.d);
    out.dist[i] = sd.dist;
    out.weight[i] = sd.weight;
    out.valid[i] = sd.valid ? 1 : 0;
  }
}

// Connects the camera and light subpaths of a lane (mtx_core/bdpt.h): every
// strategy, or one, with its weight walk reading the stores' planes; VIS: a
// connection's shadow ray through the any-hit tree on this thread's stack
// column, only where the unoccluded contribution is non-zero.
struct BdptNoShadow {
  __device__ __forceinline__ bool operator()(const Ray &) const { return false; }
};
struct BdptShadow {
  const DevScene &s;
  uint32_t *stk;
  __device__ __forceinline__ bool operator()(const Ray &sr) const {
    const TraceRay r = make_trace_ray(sr.o, sr.d, sr.maxt);
    uint32_t nv = 0, tv = 0;
    return traverse_occ(s, stk, r, sr.maxt, nv, tv);
  }
};

template <bool VIS>
__global__ __launch_bounds__(kTraceBlock) void k_blk_bdpt_connect(DevScene s, uint32_t n_materials, uint32_t n,
                                                                  mtx_path_planes cam, mtx_path_planes lit, int ss,
                                                                  int tt, uint32_t max_depth, int mis,
                                                                  const uint8_t *active, float *L, float *weight,
                                                                  uint32_t *bad) {
  extern __shared__ int4 blk_lds[];
  const SceneView view = make_view(s);  // the counts, before any load that depends on a caller's index
  const uint32_t n_emitters = view.n_emitters;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    V3 l = v3s(0.f);
    float w = 0.f;
    if (lane_on(active, i)) {
      const PathLane zc = path_lane(&cam, n, i), yl = path_lane(&lit, n, i);
      if (path_has_bad_index(zc, n_materials, n_emitters) || path_has_bad_index(yl, n_materials, n_emitters))
        atomicAdd(bad, 1u);
      if (VIS)
        l = bdpt_connect(view, n_materials, zc, yl, ss, tt, max_depth, mis != 0,
                         BdptShadow{s, reinterpret_cast<uint32_t *>(blk_lds) + threadIdx.x}, &w);
      else
        l = bdpt_connect(view, n_materials, zc, yl, ss, tt, max_depth, mis != 0, BdptNoShadow{}, &w);
    }
    st3(L, n, i, l);
    if (weight) weight[i] = w;
  }
}

// ------------------------------------------------------------------ film --
// Stage 1 of the film (DESIGN.md "Film") on samples the caller holds. The
// contribution planes are the fused film's, [slot][K][band_px] float4; a put
// loads a source pixel's accumulators from them, adds its samples in rank
// order with film_accumulate (film_dev.h) and stores them back.

// Walks the slots of one source pixel's samples in ascending sample index g:
// the accumulators of a slot are loaded when its first sample arrives and
// stored when a later slot's arrives (or at the end); slots without a sample
// of this put are neither read nor written.
template <int K>
struct PutSlots {
  float4 *planes;
  size_t band_px, o;
  uint32_t T, cur, end;
  bool held;
  __device__ __forceinline__ void init(float4 *planes_, uint32_t band_px_, uint32_t o_, uint32_t T_) {
    planes = planes_;
    band_px = band_px_;
    o = o_;
    T = T_;
    cur = 0;
    end = film_slot_end(0, T);
    held = false;
  }
  __device__ __forceinline__ void store(const float4 *acc) {
#pragma unroll
    for (int k = 0; k < K; ++k) planes[((size_t)cur * K + k) * band_px + o] = acc[k];
  }
  __device__ __forceinline__ void enter(uint32_t g, float4 *acc) {
    if (g >= end) {
      if (held) store(acc);
      held = false;
      while (g >= end) {  // film_slot(g, T), continued from the previous sample's slot
        ++cur;
        end = cur < 7 ? film_slot_end(cur, T) : 0xffffffffu;
      }
    }
    if (!held) {
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = planes[((size_t)cur * K + k) * band_px + o];
      held = true;
    }
  }
  __device__ __forceinline__ void finish(const float4 *acc) {
    if (held) store(acc);
  }
};

__device__ __forceinline__ bool finite2(V2 p) { return fabsf(p.x) < kInf && fabsf(p.y) < kInf; }

// General path, pass 1: the source-pixel key of every lane for the stable
// group-by, (y - y0) * W + x of floor(pos); an inactive lane and a dropped
// one (non-finite position, or a source pixel outside the band: counted) get
// the trash key band_px.
__global__ __launch_bounds__(kBlkBlock) void k_blk_film_keys(FilmBand g, uint32_t n, const float *pos,
                                                             const uint8_t *active, uint32_t *keys,
                                                             uint32_t *counts) {
  uint32_t dropped = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint32_t key = g.band_px;
    if (lane_on(active, i)) {
      const V2 ps = ld2(pos, n, i);
      const float fx = floorf(ps.x), fy = floorf(ps.y);
      if (finite2(ps) && fx >= 0.f && fx < (float)g.width && fy >= (float)g.y0 && fy < (float)g.y1)
        key = ((uint32_t)fy - g.y0) * g.width + (uint32_t)fx;
      else
        ++dropped;
    }
    keys[i] = key;
  }
  if (dropped) atomicAdd(counts + kPutDropped, dropped);
}

// General path, pass 2: one lane per source pixel walks the pixel's lanes in
// the group-by's order (ascending lane index).
template <int N, uint32_t F>
__global__ __launch_bounds__(film_max_block(N)) void k_blk_film_put(FilmBand g, uint32_t n, const float *pos,
                                                                    const float *L, const uint32_t *key_size,
                                                                    const uint32_t *key_offset, const uint32_t *order,
                                                                    uint32_t spp_total, uint32_t sample_offset,
                                                                    float4 *planes) {
  constexpr int K = film_taps(N);
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= g.band_px) return;
  const uint32_t cnt = key_size[q];
  if (cnt == 0) return;
  const uint32_t off = key_offset[q];
  const uint32_t row = q / g.width;
  const int y = (int)(g.y0 + row), x = (int)(q - row * g.width);
  PutSlots<K> slots;
  slots.init(planes, g.band_px, q, spp_total ? spp_total : cnt);
  float4 acc[K];
  for (uint32_t r = 0; r < cnt; ++r) {
    const uint32_t i = order[off + r];
    slots.enter(sample_offset + r, acc);
    const V2 ps = ld2(pos, n, i);
    film_accumulate<N, F>(acc, x, y, make_float2(ps.x, ps.y), ld3(L, n, i));
  }
  slots.finish(acc);
}

// Pixel-major path, pass 1: lane i claims pixel px0 + i / s. An active lane
// with a finite position keeps the claim when floor(pos) is that pixel, or
// pos lies exactly on the pixel's upper edge: (float)x + u rounds up to x + 1
// for u close to 1, and the fixed integrators keep such a sample in the
// pixel that drew it (mtx_core/film.h, the box filter's closed interval).
// counts: violations, dropped (non-finite), lanes that are not kept.
__global__ __launch_bounds__(kBlkBlock) void k_blk_film_claim(FilmBand g, uint32_t n, const float *pos,
                                                              const uint8_t *active, uint32_t s, uint32_t px0,
                                                              uint32_t *counts) {
  uint32_t bad = 0, dropped = 0, off = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (!lane_on(active, i)) {
      ++off;
      continue;
    }
    const V2 ps = ld2(pos, n, i);
    if (!finite2(ps)) {
      ++dropped;
      ++off;
      continue;
    }
    const uint32_t pix = px0 + i / s, y = pix / g.width, x = pix - y * g.width;
    const float fx = (float)x, fy = (float)y;
    const bool in_x = floorf(ps.x) == fx || ps.x == fx + 1.f, in_y = floorf(ps.y) == fy || ps.y == fy + 1.f;
    if (!in_x || !in_y) ++bad;
  }
  if (bad) atomicAdd(counts + kPutViolations, bad);
  if (dropped) atomicAdd(counts + kPutDropped, dropped);
  if (off) atomicAdd(counts + kPutOff, off);
}

// Pixel-major path, pass 2 (after a clean pass 1): a wave stages 64 pixels x
// S samples of the five planes through LDS, so every global read is a run of
// whole lines (the planes are (C, n): the 64 x s floats of the wave's pixels
// are contiguous in each); then each lane accumulates its own pixel in
// sample order. S = min(s, kPutStage); rows of S | 1 words keep the
// per-lane column reads on distinct banks. A lane that is off or dropped is
// staged as a NaN in the x plane and skipped. `ragged`: some lane of the put
// is not kept, so without spp_total a pixel's T is its own kept count,
// taken in a first sweep over the position planes.
constexpr int kPutStage = 16;

template <int N, uint32_t F>
__global__ __launch_bounds__(64) void k_blk_film_put_staged(FilmBand g, uint32_t n, const float *pos, const float *L,
                                                            const uint8_t *active, uint32_t s, uint32_t px0,
                                                            uint32_t n_px, uint32_t spp_total, uint32_t sample_offset,
                                                            int ragged, float4 *planes) {
  constexpr int K = film_taps(N);
  extern __shared__ float put_lds[];  // 5 planes (pos.xy, L.xyz) of 64 rows, sized by the launch
  const uint32_t S = min(s, (uint32_t)kPutStage), rowlen = S | 1u, plane = 64 * rowlen;
  float *const sv0 = put_lds, *const sv1 = sv0 + plane, *const sv2 = sv1 + plane, *const sv3 = sv2 + plane,
               *const sv4 = sv3 + plane;
  const uint32_t q0 = blockIdx.x * 64, lane = threadIdx.x, q = q0 + lane;
  const uint32_t n_here = min(64u, n_px - q0);
  const bool live = q < n_px;
  const uint32_t pix = px0 + q, yy = pix / g.width;
  const int y = (int)yy, x = (int)(pix - yy * g.width);
  const float nan = __int_as_float(0x7fc00000);
  uint32_t T = spp_total ? spp_total : s;
  if (ragged && !spp_total) {
    T = 0;
    for (uint32_t s0 = 0; s0 < s; s0 += S) {
      const uint32_t ns = min(S, s - s0);
      for (uint32_t e = lane; e < n_here * ns; e += 64) {
        const uint32_t j = e / ns, sm = e - j * ns;
        const uint32_t i = (q0 + j) * s + s0 + sm;
        sv0[j * rowlen + sm] = lane_on(active, i) && finite2(ld2(pos, n, i)) ? 0.f : nan;
      }
      __syncthreads();
      if (live)
        for (uint32_t sm = 0; sm < ns; ++sm) T += sv0[lane * rowlen + sm] == 0.f ? 1u : 0u;
      __syncthreads();
    }
  }
  PutSlots<K> slots;
  slots.init(planes, g.band_px, live ? pix - g.y0 * g.width : 0u, T);
  float4 acc[K];
  uint32_t rank = 0;
  for (uint32_t s0 = 0; s0 < s; s0 += S) {
    const uint32_t ns = min(S, s - s0);
    for (uint32_t e = lane; e < n_here * ns; e += 64) {
      const uint32_t j = e / ns, sm = e - j * ns;
      const uint32_t i = (q0 + j) * s + s0 + sm, a = j * rowlen + sm;
      const V2 ps = ld2(pos, n, i);
      const V3 l = ld3(L, n, i);
      sv0[a] = lane_on(active, i) && finite2(ps) ? ps.x : nan;
      sv1[a] = ps.y;
      sv2[a] = l.x;
      sv3[a] = l.y;
      sv4[a] = l.z;
    }
    __syncthreads();
    if (live)
      for (uint32_t sm = 0; sm < ns; ++sm) {
        const uint32_t a = lane * rowlen + sm;
        const float sx = sv0[a];
        if (sx != sx) continue;
        slots.enter(sample_offset + rank, acc);
        ++rank;
        film_accumulate<N, F>(acc, x, y, make_float2(sx, sv1[a]), V3{sv2[a], sv3[a], sv4[a]});
      }
    __syncthreads();
  }
  if (live) slots.finish(acc);
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
void launch_blk_sensor_ray(const mtx_camera &cam, uint32_t n, const float *pos, const uint8_t *active, float *o,
                           float *d, float *maxt, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_sensor_ray, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, cam, n, pos, active, o, d,
                     maxt);
}
void launch_blk_sample_emitter_ray(const DevScene &s, uint32_t n, const float *u_pos, const float *u_dir,
                                   const uint8_t *active, const EmitterRayPlanes &out, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_sample_emitter_ray, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, s, n, u_pos,
                     u_dir, active, out);
}
void launch_blk_sensor_direction(const DevScene &s, uint32_t n, const float *p, const float *nrm,
                                 const uint8_t *active, int test_visibility, const SensorDirPlanes &out,
                                 hipStream_t st) {
  const dim3 grid(blk_grid(n, kTraceBlock)), block(kTraceBlock);
  if (test_visibility)
    hipLaunchKernelGGL(k_blk_sensor_direction<true>, grid, block, stack_bytes(s), st, s, n, p, nrm, active, out);
  else
    hipLaunchKernelGGL(k_blk_sensor_direction<false>, grid, block, 0, st, s, n, p, nrm, active, out);
}
void launch_blk_bdpt_connect(const DevScene &s, uint32_t n_materials, uint32_t n, const mtx_path_planes &camera,
                             const mtx_path_planes &light, int ss, int tt, uint32_t max_depth, uint32_t flags,
                             const uint8_t *active, float *L, float *weight, uint32_t *bad, hipStream_t st) {
  const dim3 grid(blk_grid(n, kTraceBlock)), block(kTraceBlock);
  const int mis = (flags & MTX_BDPT_MIS) != 0;
  if (flags & MTX_BDPT_VISIBILITY)
    hipLaunchKernelGGL(k_blk_bdpt_connect<true>, grid, block, stack_bytes(s), st, s, n_materials, n, camera, light, ss,
                       tt, max_depth, mis, active, L, weight, bad);
  else
    hipLaunchKernelGGL(k_blk_bdpt_connect<false>, grid, block, 0, st, s, n_materials, n, camera, light, ss, tt,
                       max_depth, mis, active, L, weight, bad);
}
void launch_blk_film_keys(const FilmBand &g, uint32_t n, const float *pos, const uint8_t *active, uint32_t *keys,
                          uint32_t *counts, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_film_keys, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, g, n, pos, active, keys,
                     counts);
}
void launch_blk_film_claim(const FilmBand &g, uint32_t n, const float *pos, const uint8_t *active, uint32_t s,
                           uint32_t px0, uint32_t *counts, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_film_claim, dim3(blk_grid(n, kBlkBlock)), dim3(kBlkBlock), 0, st, g, n, pos, active, s, px0,
                     counts);
}
void launch_blk_film_put(const FilmBand &g, uint32_t n, const float *pos, const float *L, const uint32_t *key_size,
                         const uint32_t *key_offset, const uint32_t *order, uint32_t spp_total,
                         uint32_t sample_offset, float4 *planes, hipStream_t st) {
  with_rfilter(g.rfilter, [&](auto N, auto F) {
    hipLaunchKernelGGL((k_blk_film_put<decltype(N)::value, decltype(F)::value>), dim3((g.band_px + 127) / 128),
                       dim3(128), 0, st, g, n, pos, L, key_size, key_offset, order, spp_total, sample_offset, planes);
  });
}
void launch_blk_film_put_staged(const FilmBand &g, uint32_t n, const float *pos, const float *L,
                                const uint8_t *active, uint32_t s, uint32_t px0, uint32_t spp_total,
                                uint32_t sample_offset, int ragged, float4 *planes, hipStream_t st) {
  const uint32_t n_px = n / s;
  // 5 planes x 64 rows of min(s, kPutStage) | 1 words: 3.8 KB at s = 3, 11.5 KB at 8 or 9, 21.8 KB from 16 on
  const size_t lds = 5 * 64 * (size_t)(std::min<uint32_t>(s, kPutStage) | 1u) * sizeof(float);
  with_rfilter(g.rfilter, [&](auto N, auto F) {
    hipLaunchKernelGGL((k_blk_film_put_staged<decltype(N)::value, decltype(F)::value>), dim3((n_px + 63) / 64),
                       dim3(64), lds, st, g, n, pos, L, active, s, px0, n_px, spp_total, sample_offset, ragged, planes);
  });
}

}  // namespace mtxd
