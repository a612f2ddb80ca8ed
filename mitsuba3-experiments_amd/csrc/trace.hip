// trace.hip — the persistent traversal kernels of the fixed integrators:
// closest hit of a bounce's queue (k_trace_closest: idle lanes take prepared
// rays from the wave's LDS ring; k_trace_closest_refill: the threshold
// refill), any hit of the NEE shadow records (k_trace_shadow), bounce-0
// closest hit with derived camera rays (k_trace_camera), and mtx_trace's raw
// rays (k_trace_raw). The traversal loops themselves are device_common.h's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "camera_dev.h"
#include "device_common.h"
#include "shadow_dev.h"

namespace mtxd {

// Closest-hit queries of bounce `bounce`: queue entries are path indices.
// The hit record goes to the queue position k (not the path): the shade
// kernel, which walks the same queue, then reads it coalesced and without
// waiting for its queue entry.
struct ClosestSrc {
  using Payload = uint32_t;  // the queue position
  WaveBuffers b;
  const uint32_t *queue;
  const float4 *ro, *rd;  // this bounce's ray planes, by queue position
  __device__ __forceinline__ void load(uint32_t k, TraceRay &r, float &tmax, uint32_t &payload) const {
    const float4 o4 = ld_stream<kNtTrace>(ro + k), d4 = ld_stream<kNtTrace>(rd + k);
    r = make_trace_ray(V3{o4.x, o4.y, o4.z}, V3{d4.x, d4.y, d4.z}, o4.w);
    tmax = o4.w;
    payload = k;
  }
  __device__ __forceinline__ void finish(uint32_t slot, bool, float t, uint32_t prim, float u, float v) const {
    st_stream<kNtTraceSt>(b.hit + slot, make_float4(prim == 0xffffffffu ? kInf : t, __uint_as_float(prim), u, v));
  }
};

// 8 waves/SIMD for the trace kernels (their grid is sized for 8): left alone
// the compiler took 66 VGPRs for the any-hit kernel (7 waves); asked for 8 it
// fits without spills. Shadow 56.4 -> 55.6 ms per step (A/B, one box, 3
// rounds, round 2).
#define MTX_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(8)))
#ifndef MTX_CLOSEST_WAVES
#define MTX_CLOSEST_WAVES 8  // closest hit: waves/SIMD the register budget is sized for
#endif
// RING: idle lanes take prepared rays from the wave's LDS ring (device_common.h
// RayRing), else the threshold refill.
template <bool STATS, bool RING>
__device__ __forceinline__ void trace_closest_body(const DevScene &s, const WaveBuffers &b, uint32_t bounce) {
  // dynamic LDS: stack columns + tree top + rings (device_common.h trace_loop)
  const uint32_t rp = (bounce + b.ray_par) & 1u;
  const ClosestSrc src{b, b.queue[bounce & 1], b.ray_o[rp], b.ray_d[rp]};
  uint32_t nv = 0, tv = 0, nr = 0, wi[2] = {0, 0};
  trace_loop<false, STATS, RING>(s, src, b.counters[4 * bounce + 0], b.xheads + (2 * bounce) * kXSlotWords, nv, tv, nr,
                           wi);
  if (STATS) {
    unsigned long long a = wave_sum_u64(nv), c = wave_sum_u64(tv), n = wave_sum_u64(nr);
    unsigned long long w0 = wave_sum_u64(wi[0]), w1 = wave_sum_u64(wi[1]);
    if ((threadIdx.x & 63) == 0 && n) {
      atomicAdd(&b.stats[0], a);
      atomicAdd(&b.stats[1], c);
      atomicAdd(&b.stats[4], n);
      atomicAdd(&b.stats[6], w0);
      atomicAdd(&b.stats[7], w1);
    }
  }
}
// The closest-hit kernel: prepared-ray rings (DevScene::trace_ring rays per wave).
template <bool STATS>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MTX_CLOSEST_WAVES))) void k_trace_closest(DevScene s, WaveBuffers b, uint32_t bounce) {
  trace_closest_body<STATS, true>(s, b, bounce);
}
// MTX_TRACE_RING=0: the same loop with the threshold refill (DevScene::urefill),
// the reference the ring is measured and tested against.
template <bool STATS>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MTX_CLOSEST_WAVES))) void k_trace_closest_refill(DevScene s, WaveBuffers b, uint32_t bounce) {
  trace_closest_body<STATS, false>(s, b, bounce);
}

// Any-hit traversal of the NEE shadow rays; a record's forms: shadow_dev.h.
struct ShadowSrc {
  struct Payload {
    uint32_t k, li;  // record, L index of the target (plane * capacity + position)
    float4 t;        // L after an unoccluded ray | flags
  };
  WaveBuffers b;
  __device__ __forceinline__ void load(uint32_t k, TraceRay &r, float &tmax, Payload &pl) const {
    const float4 o4 = ld_stream<kNtTrace>(shadow_word(b, 0, k)), d4 = ld_stream<kNtTrace>(shadow_word(b, 1, k));
    r = make_trace_ray(V3{o4.x, o4.y, o4.z}, V3{d4.x, d4.y, d4.z}, o4.w);
    tmax = o4.w;
    pl.k = k;
    pl.li = __float_as_uint(d4.w);
    pl.t = ld_stream<kNtTrace>(shadow_word(b, 2, k));
  }
  __device__ __forceinline__ void finish(const Payload &pl, bool occluded, float, uint32_t, float, float) const {
    const uint32_t fl = __float_as_uint(pl.t.w);
    if (!(fl & kShadowFinal)) {
      // make_shadow's form (the nerad integrators keep L by path outside
      // k_shade's stores): read-modify-write of L
      if (occluded && (fl & 14u) == 0u) return;
      float4 L = b.L[0][pl.li];
      apply_shadow(L, pl.t, *shadow_word(b, 3, pl.k), occluded);
      b.L[0][pl.li] = L;
      return;
    }
    if (!occluded) {
      typedef float v3f __attribute__((ext_vector_type(3)));
      *reinterpret_cast<v3f *>(b.L[0] + pl.li) = v3f{pl.t.x, pl.t.y, pl.t.z};
    } else if (fl & 14u) {
      float4 L = b.L[0][pl.li];
      const float qnan = __uint_as_float(0x7fc00000u);
      if (fl & 2u) L.x = qnan;
      if (fl & 4u) L.y = qnan;
      if (fl & 8u) L.z = qnan;
      b.L[0][pl.li] = L;
    }
    // occluded without flags: L unchanged, nothing to store
  }
};

template <bool STATS>
__global__ __launch_bounds__(kTraceBlock) MTX_TRACE_ATTR void k_trace_shadow(DevScene s, WaveBuffers b, uint32_t bounce) {
  // dynamic LDS: stack columns + tree top (device_common.h trace_loop)
  const ShadowSrc src{b};
  uint32_t nv = 0, tv = 0, nr = 0;
  trace_loop<true>(s, src, b.counters[4 * (bounce + 1) + 1], b.xheads + (2 * bounce + 1) * kXSlotWords, nv, tv, nr);
  if (STATS) {
    unsigned long long a = wave_sum_u64(nv), c = wave_sum_u64(tv), n = wave_sum_u64(nr);
    if ((threadIdx.x & 63) == 0 && n) {
      atomicAdd(&b.stats[2], a);
      atomicAdd(&b.stats[3], c);
      atomicAdd(&b.stats[5], n);
    }
  }
}

// Bounce-0 closest hit of a camera chunk without stored rays (ChunkParams::
// cam0): the ray of queue position k (= path k, the identity queue) is derived
// where the traversal takes it; the hit record goes where ClosestSrc puts it.
struct CameraSrc {
  using Payload = uint32_t;  // the queue position
  const DevScene &s;
  const WaveBuffers &b;
  const ChunkParams &p;
  __device__ __forceinline__ void load(uint32_t k, TraceRay &r, float &tmax, uint32_t &payload) const {
    const CamPath cp = camera_path(s.camera, s.has_env != 0, p, k);
    r = make_trace_ray(cp.ray.o, cp.ray.d, cp.ray.maxt);
    tmax = cp.ray.maxt;
    payload = k;
  }
  __device__ __forceinline__ void finish(uint32_t slot, bool, float t, uint32_t prim, float u, float v) const {
    st_stream<kNtTraceSt>(b.hit + slot, make_float4(prim == 0xffffffffu ? kInf : t, __uint_as_float(prim), u, v));
  }
};

// Its own kernel: k_trace_closest keeps its code and registers. Launched with
// the refill threshold DevScene::cam_urefill (launch_trace_camera): load() is
// ~300 VALU instructions, run for the refilling lanes only.
template <bool STATS>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MTX_CLOSEST_WAVES))) void k_trace_camera(DevScene s, WaveBuffers b, ChunkParams p) {
  // dynamic LDS: stack columns + tree top (device_common.h trace_loop)
  const CameraSrc src{s, b, p};
  uint32_t nv = 0, tv = 0, nr = 0, wi[2] = {0, 0};
  trace_loop<false, STATS>(s, src, p.n_paths, b.xheads, nv, tv, nr, wi);
  if (STATS) {
    unsigned long long a = wave_sum_u64(nv), c = wave_sum_u64(tv), n = wave_sum_u64(nr);
    unsigned long long w0 = wave_sum_u64(wi[0]), w1 = wave_sum_u64(wi[1]);
    if ((threadIdx.x & 63) == 0 && n) {
      atomicAdd(&b.stats[0], a);
      atomicAdd(&b.stats[1], c);
      atomicAdd(&b.stats[4], n);
      atomicAdd(&b.stats[6], w0);
      atomicAdd(&b.stats[7], w1);
    }
  }
}

// Raw traversal for mtx_trace: rays as (o.xyz, maxt), (d.xyz, 0). mode 0
// closest hit (4-wide tree), 1 any hit (8-wide occlusion tree).
__device__ __forceinline__ void trace_raw_one(const DevScene &s, const float4 *rays, uint32_t i, int any_hit,
                                              uint32_t *hits, uint32_t *visits, int4 *raw_lds) {
  const float4 o4 = rays[2 * (size_t)i], d4 = rays[2 * (size_t)i + 1];
  TraceRay r = make_trace_ray(V3{o4.x, o4.y, o4.z}, V3{d4.x, d4.y, d4.z}, o4.w);
  float tbest = o4.w, bu = 0.f, bv = 0.f;
  uint32_t prim = 0xffffffffu, nv = 0, tv = 0;
  if (any_hit == 1) {
    hits[i] = traverse_occ(s, reinterpret_cast<uint32_t *>(raw_lds) + threadIdx.x, r, o4.w, nv, tv) ? 1u : 0u;
  } else {
    traverse_closest(s, reinterpret_cast<int32_t *>(raw_lds) + threadIdx.x, r, tbest, prim, bu, bv, nv, tv);
    if (prim == 0xffffffffu) tbest = kInf;
    hits[4 * (size_t)i + 0] = __float_as_uint(tbest);
    hits[4 * (size_t)i + 1] = prim;
    hits[4 * (size_t)i + 2] = __float_as_uint(bu);
    hits[4 * (size_t)i + 3] = __float_as_uint(bv);
  }
  if (visits) {
    visits[2 * (size_t)i] = nv;
    visits[2 * (size_t)i + 1] = tv;
  }
}

__global__ __launch_bounds__(kTraceBlock) void k_trace_raw(DevScene s, const float4 *rays, uint32_t n, int any_hit,
                                                           uint32_t *hits, uint32_t *visits) {
  extern __shared__ int4 raw_lds[];  // one stack column per thread (device_common.h stack_bytes)
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    trace_raw_one(s, rays, i, any_hit, hits, visits, raw_lds);
}

// f(std::true_type or std::false_type): a trace kernel's STATS argument for the runtime flag.
template <class Fn>
static void with_stats(uint32_t stats, Fn &&f) {
  if (stats)
    f(std::true_type{});
  else
    f(std::false_type{});
}
void launch_trace_closest(const DevScene &scene, const WaveBuffers &b, uint32_t bounce, uint32_t stats, int grid,
                          hipStream_t st) {
  if (scene.trace_ring) {
    const DevScene s = ring_view(scene);
    const size_t lds = ring_stack_bytes(scene);
    with_stats(stats, [&](auto S) {
      hipLaunchKernelGGL(k_trace_closest<decltype(S)::value>, dim3(grid), dim3(kTraceBlock), lds, st, s, b, bounce);
    });
    return;
  }
  const size_t lds = persistent_stack_bytes(scene, false);
  with_stats(stats, [&](auto S) {
    hipLaunchKernelGGL(k_trace_closest_refill<decltype(S)::value>, dim3(grid), dim3(kTraceBlock), lds, st, scene, b,
                       bounce);
  });
}
void launch_trace_camera(const DevScene &scene, const WaveBuffers &b, const ChunkParams &p, int grid, hipStream_t st) {
  DevScene s = scene;
  s.urefill = scene.cam_urefill;  // the traversal's refill threshold, for this kernel
  const size_t lds = persistent_stack_bytes(s, false);
  with_stats(p.stats, [&](auto S) {
    hipLaunchKernelGGL(k_trace_camera<decltype(S)::value>, dim3(grid), dim3(kTraceBlock), lds, st, s, b, p);
  });
}
void launch_trace_shadow(const DevScene &s, const WaveBuffers &b, uint32_t bounce, uint32_t stats, int grid,
                         hipStream_t st) {
  with_stats(stats, [&](auto S) {
    hipLaunchKernelGGL(k_trace_shadow<decltype(S)::value>, dim3(grid), dim3(kTraceBlock),
                       persistent_stack_bytes(s, true), st, s, b, bounce);
  });
}
// Resident blocks per CU of the persistent kernels (grid = n_cu x this):
// the any-hit kernels (shadow, ReSTIR visibility) and the closest-hit kernel.
int trace_blocks_per_cu(const DevScene &s) {
  int na = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&na, k_trace_shadow<false>, kTraceBlock,
                                                   persistent_stack_bytes(s, true)) != hipSuccess ||
      na <= 0)
    na = 4;
  return na;
}
int closest_blocks_per_cu(const DevScene &s) {
  int nc = 0;
  const hipError_t e =
      s.trace_ring ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nc, k_trace_closest<false>, kTraceBlock,
                                                                  ring_stack_bytes(s))
                   : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nc, k_trace_closest_refill<false>, kTraceBlock,
                                                                  persistent_stack_bytes(s, false));
  if (e != hipSuccess || nc <= 0)
    nc = 4;
  return nc;
}
void launch_trace_raw(const DevScene &s, const float4 *rays, uint32_t n, int any_hit, uint32_t *hits,
                      uint32_t *visits, hipStream_t st) {
  // at most the persistent grid's threads: mode 2 indexes the spill area by thread
  const unsigned grid = std::min<unsigned>(blocks_for(n, kTraceBlock), s.ovf_threads / kTraceBlock);
  hipLaunchKernelGGL(k_trace_raw, dim3(std::max(1u, grid)), dim3(kTraceBlock), stack_bytes(s), st, s, rays, n, any_hit,
                     hits, visits);
}

}  // namespace mtxd
