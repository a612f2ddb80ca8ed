// shade.hip — the wavefront shade step and the per-path kernels around it:
// raygen (stored camera or caller rays), the persistent shade loop (k_shade,
// k_shade_cam: one bounce of shade_dev.h's bodies, survivors and shadow
// records stream-compacted with one reservation per block step), the tail
// flush, the NRC cache apply and the PSSMLT chain kernels.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_common.h"
#include "shade_dev.h"

// Minimum resident shade blocks per CU (caps the shade kernels' VGPRs: 3
// blocks of 256 threads = 3 waves/SIMD at <= 168 VGPRs). 4 blocks (<= 128
// VGPRs) spill 26 VGPRs of k_shade<2>: shade 63.4 -> 74.6 ms per step, and
// 69.4 ms with the NEE record staged in LDS (13 spilled); the record in LDS
// at 3 blocks (149 VGPRs): 64.4 ms (profiles/r6e_ab_shade_vgpr_budget.jsonl).
// The same budget for every integrator (pssmltpath.py's shade at 2 blocks,
// without its spills, measured slower: DESIGN.md §7).
#ifndef MTX_SHADE_MIN_BLOCKS
#define MTX_SHADE_MIN_BLOCKS 3
#endif
constexpr int kShadeMinBlocks = MTX_SHADE_MIN_BLOCKS;

namespace mtxd {

__global__ void k_raygen_camera(DevScene s, WaveBuffers b, ChunkParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) b.counters[0] = p.n_paths;
  if (i >= p.n_paths) return;
  const CamPath cp = camera_path(s.camera, s.has_env != 0, p, i);
  init_path(b, p, i, cp.ray, cp.rng, cp.pos, s.has_env != 0);
}

__global__ void k_raygen_rays(DevScene s, WaveBuffers b, ChunkParams p, const float *rays, const uint32_t *lanes,
                              uint32_t rng_skip) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) b.counters[0] = p.n_paths;
  if (i >= p.n_paths) return;
  Pcg32 rng = sampler_lane(p.seed, lanes[i]);
  for (uint32_t k = 0; k < rng_skip; ++k) rng.next_u32();
  const float *r = rays + 6 * (size_t)i;
  Ray ray{V3{r[0], r[1], r[2]}, V3{r[3], r[4], r[5]}, kLargest};
  init_path(b, p, i, ray, rng, make_float2(0.f, 0.f), s.has_env != 0);
}

#if MTX_DIAG_STAMPS
__device__ unsigned long long g_shade_stamps[kStampSegs + 2];  // the stamp sums (shade_dev.h Stamps)
#endif

// Diagnostic build only (MTX_DIAG_CLASSES=1, tools/shade_class_mix.py): what
// the waves of the mixed loop hold. Per bounce: the wave-steps with 1, 2 and
// 3 shading classes among their entries, then the entries of each class.
#ifndef MTX_DIAG_CLASSES
#define MTX_DIAG_CLASSES 0
#endif
#if MTX_DIAG_CLASSES
constexpr uint32_t kMixBounces = 16, kMixWords = 2 * mtx::kShadeClasses;
__device__ unsigned long long g_class_mix[kMixBounces][kMixWords];
__device__ __forceinline__ void class_mix_count(const DevScene &s, uint32_t bounce, bool valid, const float4 h) {
  const uint32_t prim = __float_as_uint(h.y);
  uint32_t cw = 0;
  if (valid && prim != 0xffffffffu) cw = __float_as_uint(s.shade_rec[8 * (size_t)prim + 2].w);
  const uint32_t cls = mtx::shade_class_of_rec(cw);
  uint32_t held = 0, n[mtx::kShadeClasses];
  for (uint32_t k = 0; k < mtx::kShadeClasses; ++k) {
    n[k] = (uint32_t)__popcll(__ballot(valid && cls == k));
    held += n[k] ? 1u : 0u;
  }
  if ((threadIdx.x & 63u) == 0 && held && bounce < kMixBounces) {
    atomicAdd(&g_class_mix[bounce][held - 1], 1ull);
    for (uint32_t k = 0; k < mtx::kShadeClasses; ++k)
      atomicAdd(&g_class_mix[bounce][mtx::kShadeClasses + k], (unsigned long long)n[k]);
  }
}
#endif

// The persistent shade loop of a bounce: k_shade's body. CAM: bounce 0 of a
// cam0 chunk (k_shade_cam), bounce_ is 0.
//
// CLS (path-mis and path; the launch carries shade_class_lds_bytes() of
// dynamic LDS): the same bounce with class-uniform block steps. A block sorts
// its grid-stride queue windows into one LDS ring per shading class
// (mtx_core/shade_class.h) and shades 256 entries of one class at a time, so
// a wave's lanes run one case of the BSDF switch; no pass over HBM is added.
// Per iteration: while no ring holds a full step and the queue has windows
// left, the next window is ingested (a lane's rank in its ring: one ballot
// per class, mbcnt and the waves' counts through LDS, so a ring stays in
// queue order), which always fits: no ring holds 256, and a ring has room for
// 512. Then the oldest 256 entries of the fullest ring are shaded, lane t
// taking entry head + t; once the queue is exhausted the rings' remainders
// are shaded packed, mixed as without CLS. The step itself is the same; path
// state is read at the entry's own queue position, survivors get consecutive
// append slots. The class of a window's entries comes from flag word 11 of
// their shading records; that load also is the L2 warm-up of the record
// (io.warm without CLS). A window loads ahead of its ingest: queue entries
// and hit records behind the ingest before, the class words behind the shade
// step before (6 registers live across a step; loaded at the ingest instead
// the bench step takes 135.8 against 134.2 ms). The ingest is an inner loop
// on purpose: as a branch of one loop with the shade step, ShadeIO's
// conditionally written fields became loop-carried copies and k_shade<2>
// spilled 42 VGPRs at its 168-VGPR budget.
template <int INT, bool CAM, bool CLS = false>
__device__ __forceinline__ void shade_loop(const DevScene &s, const WaveBuffers &b, const ChunkParams &p,
                                           uint32_t bounce_) {
  static_assert(!CLS || (shade_has_classes(INT) && !CAM), "class queues: k_shade of path-mis and path");
  const uint32_t bounce = CAM ? 0u : bounce_;
  const SceneView sv = make_view(s);
  const uint32_t count = b.counters[4 * bounce + 0];
  const uint32_t *in_q = b.queue[bounce & 1];
  uint32_t *out_q = b.queue[(bounce + 1) & 1];
  // [4(bounce+1)] next queue count, [4(bounce+1)+1] this bounce's shadow
  // rays: one 64-bit pair, reserved by one atomic per block step
  uint32_t *out_cnt = &b.counters[4 * (bounce + 1) + 0];
  const uint32_t rp = (bounce + b.ray_par) & 1u;  // this bounce's ray planes; the next ray goes to rp ^ 1
  // the nerad integrators keep thr / prev / L / misc by path (plane 0 / kFinal)
  constexpr bool kNerad = INT == MTX_INT_NERAD_RHS || INT == MTX_INT_NERAD;
  const uint32_t stride = gridDim.x * kShadeBlock;
  uint32_t parity = 0;
  // software pipeline over the persistent loop: the next step's queue entry
  // loads during this step, its hit record before this step's appends. Hit
  // records are stored by queue position (ClosestSrc), so they load
  // coalesced and in parallel with the queue entry. (CLS: path / h are the
  // window to ingest next, at nbase.)
  uint32_t path = 0;
  float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
  // an identity bounce-0 queue is not stored: position i is path i
  const bool ident = bounce == 0 && p.ident0;
  if (blockIdx.x * kShadeBlock + threadIdx.x < count) {
    const uint32_t i0 = blockIdx.x * kShadeBlock + threadIdx.x;
    path = ident ? i0 : ld_stream<kNtQueue>(in_q + i0);
    h = ld_stream<kNtShade>(b.hit + i0);
  }
  // CLS: the rings, [class][kClassRing] hit records, then [class][kClassRing]
  // position | path; an ingest's entries per wave and class; the block-uniform
  // ring state (scalar registers); the class words of the window at nbase
  constexpr uint32_t kC = mtx::kShadeClasses, kW = kShadeBlock / 64, kMask = kClassRing - 1;
  static_assert((kClassRing & kMask) == 0 && kClassRing >= 2 * kShadeBlock, "a ring holds two block steps");
  static_assert(kClassEntryBytes == sizeof(float4) + sizeof(uint2), "ring entry: hit record | position, path");
  extern __shared__ float4 class_lds[];
  float4 *ring_h = class_lds;
  uint2 *ring_ip = reinterpret_cast<uint2 *>(class_lds + kC * kClassRing);
  __shared__ uint32_t class_wcnt[CLS ? kW : 1][kC];
  uint32_t head[kC] = {}, fill[kC] = {};
  uint32_t nbase = blockIdx.x * kShadeBlock, cw = 0;
  bool cw_due = CLS && nbase < count;  // the window's class words are not loaded yet
  auto load_class_word = [&]() {
    const uint32_t pn = __float_as_uint(h.y);
    cw = 0;  // a miss or a lane past the queue's end: no record, class 0
    if (nbase + threadIdx.x < count && pn != 0xffffffffu) cw = __float_as_uint(s.shade_rec[8 * (size_t)pn + 2].w);
    cw_due = false;
  };

  Stamps stp{};
  MTX_STAMP_BEGIN(stp);
  for (uint32_t base = blockIdx.x * kShadeBlock; CLS || base < count; base += CLS ? 0u : stride, parity ^= 1u) {
    uint32_t i = base + threadIdx.x, path_s = path, path_n = 0;
    float4 h_s = h, hn = make_float4(0.f, 0.f, 0.f, 0.f);
    bool valid = i < count;
    const float4 *wp = nullptr;
    if constexpr (!CLS) {
      const uint32_t inext = i + stride;
      if (inext < count) path_n = ident ? inext : ld_stream<kNtQueue>(in_q + inext);
      // the next step's hit record, and from it the address of the shading
      // record that step will read: shade_path touches one word of it (L2 warm-up)
      if (inext < count) hn = b.hit[inext];
      const uint32_t pn = __float_as_uint(hn.y);
      wp = (inext < count && pn != 0xffffffffu) ? s.shade_rec + 8 * (size_t)pn : nullptr;
    } else {
      const uint32_t wave = threadIdx.x >> 6;
      uint32_t c, most, held;  // the fullest ring, its entries, all rings' entries
      for (;;) {
        c = 0;
        most = held = fill[0];
#pragma unroll
        for (uint32_t k = 1; k < kC; ++k) {
          if (fill[k] > most) {
            most = fill[k];
            c = k;
          }
          held += fill[k];
        }
        if (most >= (uint32_t)kShadeBlock || nbase >= count) break;
        // ---- ingest the window at nbase
        if (cw_due) load_class_word();
        const uint32_t i_n = nbase + threadIdx.x;
        const bool in = i_n < count;
        const uint32_t cls = mtx::shade_class_of_rec(cw);
        uint64_t m[kC];
#pragma unroll
        for (uint32_t k = 0; k < kC; ++k) m[k] = __ballot(in && cls == k);
        if ((threadIdx.x & 63u) == 0) {
#pragma unroll
          for (uint32_t k = 0; k < kC; ++k) class_wcnt[wave][k] = (uint32_t)__popcll(m[k]);
        }
        __syncthreads();
        uint32_t slot = 0;
#pragma unroll
        for (uint32_t k = 0; k < kC; ++k) {
          uint32_t before = 0, total = 0;
#pragma unroll
          for (uint32_t w = 0; w < kW; ++w) {
            const uint32_t n = __builtin_amdgcn_readfirstlane(class_wcnt[w][k]);
            if (w < wave) before += n;
            total += n;
          }
          const uint32_t rank = before + __builtin_amdgcn_mbcnt_hi((uint32_t)(m[k] >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)m[k], 0u));
          if (cls == k) slot = k * kClassRing + ((head[k] + fill[k] + rank) & kMask);
          fill[k] += total;
        }
        if (in) {
          ring_h[slot] = h;
          ring_ip[slot] = make_uint2(i_n, path);
        }
        nbase += stride;
        if (nbase + threadIdx.x < count) {  // the next window, with the policies of the mixed loop's next step
          path = ident ? nbase + threadIdx.x : ld_stream<kNtQueue>(in_q + nbase + threadIdx.x);
          h = b.hit[nbase + threadIdx.x];
        }
        cw_due = nbase < count;
        __syncthreads();  // the entries are in the rings; class_wcnt is free for the next ingest
      }
      if (held == 0) break;
      // ---- this step's entries: 256 of ring c, or (the queue is exhausted) the rings' remainders packed
      valid = false;
      if (most >= (uint32_t)kShadeBlock) {
        uint32_t hc = 0;
#pragma unroll
        for (uint32_t k = 0; k < kC; ++k)  // head[] and fill[] stay registers: no dynamic index
          if (c == k) {
            hc = head[k];
            head[k] = (head[k] + kShadeBlock) & kMask;
            fill[k] -= kShadeBlock;
          }
        const uint32_t slot = c * kClassRing + ((hc + threadIdx.x) & kMask);
        const uint2 ip = ring_ip[slot];
        h_s = ring_h[slot];
        i = ip.x;
        path_s = ip.y;
        valid = true;
      } else {
        uint32_t t = threadIdx.x, room = kShadeBlock;
#pragma unroll
        for (uint32_t k = 0; k < kC; ++k) {
          const uint32_t take = fill[k] < room ? fill[k] : room;  // uniform
          if (!valid && t < take) {
            const uint32_t slot = k * kClassRing + ((head[k] + t) & kMask);
            const uint2 ip = ring_ip[slot];
            h_s = ring_h[slot];
            i = ip.x;
            path_s = ip.y;
            valid = true;
          }
          t -= take;  // wraps for the lanes that took an entry: valid keeps them out
          head[k] = (head[k] + take) & kMask;
          fill[k] -= take;
          room -= take;
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < kC; ++k) {
        head[k] = __builtin_amdgcn_readfirstlane(head[k]);
        fill[k] = __builtin_amdgcn_readfirstlane(fill[k]);
      }
    }
    ShadeIO io;
    io.reset();
    MTX_STAMP_STEP(stp);
    io.st = stp;
    bool cont = false;
#if MTX_DIAG_CLASSES
    if constexpr (!CAM && !CLS && shade_has_classes(INT)) class_mix_count(s, bounce, valid, h_s);
#endif
    if (valid) {
      if constexpr (INT == MTX_INT_PSSMLT_SIMPLE)
        cont = shade_pssmlt(s, sv, b, p, bounce, path_s, i, h_s, io);
      else if constexpr (INT == MTX_INT_SIMPLE)
        cont = shade_simple<CAM>(s, sv, b, p, bounce, path_s, i, h_s, io);
      else if constexpr (INT == MTX_INT_PSSMLT_PATH)
        cont = shade_pssmlt_path(s, sv, b, p, bounce, path_s, i, h_s, io);
      else if constexpr (INT == MTX_INT_NERAD_RHS)
        cont = shade_nerad<false>(s, sv, b, bounce, path_s, i, h_s, io);
      else if constexpr (INT == MTX_INT_NERAD)
        cont = shade_nerad<true>(s, sv, b, bounce, path_s, i, h_s, io);
      else
        cont = shade_path<INT, CAM>(s, sv, b, p, bounce, path_s, i, h_s, io, wp);
    }
    (void)wp;
    const uint32_t path_c = path_s;
    if constexpr (!CLS) {
      path = path_n;
      h = hn;
      asm volatile("" ::"v"(io.warm));  // the warm-up load completes in this iteration
    } else {
      if (cw_due) load_class_word();  // the window's hit records arrived during the step
    }
    stp = io.st;

    uint32_t slot, sslot;
    block_append2<kShadeBlock>(cont, io.emit, io.emit && io.em_hi, out_cnt, parity, slot, sslot);
    MTX_STAMP(stp, 6);
    if (cont) {
      st_stream<kNtQueue>(out_q + slot, path_c);
      st_stream<kNtShadeSt>(b.ray_o[rp ^ 1u] + slot, io.nro);
      st_stream<kNtShadeSt>(b.ray_d[rp ^ 1u] + slot, io.nrd);
      if constexpr (!kNerad) st_stream<kNtShadeSt>(b.thr[rp ^ 1u] + slot, io.nthr);
      if constexpr (INT == MTX_INT_PATH_MIS || INT == MTX_INT_PATH || INT == MTX_INT_NRC || INT == MTX_INT_PSSMLT_PATH)
        st_stream<kNtShadeSt>(b.prev[rp ^ 1u] + slot, io.nprev);
      if constexpr (!kNerad) {
        st_stream<kNtShadeSt>(b.L[rp ^ 1u] + slot, io.nL);
        st_stream<kNtShadeSt>(b.misc[rp ^ 1u] + slot, io.nmisc);
      }
    } else if (!kNerad && valid) {
      st_stream<kNtShadeSt>(b.L[kFinal] + path_c, io.nL);
      if (!p.drop_end_misc) st_stream<kNtShadeSt>(b.misc[kFinal] + path_c, io.nmisc);
    }
    if (io.emit) {
      // the contribution goes to the path's L where the next shade (or the
      // film) reads it; the integrators that emit shadow rays (path-mis,
      // path, nrc, pssmltpath; not the nerad ones) store io.nL there
      const uint32_t li = (kNerad || !cont) ? kFinal * b.capacity + path_c : (rp ^ 1u) * b.capacity + slot;
      io.rec.d.w = __uint_as_float(li);
      if constexpr (!kNerad) io.rec.x.w = io.nL.w;  // final-value form: L.w (set after the NEE)
      st_stream<kNtShadeSt>(shadow_word(b, 0, sslot), io.rec.o);
      st_stream<kNtShadeSt>(shadow_word(b, 1, sslot), io.rec.d);
      st_stream<kNtShadeSt>(shadow_word(b, 2, sslot), io.rec.t);
      // a final-value record has no x: it is its target's L, stored above
      if constexpr (kNerad) st_stream<kNtShadeSt>(shadow_word(b, 3, sslot), io.rec.x);
    }
    MTX_STAMP(stp, 7);
    if constexpr (INT == MTX_INT_NRC || INT == MTX_INT_NERAD_RHS || INT == MTX_INT_NERAD) {
      if (INT != MTX_INT_NRC || p.nrc_cache) {
        const uint32_t q = block_reserve<kShadeBlock>(io.query ? 1u : 0u, b.cq_count);
        if (io.query) {
          b.cq_p[q] = io.qp;
          b.cq_d[q] = io.qd;
          b.cq_t[q] = io.qt;
        }
      }
    }
    MTX_STAMP(stp, 8);
  }
#if MTX_DIAG_STAMPS
  if ((threadIdx.x & 63u) == 0) {
    for (int k = 0; k < kStampSegs; ++k) atomicAdd(&g_shade_stamps[k], stp.acc[k]);
    atomicAdd(&g_shade_stamps[kStampSegs], stp.steps);
    atomicAdd(&g_shade_stamps[kStampSegs + 1], 1ull);
  }
#endif
}

// k_shade: the production kernel of every integrator (path-mis and path
// with class queues). k_shade_mixed: the mixed loop of those two, the form
// MTX_SHADE_CLASSES=0 launches.
template <int INT>
__global__ __launch_bounds__(kShadeBlock, kShadeMinBlocks) void k_shade(DevScene s, WaveBuffers b, ChunkParams p, uint32_t bounce) {
  shade_loop<INT, false, shade_has_classes(INT)>(s, b, p, bounce);
}
template <int INT>
__global__ __launch_bounds__(kShadeBlock, kShadeMinBlocks) void k_shade_mixed(DevScene s, WaveBuffers b, ChunkParams p, uint32_t bounce) {
  static_assert(shade_has_classes(INT), "k_shade_mixed: the integrators whose k_shade runs class queues");
  shade_loop<INT, false>(s, b, p, bounce);
}
// Bounce 0 of a cam0 chunk (path, path-mis, nrc, simple): the camera sample
// is derived, not loaded. Its own kernel: k_shade keeps its code and
// registers (in one kernel the camera's and the chunk's scalars stay live
// through every bounce's loop, and k_shade<NRC>, at its 168-VGPR budget,
// spills), and bounce == 0 is a constant here (no state loads at all).
template <int INT>
__global__ __launch_bounds__(kShadeBlock, kShadeMinBlocks) void k_shade_cam(DevScene s, WaveBuffers b, ChunkParams p) {
  static_assert(INT == MTX_INT_PATH || INT == MTX_INT_PATH_MIS || INT == MTX_INT_NRC || INT == MTX_INT_SIMPLE,
                "k_shade_cam: the integrators whose bounce-0 shade derives the camera sample");
  shade_loop<INT, true>(s, b, p, 0u);
}

// Paths still queued after a chunk's last bounce (its depth limit stops
// every integrator's paths first; kept so that no loop bound can leave a
// result in a queue plane): their L / misc move to the per-path plane.
// A path-mis path's final L.w holds valid_ray (end_w), not its prev_bsdf_pdf.
__global__ void k_flush_tail(WaveBuffers b, uint32_t bounce, uint32_t integrator) {
  const uint32_t n = b.counters[4 * bounce];
  const uint32_t *q = b.queue[bounce & 1];
  const uint32_t rp = (bounce + b.ray_par) & 1u;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const uint32_t path = q[k];
    float4 L = b.L[rp][k];
    const uint4 m = b.misc[rp][k];
    // decided by the shade variant: ReSTIR GI's secondary paths are shaded by
    // the path-mis kernel (launch_shade), so their final L.w is valid_ray too,
    // the bits k_path_mega<PATH_MIS> stores for the same path
    if (integrator == MTX_INT_PATH_MIS || integrator == MTX_INT_RESTIR_GI) L.w = end_w(m.w >> 16);
    b.L[kFinal][path] = L;
    b.misc[kFinal][path] = m;
  }
}

// L += T * Field(query) for the NRC cache queries of a chunk (nrc.py L is a
// plain sum: L = L + T * out, as the oracle-side composition in the tests).
__global__ void k_cache_apply(WaveBuffers b, const float *out, const uint32_t *perm) {
  const uint32_t n = *b.cq_count;
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const float4 t = b.cq_t[perm ? perm[q] : q];  // out row q belongs to query perm[q]
    const uint32_t path = __float_as_uint(t.w);
    float4 L = b.L[kFinal][path];
    L.x = L.x + t.x * out[3 * (size_t)q];
    L.y = L.y + t.y * out[3 * (size_t)q + 1];
    L.z = L.z + t.z * out[3 * (size_t)q + 2];
    b.L[kFinal][path] = L;
  }
}

// ---------------------------------------------------------------------------
// PSSMLT chain kernels (pssmlt.py:167-228). Chains of a chunk keep their
// state in HBM across all Metropolis iterations; chain i of the chunk is
// chain s = sample_offset + i % spp of pixel px0 + i / spp, sampler lane
// pixel * spp_total + s (pssmlt.py:188-193 with wavefront W*H*spp_total): a
// chain range [sample_offset, sample_offset + spp) of every pixel is a shard
// of the spp_total-chain render (multi-GPU, chains never leave their pixel).
// ---------------------------------------------------------------------------
__global__ void k_mlt_init(WaveBuffers b, ChunkParams p, uint32_t max_depth) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_paths) return;
  const uint32_t q = i / p.spp;
  const Pcg32 rng = sampler_lane(p.seed, (p.px0 + q) * p.spp_total + p.sample_offset + (i - q * p.spp));
  b.misc[kFinal][i] = st_rng(rng, 0u);
  // offset = 0.5, cumulative_weight = 0 (:198-200); w: vertex depths that may
  // differ between the proposed and current buffers (k_mlt_end)
  b.mlt_cur[i] = make_float4(0.5f, 0.5f, 0.f, 0.f);
  b.mlt_L[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (uint32_t d = 0; d < max_depth; ++d) {
    b.vpath[(size_t)d * b.capacity + i] = make_float4(0.f, 0.f, 0.f, 0.f);
    b.vprop[(size_t)d * b.capacity + i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.integrator == MTX_INT_PSSMLT_PATH) {
      b.vpath_es[(size_t)d * b.capacity + i] = make_float2(0.f, 0.f);
      b.vprop_es[(size_t)d * b.capacity + i] = make_float2(0.f, 0.f);
    }
  }
}

// render_sample head (:122-129): offset mutation, camera ray, path state.
__global__ void k_mlt_begin(DevScene s, WaveBuffers b, ChunkParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) b.counters[0] = p.n_paths;
  if (i >= p.n_paths) return;
  const uint4 mi = b.misc[kFinal][i];
  Pcg32 rng = ld_rng(mi);
  const V2 u = rng.next_2d();
  V2 po;
  if (p.large_step) {
    po = u;
  } else {  // mutate_offset (:245-255)
    const float4 cur = b.mlt_cur[i];
    const V2 g = square_to_std_normal(u);
    const float k = 0.31622776601683794f;  // sqrt(0.1)
    po = V2{dr_clamp(g.x * k + cur.x, 0.f, 1.f), dr_clamp(g.y * k + cur.y, 0.f, 1.f)};
  }
  const uint32_t pix = p.px0 + i / p.spp;
  const uint32_t y = pix / p.width, x = pix - y * p.width;
  const V2 sp = V2{((float)x + po.x) / (float)p.width, ((float)y + po.y) / (float)p.height};
  const Ray ray = camera_ray(s.camera, sp);
  b.mlt_prop[i] = make_float2(po.x, po.y);
  b.ray_o[0][i] = f4(ray.o, ray.maxt);  // queue position i (identity)
  b.ray_d[0][i] = f4(ray.d, 0.f);
  b.thr[0][i] = make_float4(1.f, 1.f, 1.f, 1.f);
  b.L[0][i] = make_float4(0.f, 0.f, 0.f, 1.f);  // prev_bsdf_pdf = 1 (queue position i)
  // pssmltpath.py:39-44: prev_si zero, prev_bsdf_delta = True, valid_ray = scene.environment() is not None
  const uint32_t fl =
      p.integrator == MTX_INT_PSSMLT_PATH ? ((PF_PREV_DELTA | (s.has_env ? PF_VALID_RAY : 0u)) << 16) : 0u;
  if (p.integrator == MTX_INT_PSSMLT_PATH) b.prev[0][i] = make_float4(0.f, 0.f, 0.f, 0.f);
  b.misc[0][i] = st_rng(rng, fl);
  if (!p.ident0) b.queue[0][i] = i;
}

// render_sample tail (:137-159): acceptance, cumulative weights, state swap.
__global__ void k_mlt_end(WaveBuffers b, ChunkParams p, uint32_t max_depth) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_paths) return;
  const uint4 mi = b.misc[kFinal][i];
  Pcg32 rng = ld_rng(mi);
  const float4 lp4 = b.L[kFinal][i];
  const V3 Lp = V3{lp4.x, lp4.y, lp4.z};
  float4 cur = b.mlt_cur[i];
  const float4 lc4 = b.mlt_L[i];
  const float a = dr_clamp(luminance(Lp) / luminance(V3{lc4.x, lc4.y, lc4.z}), 0.f, 1.f);
  const bool accept = rng.next_1d() < a;
  if (accept) {
    cur.z = a;
  } else {
    cur.z += 1.f - a;
  }
  // The reference copies all max_depth proposed vertices on acceptance
  // (dr.tile(accept, max_depth), :155-158). A proposal writes depths
  // 0..depth only (its final depth is in misc), so the two vertex buffers can
  // differ only below the largest such bound since the chain's last
  // acceptance (cur.w): copying those depths gives the same current path.
  uint32_t dirty = max((uint32_t)cur.w, min(max_depth, (mi.w & 0xffffu) + 1u));
  if (accept) {
    const float2 po = b.mlt_prop[i];
    cur.x = po.x;
    cur.y = po.y;
    b.mlt_L[i] = f4(Lp, 0.f);
    for (uint32_t d = 0; d < dirty; ++d)
      b.vpath[(size_t)d * b.capacity + i] = b.vprop[(size_t)d * b.capacity + i];
    if (p.integrator == MTX_INT_PSSMLT_PATH)
      for (uint32_t d = 0; d < dirty; ++d)
        b.vpath_es[(size_t)d * b.capacity + i] = b.vprop_es[(size_t)d * b.capacity + i];
    dirty = 0;
  }
  cur.w = (float)dirty;
  b.mlt_cur[i] = cur;
  b.misc[kFinal][i] = st_rng(rng, 0u);
}

void launch_raygen_camera(const DevScene &s, const WaveBuffers &b, const ChunkParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_raygen_camera, dim3(blocks_for(p.n_paths, 256)), dim3(256), 0, st, s, b, p);
}
void launch_raygen_rays(const DevScene &s, const WaveBuffers &b, const ChunkParams &p, const float *rays,
                        const uint32_t *lanes, uint32_t rng_skip, hipStream_t st) {
  hipLaunchKernelGGL(k_raygen_rays, dim3(blocks_for(p.n_paths, 256)), dim3(256), 0, st, s, b, p, rays, lanes,
                     rng_skip);
}
void launch_shade(const DevScene &s, const WaveBuffers &b, const ChunkParams &p, uint32_t bounce, int grid,
                  hipStream_t st, bool classes) {
  const size_t rings = shade_class_lds_bytes();
  if (bounce == 0 && p.cam0) {  // no stored raygen (mtx_render sets cam0 for these four only)
    switch (p.integrator) {
      case MTX_INT_PATH:
        hipLaunchKernelGGL(k_shade_cam<MTX_INT_PATH>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p);
        break;
      case MTX_INT_NRC:
        hipLaunchKernelGGL(k_shade_cam<MTX_INT_NRC>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p);
        break;
      case MTX_INT_SIMPLE:
        hipLaunchKernelGGL(k_shade_cam<MTX_INT_SIMPLE>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p);
        break;
      default:
        hipLaunchKernelGGL(k_shade_cam<MTX_INT_PATH_MIS>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p);
    }
    return;
  }
  switch (p.integrator) {
    case MTX_INT_PATH:
      if (classes)
        hipLaunchKernelGGL(k_shade<MTX_INT_PATH>, dim3(grid), dim3(kShadeBlock), rings, st, s, b, p, bounce);
      else
        hipLaunchKernelGGL(k_shade_mixed<MTX_INT_PATH>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p, bounce);
      break;
    case MTX_INT_NRC:
      hipLaunchKernelGGL(k_shade<MTX_INT_NRC>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p, bounce);
      break;
    case MTX_INT_PSSMLT_SIMPLE:
      hipLaunchKernelGGL(k_shade<MTX_INT_PSSMLT_SIMPLE>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p, bounce);
      break;
    case MTX_INT_SIMPLE:
      hipLaunchKernelGGL(k_shade<MTX_INT_SIMPLE>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p, bounce);
      break;
    case MTX_INT_PSSMLT_PATH:
      hipLaunchKernelGGL(k_shade<MTX_INT_PSSMLT_PATH>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p, bounce);
      break;
    case MTX_INT_NERAD_RHS:
      hipLaunchKernelGGL(k_shade<MTX_INT_NERAD_RHS>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p, bounce);
      break;
    case MTX_INT_NERAD:
      hipLaunchKernelGGL(k_shade<MTX_INT_NERAD>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p, bounce);
      break;
    default:
      if (classes)
        hipLaunchKernelGGL(k_shade<MTX_INT_PATH_MIS>, dim3(grid), dim3(kShadeBlock), rings, st, s, b, p, bounce);
      else
        hipLaunchKernelGGL(k_shade_mixed<MTX_INT_PATH_MIS>, dim3(grid), dim3(kShadeBlock), 0, st, s, b, p, bounce);
  }
}
// MTX_DIAG_STAMPS builds: read (and zero) the shade stamp sums; -1 otherwise.
int shade_stamps(unsigned long long *out) {
#if MTX_DIAG_STAMPS
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_shade_stamps), sizeof(unsigned long long) * (kStampSegs + 2)) !=
      hipSuccess)
    return -1;
  unsigned long long z[kStampSegs + 2] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_shade_stamps), z, sizeof(z)) != hipSuccess) return -1;
  return kStampSegs;
#else
  (void)out;
  return -1;
#endif
}
// MTX_DIAG_CLASSES builds: read (and zero) the class-mix counts, kMixBounces rows
// of kMixWords; returns kMixWords, or -1 otherwise.
int shade_class_mix(unsigned long long *out) {
#if MTX_DIAG_CLASSES
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_class_mix), sizeof(unsigned long long) * kMixBounces * kMixWords) !=
      hipSuccess)
    return -1;
  unsigned long long z[kMixBounces * kMixWords] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_class_mix), z, sizeof(z)) != hipSuccess) return -1;
  return (int)kMixWords;
#else
  (void)out;
  return -1;
#endif
}
int shade_blocks_per_cu(bool classes) {
  int nb = 0;
  const hipError_t e =
      classes ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_shade<MTX_INT_PATH_MIS>, kShadeBlock,
                                                             shade_class_lds_bytes())
              : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_shade_mixed<MTX_INT_PATH_MIS>, kShadeBlock, 0);
  if (e != hipSuccess || nb <= 0)
    nb = 2;
  return nb;
}
void launch_cache_apply(const WaveBuffers &b, const float *out, uint32_t capacity, hipStream_t st,
                        const uint32_t *perm) {
  const unsigned blocks = (unsigned)std::min<uint64_t>((capacity + 255) / 256, 16384);
  hipLaunchKernelGGL(k_cache_apply, dim3(std::max(1u, blocks)), dim3(256), 0, st, b, out, perm);
}
void launch_flush_tail(const WaveBuffers &b, uint32_t bounce, uint32_t capacity, uint32_t integrator,
                       hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<uint64_t>((capacity + 255) / 256, 1024);
  hipLaunchKernelGGL(k_flush_tail, dim3(std::max(1u, blocks)), dim3(256), 0, st, b, bounce, integrator);
}
void launch_mlt_init(const WaveBuffers &b, const ChunkParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_mlt_init, dim3(blocks_for(p.n_paths, 256)), dim3(256), 0, st, b, p, p.max_depth);
}
void launch_mlt_begin(const DevScene &s, const WaveBuffers &b, const ChunkParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_mlt_begin, dim3(blocks_for(p.n_paths, 256)), dim3(256), 0, st, s, b, p);
}
void launch_mlt_end(const WaveBuffers &b, const ChunkParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_mlt_end, dim3(blocks_for(p.n_paths, 256)), dim3(256), 0, st, b, p, p.max_depth);
}

}  // namespace mtxd

#ifdef MTX_TEST_BAD_SHADOW_FORM
// tests/test_abi.py::test_shadow_record_form_is_checked: an integrator whose L
// lives outside k_shade's stores asking for the final-value form must not compile.
__device__ void mtx_bad_shadow_form(mtxd::ShadeIO &io, const mtx::SurfaceInteraction &si,
                                    const mtx::DirectionSample &ds) {
  const mtx::V3 L = mtx::v3s(0.f);
  mtxd::make_shadow<MTX_INT_NERAD_RHS, true>(io, si, ds, L, L, L, true, &L);
}
#endif
