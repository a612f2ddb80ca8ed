// mega.hip — the two per-lane megakernels for short wavefronts: k_path_mega
// runs every bounce of a queued path (closest hit, shade_path, the NEE shadow
// ray applied at once), k_rs_stage_a runs ReSTIR GI's stage A of a pixel
// sample the same way. Same per-path operations as the wavefront kernels, so
// the same bits.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "restir_dev.h"
#include "shade_dev.h"

namespace mtxd {

// Path megakernel for short wavefronts (ReSTIR GI's secondary paths of a
// row band): each thread takes one queued path and runs all of its bounces
// -- closest hit (traverse_closest), shade_path, the NEE shadow ray
// (traverse_occ) applied to its L at once -- with its state kept at its own
// queue position (no compaction). A short queue leaves most lanes of the
// wavefront kernels idle and each launch waits for its slowest ray, once per
// bounce and kernel; here a path waits only on its own chain. Same operations
// per path as the wavefront kernels (same hits: the closest hit does not
// depend on the visit order; same shading code), so the same bits. The block's
// dynamic LDS holds one traversal stack column per thread (stack_bytes).
#ifndef MTX_MEGA_MIN_BLOCKS
#define MTX_MEGA_MIN_BLOCKS 3  // A/B: 4 = <= 128 VGPRs (spills), every band path resident at once
#endif
// The traversals index their LDS stack columns with the stride kTraceBlock and
// stack_bytes() sizes the allocation with it: a megakernel block of another
// width would let threads share stack words.
static_assert(kShadeBlock == kTraceBlock, "k_path_mega: stack column stride must equal the block width");
// Round 5: lanes, not waves, take paths. Each iteration a lane runs ONE
// bounce of its path; a lane whose path has ended takes the next queued path
// as soon as kMegaRefill lanes of its wave are idle (one claim atomic per
// refill for all of them, consecutive queue positions), so a wave no longer
// waits for the longest of its 64 paths before any lane starts another (the
// round-4 form claimed 64 paths per wave and ran them to completion).
#ifndef MTX_MEGA_REFILL
#define MTX_MEGA_REFILL 16  // idle lanes of a wave that trigger a claim (64: the round-4 whole-wave batches)
#endif
template <int INT>
__global__ __launch_bounds__(kShadeBlock, MTX_MEGA_MIN_BLOCKS) void k_path_mega(DevScene s, WaveBuffers b, ChunkParams p) {
  static_assert(INT == MTX_INT_PATH_MIS || INT == MTX_INT_PATH, "megakernel: path / path-mis only");
  extern __shared__ int4 mega_lds[];
  const SceneView sv = make_view(s);
  const uint32_t count = b.counters[0];
  const uint32_t iters = p.max_depth > 1u ? p.max_depth : 1u;
  int32_t *stk = reinterpret_cast<int32_t *>(mega_lds) + threadIdx.x;
  uint32_t *ostk = reinterpret_cast<uint32_t *>(mega_lds) + threadIdx.x;  // the same column
  const uint32_t lane = threadIdx.x & 63u;
  bool has = false, drained = false;
  uint32_t qi = 0, path = 0, bounce = 0;
  while (true) {
    // ---- refill: the idle lanes of the wave claim consecutive queue positions
    if (!drained) {
      const uint64_t idle = __ballot(!has);
      const uint32_t n_idle = (uint32_t)__popcll(idle);
      if (n_idle >= MTX_MEGA_REFILL || idle == ~0ull) {
        const uint32_t leader = (uint32_t)(__ffsll((unsigned long long)idle) - 1);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&b.counters[2], n_idle);
        base = __builtin_amdgcn_readlane(base, leader);
        if (base + n_idle >= count) drained = true;
        const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        if (!has && base + rk < count) {
          has = true;
          qi = base + rk;
          path = p.ident0 ? qi : b.queue[0][qi];
          bounce = 0;
        }
      }
    }
    if (__ballot(has) == 0) break;
    if (has) {
      // ---- one bounce of the lane's path
      const uint32_t rp = (bounce + b.ray_par) & 1u;
      const float4 o4 = b.ray_o[rp][qi], d4 = b.ray_d[rp][qi];
      const TraceRay r = make_trace_ray(V3{o4.x, o4.y, o4.z}, V3{d4.x, d4.y, d4.z}, o4.w);
      float tbest = o4.w, bu = 0.f, bv = 0.f;
      uint32_t prim = 0xffffffffu, nv = 0, tv = 0;
      traverse_closest(s, stk, r, tbest, prim, bu, bv, nv, tv);
      const float4 h = make_float4(prim == 0xffffffffu ? kInf : tbest, __uint_as_float(prim), bu, bv);
      ShadeIO io;
      io.reset();
      const bool cont = shade_path<INT>(s, sv, b, p, bounce, path, qi, h, io);
      if (io.emit) {
        const float4 so = io.rec.o, sd = io.rec.d;
        const TraceRay sr = make_trace_ray(V3{so.x, so.y, so.z}, V3{sd.x, sd.y, sd.z}, so.w);
        apply_shadow_rec(io.nL, io.rec, traverse_occ(s, ostk, sr, so.w, nv, tv));
      }
      ++bounce;
      if (cont && bounce < iters) {
        b.ray_o[rp ^ 1u][qi] = io.nro;
        b.ray_d[rp ^ 1u][qi] = io.nrd;
        b.thr[rp ^ 1u][qi] = io.nthr;
        b.prev[rp ^ 1u][qi] = io.nprev;
        b.L[rp ^ 1u][qi] = io.nL;
        b.misc[rp ^ 1u][qi] = io.nmisc;
      } else {
        // ended, or still queued after the last bounce (k_flush_tail's move:
        // a path-mis path's final L.w holds valid_ray)
        float4 L = io.nL;
        if (cont && INT == MTX_INT_PATH_MIS) L.w = end_w(io.nmisc.w >> 16);
        b.L[kFinal][path] = L;
        if (!p.drop_end_misc || cont) b.misc[kFinal][path] = io.nmisc;
        has = false;
      }
    }
  }
}

// ReSTIR GI stage A of a short band in ONE launch (round 5): a lane takes a
// pixel sample t of the band and runs restirgi.py's sample_initial for it --
// the camera ray (k_raygen_camera), the primary closest hit, k_rs_begin's
// emittance and BSDF / hemisphere sample (:419-448), then the secondary
// path's bounces (the path megakernel's body, :459-588) and k_rs_collect's
// L_o / sampler store -- with its path state at its own position t, then
// takes the next sample (lanes refill as in k_path_mega). The same per-lane
// operations as the five launches it replaces (hits do not depend on the
// traversal order), so the same reservoirs and films; k_rs_temporal follows
// as its own launch (it reads other pixels' samples).
__global__ __launch_bounds__(kShadeBlock, MTX_MEGA_MIN_BLOCKS) void k_rs_stage_a(DevScene s, WaveBuffers b,
                                                                                  ChunkParams p, RestirBuffers r) {
  extern __shared__ int4 mega_lds[];
  const SceneView sv = make_view(s);
  const uint32_t count = r.nb;
  const uint32_t iters = p.max_depth > 1u ? p.max_depth : 1u;
  int32_t *stk = reinterpret_cast<int32_t *>(mega_lds) + threadIdx.x;
  uint32_t *ostk = reinterpret_cast<uint32_t *>(mega_lds) + threadIdx.x;
  // b.ray_par == 1 (launch_rs_stage_a): the secondary loop's bounce-0 rays are parity 1
  const uint32_t lane = threadIdx.x & 63u;
  const size_t n = r.n;
  bool has = false, drained = false, started = false;
  uint32_t t = 0, bounce = 0;
  while (true) {
    if (!drained) {
      const uint64_t idle = __ballot(!has);
      const uint32_t n_idle = (uint32_t)__popcll(idle);
      if (n_idle >= MTX_MEGA_REFILL || idle == ~0ull) {
        const uint32_t leader = (uint32_t)(__ffsll((unsigned long long)idle) - 1);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&b.counters[2], n_idle);
        base = __builtin_amdgcn_readlane(base, leader);
        if (base + n_idle >= count) drained = true;
        const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
        if (!has && base + rk < count) {
          has = true;
          started = false;
          t = base + rk;
        }
      }
    }
    if (__ballot(has) == 0) break;
    if (has) {
      const uint32_t i = r.lane0 + t;
      float4 o4, d4;
      Pcg32 rng;
      if (!started) {
        // the camera ray of sample t (k_raygen_camera; init_path's sampler state)
        const uint32_t px_local = t / p.spp, smp = t - px_local * p.spp;
        const uint32_t pix = p.px0 + px_local;
        const uint32_t y = pix / p.width, x = pix - y * p.width;
        rng = sampler_lane(p.seed, pix * p.spp_total + p.sample_offset + smp);
        const V2 u = rng.next_2d();  // film jitter (path.py:45)
        const Ray ray = camera_ray(s.camera, V2{((float)x + u.x) / (float)p.width, ((float)y + u.y) / (float)p.height});
        o4 = f4(ray.o, ray.maxt);
        d4 = f4(ray.d, 0.f);
      } else {
        const uint32_t rp = (bounce + 1u) & 1u;
        o4 = b.ray_o[rp][t];
        d4 = b.ray_d[rp][t];
      }
      const TraceRay tr = make_trace_ray(V3{o4.x, o4.y, o4.z}, V3{d4.x, d4.y, d4.z}, o4.w);
      float tbest = o4.w, bu = 0.f, bv = 0.f;
      uint32_t prim = 0xffffffffu, nv = 0, tv = 0;
      traverse_closest(s, stk, tr, tbest, prim, bu, bv, nv, tv);
      const float4 h = make_float4(prim == 0xffffffffu ? kInf : tbest, __uint_as_float(prim), bu, bv);
      float4 Lf;
      uint4 mf;
      bool done = false;
      if (!started) {
        // k_rs_begin (:419-448)
        r.prim_hit[i] = h;
        r.prim_dir[i] = d4;
        const SurfaceInteraction si = compute_si_dev(s, h.x, __float_as_uint(h.y), h.z, h.w, V3{d4.x, d4.y, d4.z});
        r.emit[i] = f4(emitter_eval(sv, si.emitter, si.wi), 0.f);
        V3 wo;
        float pdf;
        if (r.flags & MTX_RESTIR_BSDF_SAMPLING) {
          const float s1 = rng.next_1d();
          const V2 s2 = rng.next_2d();
          BSDFSample bs;
          bs.wo = v3s(0.f);
          bs.pdf = 0.f;
          if (si.valid) bsdf_sample(sv.bsdf, sv.materials[si.material], si.uv, si.wi, s1, s2, &bs);
          wo = bs.wo;
          pdf = bs.pdf;
        } else {
          wo = square_to_uniform_hemisphere(rng.next_2d());
          pdf = square_to_uniform_hemisphere_pdf(wo);
        }
        r.cur[i] = si.valid ? f4(si.p, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        r.cur[n + i] = si.valid ? f4(si.n, pdf) : make_float4(0.f, 0.f, 0.f, pdf);
        if (si.valid) {
          const Ray nr = spawn_ray(si.p, si.n, to_world(si.sh, wo));
          b.ray_o[1][t] = f4(nr.o, nr.maxt);
          b.ray_d[1][t] = f4(nr.d, 0.f);
          b.misc[1][t] = st_rng(rng, PF_PREV_DELTA << 16);  // depth 0, prev_bsdf_delta
          started = true;
          bounce = 0;
        } else {
          rng.advance(6);
          Lf = make_float4(0.f, 0.f, 0.f, 1.f);
          mf = st_rng(rng, 0u);
          b.rs_xs[t] = make_float4(0.f, 0.f, 0.f, 0.f);
          b.rs_ns[t] = make_float4(0.f, 0.f, 0.f, 0.f);
          done = true;
        }
      } else {
        // one bounce of the secondary path (k_path_mega's body)
        const uint32_t rp = (bounce + 1u) & 1u;
        ShadeIO io;
        io.reset();
        const bool cont = shade_path<MTX_INT_PATH_MIS>(s, sv, b, p, bounce, t, t, h, io);
        if (io.emit) {
          const float4 so = io.rec.o, sd = io.rec.d;
          const TraceRay sr = make_trace_ray(V3{so.x, so.y, so.z}, V3{sd.x, sd.y, sd.z}, so.w);
          apply_shadow_rec(io.nL, io.rec, traverse_occ(s, ostk, sr, so.w, nv, tv));
        }
        ++bounce;
        if (cont && bounce < iters) {
          b.ray_o[rp ^ 1u][t] = io.nro;
          b.ray_d[rp ^ 1u][t] = io.nrd;
          b.thr[rp ^ 1u][t] = io.nthr;
          b.prev[rp ^ 1u][t] = io.nprev;
          b.L[rp ^ 1u][t] = io.nL;
          b.misc[rp ^ 1u][t] = io.nmisc;
        } else {
          Lf = io.nL;
          if (cont) Lf.w = end_w(io.nmisc.w >> 16);
          mf = io.nmisc;
          done = true;
        }
      }
      if (done) {
        // k_rs_collect: L_o = select(valid_ray, result, 0) (:588), x_s / n_s of
        // the first secondary hit (written by the bounce-0 shade), sampler state
        const bool valid_ray = ((mf.w >> 16) & PF_VALID_RAY) != 0;
        r.cur[2 * n + i] = b.rs_xs[t];
        r.cur[3 * n + i] = b.rs_ns[t];
        r.cur[4 * n + i] = valid_ray ? make_float4(Lf.x, Lf.y, Lf.z, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        r.rng[i] = mf;
        has = false;
      }
    }
  }
}
void launch_rs_stage_a(const DevScene &s, const WaveBuffers &b, const ChunkParams &p, const RestirBuffers &r,
                       int grid, hipStream_t st) {
  WaveBuffers b1 = b;
  b1.ray_par = 1;
  hipLaunchKernelGGL(k_rs_stage_a, dim3(grid), dim3(kShadeBlock), stack_bytes(s), st, s, b1, p, r);
}

// Resident blocks per CU of the path megakernel (its LDS stacks and the shade
// register budget).
int mega_blocks_per_cu(const DevScene &s) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_path_mega<MTX_INT_PATH_MIS>, kShadeBlock, stack_bytes(s)) !=
          hipSuccess ||
      nb <= 0)
    nb = 1;
  return nb;
}
void launch_path_mega(const DevScene &s, const WaveBuffers &b, const ChunkParams &p, int grid, hipStream_t st) {
  if (p.integrator == MTX_INT_PATH)
    hipLaunchKernelGGL(k_path_mega<MTX_INT_PATH>, dim3(grid), dim3(kShadeBlock), stack_bytes(s), st, s, b, p);
  else
    hipLaunchKernelGGL(k_path_mega<MTX_INT_PATH_MIS>, dim3(grid), dim3(kShadeBlock), stack_bytes(s), st, s, b, p);
}

}  // namespace mtxd
