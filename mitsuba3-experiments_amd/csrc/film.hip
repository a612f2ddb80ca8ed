// film.hip — the film of the fixed integrators: a path's final L
// (final_L, k_collect), the deterministic gather-form splat in two stages
// (k_film_src / k_film_src_staged, k_film_gather) and the PSSMLT chains'
// running accumulation (k_mlt_film).
#include <hip/hip_runtime.h>

#include "camera_dev.h"
#include "device_common.h"
#include "film_dev.h"
#include "mtx_core/film.h"

namespace mtxd {

// Stage 1 per source pixel ((2N+1)^2 footprint of the reconstruction filter,
// samples in order), stage 2 per film pixel (the (2N+1)^2 neighbours in fixed
// order). The kernels are templates on the filter's reach N and the filter F
// (mtx_core/film.h): <1, tent> is the default, <0, box> and <2, gaussian> are
// opt-in (mtx_render_args.rfilter). See DESIGN.md.

// valid_ray of an ended path-mis path, from its final L.w (shade_dev.h end_w).
__device__ __forceinline__ bool end_valid(float lw) { return lw != 0.f; }
__device__ __forceinline__ V3 final_L(const WaveBuffers &b, const ChunkParams &p, uint32_t path) {
  const float4 l = b.L[kFinal][path];
  V3 L = V3{l.x, l.y, l.z};
  if (p.integrator == MTX_INT_PATH_MIS && !end_valid(l.w)) L = v3s(0.f);  // path-mis.py:155
  return L;
}

// Pixel-major chunks: a pixel's samples are contiguous, so one wave stages
// 64 pixels x kFilmStage samples through LDS with coalesced loads, then each
// lane accumulates its own pixel in sample order (same order as below).
constexpr int kFilmStage = 8;  // 8 (11.5 KB of LDS per wave, twice the waves per CU) beat 16 by 0.8 ms, and 4

// film_taps, film_max_block and film_accumulate (the splat of one sample):
// film_dev.h, shared with the building blocks' film put (blocks.hip).

// Partial film slots (mtx_core/common.h film_slot): with p.film_slots == 8
// a lane moves on to the next slot's contribution planes whenever its sample
// index passes a slot end (the same for every lane of the launch: no
// divergence) and writes all 8 slots (zeros for slots without samples);
// otherwise one slot. contrib: [slot][K][band_px], K = (2N+1)^2 taps.
template <int K>
struct FilmSlots {
  uint32_t cur, end, T, mask;
  bool eight;
  __device__ __forceinline__ void init(const ChunkParams &p) {
    eight = p.film_slots == 8;
    mask = eight ? p.slot_mask : 1u;
    T = p.spp_total;
    cur = 0;
    end = eight ? film_slot_end(0, T) : 0xffffffffu;
  }
  __device__ __forceinline__ void flush(float4 *acc, float4 *contrib, const ChunkParams &p, size_t o) {
    const bool used = (mask >> cur) & 1u;  // a slot without samples of this render stays unwritten
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (used) contrib[((size_t)cur * K + k) * p.band_px + o] = acc[k];
      acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    ++cur;
    end = cur < 7 ? film_slot_end(cur, T) : 0xffffffffu;
  }
  // before accumulating global sample g
  __device__ __forceinline__ void advance(uint32_t g, float4 *acc, float4 *contrib, const ChunkParams &p, size_t o,
                                          bool write) {
    while (g >= end) {
      if (write) {
        flush(acc, contrib, p, o);
      } else {
        ++cur;
        end = cur < 7 ? film_slot_end(cur, T) : 0xffffffffu;
      }
    }
  }
  __device__ __forceinline__ void finish(float4 *acc, float4 *contrib, const ChunkParams &p, size_t o) {
    const uint32_t n = eight ? 8u : 1u;
    while (cur < n) flush(acc, contrib, p, o);
  }
};

template <int N, uint32_t F>
__global__ __launch_bounds__(64) void k_film_src_staged(WaveBuffers b, ChunkParams p, float4 *contrib) {
  constexpr int S = kFilmStage, K = film_taps(N);
  __shared__ float sv[5][64][S + 1];  // L.xyz, pos.xy
  const uint32_t q0 = blockIdx.x * 64, lane = threadIdx.x, q = q0 + lane;
  const uint32_t pix = p.px0 + q;
  const int y = (int)(pix / p.width), x = (int)(pix - (uint32_t)y * p.width);
  const bool mask_valid = p.integrator == MTX_INT_PATH_MIS;
  const bool live = q < p.n_px;
  const size_t o = (size_t)(pix - p.band_y0 * p.width);  // contrib: [slot][K][band_px]
  FilmSlots<K> fs;
  fs.init(p);
  float4 acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (uint32_t s0 = 0; s0 < p.spp; s0 += S) {
    const uint32_t ns = min((uint32_t)S, p.spp - s0);
#pragma unroll 4
    for (int it = 0; it < S; ++it) {
      const uint32_t e = (uint32_t)it * 64 + lane, j = e / S, sm = e % S;
      if (q0 + j < p.n_px && sm < ns) {
        const uint32_t path = (q0 + j) * p.spp + s0 + sm;
        float4 l = ld_stream<kNtQueue>(b.L[kFinal] + path);
        if (mask_valid && !end_valid(l.w)) l = make_float4(0.f, 0.f, 0.f, 0.f);
        sv[0][j][sm] = l.x;
        sv[1][j][sm] = l.y;
        sv[2][j][sm] = l.z;
        if (!p.cam0) {
          const float2 ps = ld_stream<kNtQueue>(b.pos + path);
          sv[3][j][sm] = ps.x;
          sv[4][j][sm] = ps.y;
        }
      }
    }
    __syncthreads();
    for (uint32_t sm = 0; sm < ns; ++sm) {
      fs.advance(p.sample_offset + s0 + sm, acc, contrib, p, o, live);
      if (live) {
        float2 ps;
        if (p.cam0)  // no stored raygen: the sample's film position is derived
          camera_film_pos(p, pix, (uint32_t)x, (uint32_t)y, s0 + sm, ps);
        else
          ps = make_float2(sv[3][lane][sm], sv[4][lane][sm]);
        film_accumulate<N, F>(acc, x, y, ps, V3{sv[0][lane][sm], sv[1][lane][sm], sv[2][lane][sm]});
      }
    }
    __syncthreads();
  }
  if (!live) return;
  fs.finish(acc, contrib, p, o);
}

template <int N, uint32_t F>
__global__ __launch_bounds__(film_max_block(N)) void k_film_src(WaveBuffers b, ChunkParams p, float4 *contrib) {
  constexpr int K = film_taps(N);
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.n_px) return;
  const uint32_t pix = p.px0 + q;
  const int y = (int)(pix / p.width), x = (int)(pix - (uint32_t)y * p.width);
  const size_t o = (size_t)(pix - p.band_y0 * p.width);  // contrib: [slot][K][band_px]
  FilmSlots<K> fs;
  fs.init(p);
  float4 acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (uint32_t sidx = 0; sidx < p.spp; ++sidx) {
    fs.advance(p.sample_offset + sidx, acc, contrib, p, o, true);
    const uint32_t path = q * p.spp + sidx;
    float2 ps;
    if (p.cam0)  // no stored raygen: the sample's film position is derived
      camera_film_pos(p, pix, (uint32_t)x, (uint32_t)y, sidx, ps);
    else
      ps = b.pos[path];
    film_accumulate<N, F>(acc, x, y, ps, final_L(b, p, path));
  }
  fs.finish(acc, contrib, p, o);
}

// Stage 2: per film pixel and slot the (2N+1)^2 neighbours in (dy, dx) order, then
// the slots' fixed binary tree (film_tree8) when nslots == 8. Slots outside
// slot_mask hold no sample of the render: they are zero, not read (a sum
// that starts at +0 never becomes -0, so adding their +0 changes nothing).
template <int N>
__global__ void k_film_gather(const float4 *contrib, float4 *film, uint32_t W, uint32_t y0, uint32_t y1,
                              uint32_t nslots, uint32_t slot_mask) {
  constexpr int D = 2 * N + 1, K = D * D;
  const uint32_t FW = W + 2 * N, FH = (y1 - y0) + 2 * N;
  const size_t P = (size_t)(y1 - y0) * W;  // contrib: [slot][K][band pixels]
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= FW * FH) return;
  const int px = (int)(q % FW) - N, py = (int)(y0 + q / FW) - N;
  V4 sl[8];
  const uint32_t ns = nslots == 8 ? 8u : 1u;
  for (uint32_t k = 0; k < ns; ++k) {
    float r = 0.f, g = 0.f, bl = 0.f, w = 0.f;
    if (ns == 8 && !((slot_mask >> k) & 1u)) {
      sl[k] = V4{r, g, bl, w};
      continue;
    }
#pragma unroll
    for (int dy = 0; dy < D; ++dy)
#pragma unroll
      for (int dx = 0; dx < D; ++dx) {
        const int sxp = px - dx + N, syp = py - dy + N;
        if (sxp < 0 || sxp >= (int)W || syp < (int)y0 || syp >= (int)y1) continue;
        const float4 c = contrib[((size_t)k * K + (size_t)(dy * D + dx)) * P + (size_t)(syp - (int)y0) * W + sxp];
        r = r + c.x;
        g = g + c.y;
        bl = bl + c.z;
        w = w + c.w;
      }
    sl[k] = V4{r, g, bl, w};
  }
  const V4 f = ns == 8 ? film_tree8(sl) : sl[0];
  film[q] = make_float4(f.x, f.y, f.z, f.w);
}

__global__ void k_collect(WaveBuffers b, ChunkParams p, float *L_out, uint8_t *valid_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_paths) return;
  const V3 L = final_L(b, p, i);
  L_out[3 * (size_t)i] = L.x;
  L_out[3 * (size_t)i + 1] = L.y;
  L_out[3 * (size_t)i + 2] = L.z;
  const uint32_t flags = b.misc[kFinal][i].w >> 16;
  uint8_t v = 1;
  if (p.integrator == MTX_INT_PATH_MIS) v = (flags & PF_VALID_RAY) ? 1 : 0;
  if (p.integrator == MTX_INT_NRC) v = (flags & PF_PRIMARY_VALID) ? 1 : 0;
  if (p.integrator == MTX_INT_SIMPLE) v = (b.misc[kFinal][i].w & 0xffffu) != 0 ? 1 : 0;  // simple.py:118
  valid_out[i] = v;
}

// block.put(pos, L / cw) at the integer pixel position (:161-165), running
// accumulation per source pixel: iteration, then chain order.
template <int N, uint32_t F>
__global__ __launch_bounds__(film_max_block(N)) void k_mlt_film(WaveBuffers b, ChunkParams p, float4 *contrib) {
  constexpr int K = film_taps(N);
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.n_px) return;
  const uint32_t pix = p.px0 + q;
  const int y = (int)(pix / p.width), x = (int)(pix - (uint32_t)y * p.width);
  const size_t o = (size_t)(pix - p.band_y0 * p.width);  // contrib: K planes of band_px
  float4 acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = contrib[(size_t)k * p.band_px + o];
  for (uint32_t sidx = 0; sidx < p.spp; ++sidx) {
    const uint32_t c = q * p.spp + sidx;
    const float4 lc = b.mlt_L[c];
    const float cw = b.mlt_cur[c].z;
    const V3 res = V3{lc.x, lc.y, lc.z} / cw;
    film_accumulate<N, F>(acc, x, y, make_float2((float)x, (float)y), res);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) contrib[(size_t)k * p.band_px + o] = acc[k];
}

// p.rfilter picks the instantiation (film_dev.h with_rfilter).
void launch_mlt_film(const WaveBuffers &b, const ChunkParams &p, float4 *contrib, hipStream_t st) {
  with_rfilter(p.rfilter, [&](auto N, auto F) {
    hipLaunchKernelGGL((k_mlt_film<decltype(N)::value, decltype(F)::value>), dim3(blocks_for(p.n_px, 128)), dim3(128),
                       0, st, b, p, contrib);
  });
}
void launch_film_src(const WaveBuffers &b, const ChunkParams &p, float4 *contrib, hipStream_t st) {
  with_rfilter(p.rfilter, [&](auto N, auto F) {
    constexpr int n = decltype(N)::value;
    constexpr uint32_t f = decltype(F)::value;
    if (p.spp < 4)
      hipLaunchKernelGGL((k_film_src<n, f>), dim3(blocks_for(p.n_px, 128)), dim3(128), 0, st, b, p, contrib);
    else
      hipLaunchKernelGGL((k_film_src_staged<n, f>), dim3(blocks_for(p.n_px, 64)), dim3(64), 0, st, b, p, contrib);
  });
}
void launch_film_gather(const float4 *contrib, float4 *film, uint32_t width, uint32_t y0, uint32_t y1,
                        uint32_t nslots, uint32_t slot_mask, uint32_t rfilter, hipStream_t st) {
  const uint32_t nb = rfilter_reach(rfilter);
  const uint64_t n = (uint64_t)(width + 2 * nb) * (y1 - y0 + 2 * nb);
  const dim3 grid(blocks_for(n, 256)), block(256);
  with_rfilter(rfilter, [&](auto N, auto) {
    hipLaunchKernelGGL(k_film_gather<decltype(N)::value>, grid, block, 0, st, contrib, film, width, y0, y1, nslots,
                       slot_mask);
  });
}
void launch_collect(const WaveBuffers &b, const ChunkParams &p, float *L_out, uint8_t *valid_out, hipStream_t st) {
  hipLaunchKernelGGL(k_collect, dim3(blocks_for(p.n_paths, 256)), dim3(256), 0, st, b, p, L_out, valid_out);
}

}  // namespace mtxd
