// film_dev.h — the film splat of one sample, shared by the film source
// kernels of the fixed integrators (film.hip) and by the building blocks'
// film put (blocks.hip): the same operation sequence, so the same bits.
#pragma once
#include "device_common.h"
#include "mtx_core/film.h"

namespace mtxd {

constexpr int film_taps(int N) { return (2 * N + 1) * (2 * N + 1); }
// Block-size bound of the per-pixel kernels launched with 128 threads: the
// gaussian's 25 float4 accumulators need more than the 128 VGPRs the default
// bound (1024 threads) leaves a lane; the tent and the box keep the default.
constexpr int film_max_block(int N) { return N == 2 ? 128 : 1024; }

// Host: f(N, F) with the reach and the id of the runtime filter `rfilter` as
// std::integral_constant values, the <N, F> of the film kernels (unknown ids
// were refused before any launch; the tent is the default).
template <class Fn>
inline void with_rfilter(uint32_t rfilter, Fn &&f) {
  if (rfilter == MTX_RFILTER_BOX)
    f(std::integral_constant<int, 0>{}, std::integral_constant<uint32_t, MTX_RFILTER_BOX>{});
  else if (rfilter == MTX_RFILTER_GAUSSIAN)
    f(std::integral_constant<int, 2>{}, std::integral_constant<uint32_t, MTX_RFILTER_GAUSSIAN>{});
  else
    f(std::integral_constant<int, 1>{}, std::integral_constant<uint32_t, MTX_RFILTER_TENT>{});
}

template <int N, uint32_t F>
__device__ __forceinline__ void film_accumulate(float4 *acc, int x, int y, float2 ps, V3 L) {
  constexpr int D = 2 * N + 1;
  float wxs[D];
#pragma unroll
  for (int dx = 0; dx < D; ++dx) wxs[dx] = rfilter_eval(F, ps.x - ((float)(x + dx - N) + 0.5f));
#pragma unroll
  for (int dy = 0; dy < D; ++dy) {
    const float wy = rfilter_eval(F, ps.y - ((float)(y + dy - N) + 0.5f));
#pragma unroll
    for (int dx = 0; dx < D; ++dx) {
      const float w = wxs[dx] * wy;
      float4 &c = acc[dy * D + dx];
      c.x = c.x + L.x * w;
      c.y = c.y + L.y * w;
      c.z = c.z + L.z * w;
      c.w = c.w + w;
    }
  }
}

}  // namespace mtxd
