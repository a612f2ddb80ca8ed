// mtx_core/discrete.h — Mitsuba's DiscreteDistribution and the uniform
// triangle warp, shared by the neural radiosity surface sampler (nerad.h) and
// the mesh area emitter (interaction.h).
//   Upstream pieces restated (Mitsuba 3 core, unverifiable offline; parity
//   unpinned): DiscreteDistribution::sample / sample_reuse (cdf accumulated
//   in double, stored as float; search restricted to the non-zero range),
//   warp::square_to_uniform_triangle.
#pragma once
#include "common.h"

namespace mtx {

// One DiscreteDistribution: pmf[n], cdf[n] (inclusive prefix, double-
// accumulated, stored as float), sum = cdf[n-1], normalization = 1/sum, and
// the first / last index with a non-zero pmf (upstream m_valid).
struct DiscreteDist {
  const float *pmf, *cdf;
  uint32_t n, valid_lo, valid_hi;
  float sum, normalization;
};

// DiscreteDistribution::sample: the first index in [valid_lo, valid_hi]
// whose cdf is not below u * sum.
MTX_HD uint32_t discrete_sample(const DiscreteDist &d, float u) {
  const float value = u * d.sum;
  uint32_t lo = d.valid_lo, hi = d.valid_hi;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (d.cdf[mid] < value)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The same index as discrete_sample for a non-decreasing cdf (the lower bound
// of a monotone predicate is unique), found without data-dependent exits: the
// bisection runs bit_length(valid_hi - valid_lo) steps -- each step at least
// halves hi - lo -- and a step on a closed interval changes nothing. Lanes of
// a wave that search the same distribution run the same trip count whatever
// their u, and a step is one load, one compare and two selects.
MTX_HD uint32_t discrete_sample_fixed(const DiscreteDist &d, float u) {
  const float value = u * d.sum;
  uint32_t lo = d.valid_lo, hi = d.valid_hi;
  const uint32_t span = hi - lo;
  const int steps = span ? 32 - __builtin_clz(span) : 0;
  for (int k = 0; k < steps; ++k) {
    const uint32_t mid = (lo + hi) >> 1;  // in [lo, hi]: always a valid entry
    const bool below = d.cdf[mid] < value && lo < hi;
    lo = below ? mid + 1 : lo;
    hi = below ? hi : mid;
  }
  return lo;
}

// DiscreteDistribution::sample_reuse: index and the sample rescaled to
// [0, 1) inside the chosen interval.
MTX_HD float discrete_reuse(const DiscreteDist &d, uint32_t i, float u) {
  const float pmf = d.pmf[i] * d.normalization;
  const float cdf = i > 0 ? d.cdf[i - 1] * d.normalization : 0.f;
  return (u - cdf) / pmf;
}
MTX_HD uint32_t discrete_sample_reuse(const DiscreteDist &d, float u, float *u_out) {
  const uint32_t i = discrete_sample(d, u);
  *u_out = discrete_reuse(d, i, u);
  return i;
}
MTX_HD uint32_t discrete_sample_reuse_fixed(const DiscreteDist &d, float u, float *u_out) {
  const uint32_t i = discrete_sample_fixed(d, u);
  *u_out = discrete_reuse(d, i, u);
  return i;
}

// The pmf entry of a mesh emitter's triangle: Mesh::face_area, half the norm
// of the edge cross product in fp32. The loader (scene.py _tri_area_f32) and
// the device's table rebuild (refit.hip) both follow this sequence.
MTX_HD float tri_area(V3 p0, V3 p1, V3 p2) { return norm(cross(p1 - p0, p2 - p0)) * 0.5f; }

// When the order of a double-precision prefix sum over n fp32 areas cannot
// matter. max_bits / min_bits: the bit patterns of the largest area and of the
// smallest non-zero one (both finite and positive). With M = ilogb(largest)
// (a denormal counts as -126, which only enlarges the bound) and m =
// max(ilogb(smallest), -126) - 23 the exponent of the smallest area's last
// mantissa bit, every area is a multiple of 2^m (a larger fp32 value has a
// last bit at least as high) and below 2^(M+1), so every partial sum of every
// subset is a non-negative multiple of 2^m below n 2^(M+1) <=
// 2^(M+1+ceil(log2 n)). Such a number has at most M + 1 + ceil(log2 n) - m
// significant bits; if that is <= 53 it is a double, no addition in any
// association rounds, and every scan order gives the sequential result.
MTX_HD bool prefix_order_free(uint32_t max_bits, uint32_t min_bits, uint32_t n) {
  const int eM = (int)(max_bits >> 23), em = (int)(min_bits >> 23);
  const int M = (eM > 1 ? eM : 1) - 127, m = (em > 1 ? em : 1) - 127 - 23;
  const int lg = n > 1 ? 32 - __builtin_clz(n - 1) : 0;
  return M + 1 + lg - m <= 53;
}

MTX_HD V2 square_to_uniform_triangle(V2 s) {
  const float t = safe_sqrt(1.f - s.x);
  return V2{1.f - t, t * s.y};
}

}  // namespace mtx
