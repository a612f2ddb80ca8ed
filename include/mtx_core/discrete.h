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

MTX_HD V2 square_to_uniform_triangle(V2 s) {
  const float t = safe_sqrt(1.f - s.x);
  return V2{1.f - t, t * s.y};
}

}  // namespace mtx
