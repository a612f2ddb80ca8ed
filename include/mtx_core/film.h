// mtx_core/film.h — reconstruction filters of the film splat
// (ImageBlock.put, path.py:101), shared by the HIP film kernels and the host.
//
// A sample at film position pos lands in the (2n+1)^2 pixels around its
// source pixel, n = rfilter_reach(f); pixel p gets the separable weight
// rfilter_eval(f, r.x) * rfilter_eval(f, r.y) with r = pos - (float(p) + 0.5f).
// The film border equals the reach: a raw film of `rows` rows is
// (rows + 2n) x (W + 2n) x 4.
//
//   tent      radius 1, n = 1:  max(0, 1 - |r|)   (the default; id 0)
//   box       n = 0: Mitsuba's ImageBlock treats a box filter as "no filter":
//             the sample goes to the pixel that holds it with weight 1, no
//             border. As a function of r that is 1 for |r| <= 0.5 (closed: a
//             jittered position that rounds up to the next integer still
//             belongs to its source pixel).
//   gaussian  Mitsuba's: stddev 0.5, radius 4 sigma = 2, n = 2:
//             max(0, exp(-2 r^2) - exp(-8)), exp = mtx::dexp.
//
// Upstream details restated here that cannot be verified offline (no Mitsuba
// source or build on the development machines):
//   * exact evaluation: upstream's ImageBlock reads the filter from a
//     discretised table (ReconstructionFilter::eval_discretized); we evaluate
//     the closed form at the exact offset, so weights differ from upstream's
//     by the table's resolution.
//   * footprint: upstream's coalesced put covers n = ceil(radius - 0.5)
//     pixels to each side of floor(pos) (1 for the tent, 2 for the gaussian);
//     taps whose weight is 0 at the actual offset contribute +0.
//   * normalize = false: weights are not renormalised per sample; the weight
//     sum goes to the film's fourth channel and develop() divides by it.
#pragma once
#include "common.h"
#include "dmath.h"

#ifndef MTX_RFILTER_TENT
#define MTX_RFILTER_TENT 0u
#define MTX_RFILTER_BOX 1u
#define MTX_RFILTER_GAUSSIAN 2u
#endif

namespace mtx {

constexpr uint32_t kRfilterCount = 3;

// Pixels to each side of the source pixel that a sample reaches (= the film
// border); unknown ids: 0xffffffff.
MTX_HD constexpr uint32_t rfilter_reach(uint32_t f) {
  return f == MTX_RFILTER_TENT ? 1u : f == MTX_RFILTER_BOX ? 0u : f == MTX_RFILTER_GAUSSIAN ? 2u : 0xffffffffu;
}
MTX_HD constexpr float rfilter_radius(uint32_t f) {
  return f == MTX_RFILTER_TENT ? 1.f : f == MTX_RFILTER_BOX ? 0.5f : f == MTX_RFILTER_GAUSSIAN ? 2.f : 0.f;
}

constexpr float kGaussAlpha = -2.f;  // -1 / (2 stddev^2), stddev = 0.5

// One axis of the separable filter at offset r from the pixel centre.
MTX_HD float rfilter_eval(uint32_t f, float r) {
  if (f == MTX_RFILTER_BOX) return fabsf(r) <= 0.5f ? 1.f : 0.f;
  if (f == MTX_RFILTER_GAUSSIAN) {
    const float bias = dexp(kGaussAlpha * 4.f);  // the value at the radius, 2^2 = 4
    return fmaxf(0.f, dexp(kGaussAlpha * (r * r)) - bias);
  }
  return fmaxf(0.f, 1.f - fabsf(r));
}

}  // namespace mtx
