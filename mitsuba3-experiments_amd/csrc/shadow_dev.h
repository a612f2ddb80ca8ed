// shadow_dev.h — the NEE shadow record as it lies in memory: its word
// groups, its two forms and how a record changes its path's L. Shared by the
// any-hit kernel that applies the records (trace.hip ShadowSrc) and the shade
// code that builds them (shade_dev.h make_shadow, shade.hip shade_loop).
#pragma once
#include "device_common.h"

namespace mtxd {

// A shadow record's contribution to its path's L (T, X and flags of
// make_shadow): fma(T, X, L) or L + X when the ray is unoccluded, the
// flagged channels NaN when it is occluded.
__device__ __forceinline__ void apply_shadow(float4 &L, float4 rt, float4 rx, bool occluded) {
  const uint32_t fl = __float_as_uint(rt.w);
  if (!occluded) {
    if (fl & 1u) {
      L.x = fmaf(rt.x, rx.x, L.x);
      L.y = fmaf(rt.y, rx.y, L.y);
      L.z = fmaf(rt.z, rx.z, L.z);
    } else {
      L.x = L.x + rx.x;
      L.y = L.y + rx.y;
      L.z = L.z + rx.z;
    }
  } else {
    const float qnan = __uint_as_float(0x7fc00000u);
    if (fl & 2u) L.x = qnan;
    if (fl & 4u) L.y = qnan;
    if (fl & 8u) L.z = qnan;
  }
}

// The records lie as planes of word groups (wavefront.h). k_shade stores each record of the integrators whose L
// it stores itself (path-mis, path, nrc, pssmltpath) in its final-value form
// (make_shadow with Lcur, flag kShadowFinal): t = the path's L after an
// unoccluded ray (fma(T, X, L), path-mis.py:117, or L + X, path.py:259 /
// nrc.py:62) with the flags in t.w, and no x: the record's target already
// holds the L before the ray, L.w included (k_shade stored it there in the
// same launch that wrote the record). The unoccluded finish stores t.xyz
// alone (12 B, no read of L, L.w stays); the occluded one does nothing unless
// a flagged channel must become NaN (then it reads L from the target). The x
// plane is the read-modify-write form's (the nerad integrators).
constexpr uint32_t kShadowFinal = 16u;  // record flag: final-value form
// Word group g (0 o, 1 d | L index, 2 t | flags, 3 x) of record k:
__device__ __forceinline__ float4 *shadow_word(const WaveBuffers &b, uint32_t g, uint32_t k) {
  return b.shadow + ((size_t)g * b.capacity + k);
}

}  // namespace mtxd
