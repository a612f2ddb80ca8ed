// mtx_core/refit.h — refit of the two BVHs of mtx.h after a vertex update:
// topology, leaf order and slot order stay, only the quantised child boxes
// are recomputed bottom-up. Compiled for the host (mtx_bvh_refit,
// mtx_bvh_refit_occlusion in bvh_build.cpp) and for the device (refit.hip), so
// both produce the same words; with unchanged vertices those are the
// builder's own (the builder quantises through the same geometry.h functions).
//
// Box definitions, as in the builder:
//   closest-hit tree: a triangle's box is that of its three exact vertices,
//     extent = largest |coordinate| over the referenced vertices;
//   occlusion tree: a triangle's box is that of v0, v0 + e1, v0 + e2 (fp32) of
//     its record, extent = largest |coordinate| over those points;
//   a child's box = pad_bounds(exact union of its triangles' boxes); the
//     node's frame is the union of its children's padded boxes.
// Boxes are 6 floats: lo.xyz, hi.xyz. A node's own (unpadded) union is stored
// for its parent.
#pragma once
#include "geometry.h"

namespace mtx {

// kRefitMaxCoord (1 + 2^-20): the bound on v0 + e of a record whose vertices
// obey kRefitMaxCoord (e = fl(v1 - v0) and the sum round once each).
constexpr float kRefitMaxPoint = 137439084544.f;  // 2^37 + 2^17

MTX_HD void box_reset(float *b) {
  b[0] = b[1] = b[2] = kInf;
  b[3] = b[4] = b[5] = -kInf;
}
// std::min / std::max of the builder's Box::grow
MTX_HD void box_grow_point(float *b, const float *p) {
  for (int a = 0; a < 3; ++a) {
    b[a] = p[a] < b[a] ? p[a] : b[a];
    b[3 + a] = b[3 + a] < p[a] ? p[a] : b[3 + a];
  }
}
MTX_HD void box_grow(float *b, const float *o) {
  for (int a = 0; a < 3; ++a) {
    b[a] = o[a] < b[a] ? o[a] : b[a];
    b[3 + a] = b[3 + a] < o[3 + a] ? o[3 + a] : b[3 + a];
  }
}

// |x| as its bit pattern: an order-preserving key for finite x >= 0, so the
// maximum over any order of visits is the same word.
MTX_HD uint32_t abs_bits(float x) { return f2u(x) & 0x7fffffffu; }

// The {v0, e1, e2} record of a triangle (the builder's tri_geom arithmetic).
MTX_HD void tri_record(const float *p0, const float *p1, const float *p2, float *v0, float *e1, float *e2) {
  for (int a = 0; a < 3; ++a) {
    v0[a] = p0[a];
    e1[a] = p1[a] - p0[a];
    e2[a] = p2[a] - p0[a];
  }
}

// The three points the occlusion tree takes a record's box from.
MTX_HD void occ_points(const float *v0, const float *e1, const float *e2, float pts[9]) {
  for (int a = 0; a < 3; ++a) {
    pts[a] = v0[a];
    pts[3 + a] = v0[a] + e1[a];
    pts[6 + a] = v0[a] + e2[a];
  }
}

// Re-quantise closest-hit node W (16 words) in place from its children's
// boxes: tbox per leaf-order triangle, nbox per node (the children's, written
// by the deeper levels). Child refs, the child count and the bytes of unused
// slots stay. self_out: the node's unpadded union. False: a bound could not be
// quantised (cannot happen for coordinates within kRefitMaxCoord).
MTX_HD bool refit_node4(int32_t *W, const float *tbox, const float *nbox, float extent, float *self_out) {
  const uint32_t w3 = (uint32_t)W[3];
  const int nch = (int)(w3 >> 24);
  float cb[4][6], u[6], self[6];
  box_reset(u);
  box_reset(self);
  for (int k = 0; k < 4; ++k) {
    if (k >= nch) break;
    const int32_t ref = W[4 + k];
    box_reset(cb[k]);
    if (ref >= 0) {
      box_grow(cb[k], nbox + 6 * (size_t)ref);
    } else {
      uint32_t first, cnt;
      leaf_decode(ref, &first, &cnt);
      for (uint32_t t = 0; t < cnt; ++t) box_grow(cb[k], tbox + 6 * (size_t)(first + t));
    }
    box_grow(self, cb[k]);
    for (int a = 0; a < 3; ++a) pad_bounds(&cb[k][a], &cb[k][3 + a], extent);
    box_grow(u, cb[k]);
  }
  bool ok = true;
  uint32_t eb = 0;
  for (int a = 0; a < 3; ++a) {
    const float org = u[a];
    const int e = quantise_exponent(org, u[3 + a]);
    uint32_t wl = (uint32_t)W[8 + 2 * a], wh = (uint32_t)W[9 + 2 * a];
    for (int k = 0; k < 4; ++k) {
      if (k >= nch) break;
      uint32_t qlo, qhi;
      ok = quantise_bounds(org, e, cb[k][a], cb[k][3 + a], &qlo, &qhi) && ok;
      wl = (wl & ~(255u << (8 * k))) | (qlo << (8 * k));
      wh = (wh & ~(255u << (8 * k))) | (qhi << (8 * k));
    }
    W[a] = (int32_t)f2u(org);
    W[8 + 2 * a] = (int32_t)wl;
    W[9 + 2 * a] = (int32_t)wh;
    eb |= (uint32_t)(e & 255) << (8 * a);
  }
  W[3] = (int32_t)((w3 & 0xff000000u) | eb);
  for (int j = 0; j < 6; ++j) self_out[j] = self[j];
  return ok;
}

// The same for occlusion node W (20 words): imask, child_base, tri_base, meta
// and the bytes of empty slots (q_lo 255, q_hi 0) stay.
MTX_HD bool refit_node8(uint32_t *W, const float *tbox, const float *nbox, float extent, float *self_out) {
  const uint32_t w3 = W[3], imask = w3 >> 24, child_base = W[4], tri_base = W[5];
  float cb[8][6], u[6], self[6];
  uint32_t used = 0, inner = 0;
  box_reset(u);
  box_reset(self);
  for (int sl = 0; sl < 8; ++sl) {
    const uint32_t m = (W[6 + (sl >> 2)] >> (8 * (sl & 3))) & 255u;
    box_reset(cb[sl]);
    if ((imask >> sl) & 1u) {
      box_grow(cb[sl], nbox + 6 * (size_t)(child_base + inner++));
    } else if (m != 0u) {
      const uint32_t cnt = (uint32_t)popc32(m >> 5), first = tri_base + (m & 31u);
      for (uint32_t t = 0; t < cnt; ++t) box_grow(cb[sl], tbox + 6 * (size_t)(first + t));
    } else {
      continue;
    }
    used |= 1u << sl;
    box_grow(self, cb[sl]);
    for (int a = 0; a < 3; ++a) pad_bounds(&cb[sl][a], &cb[sl][3 + a], extent);
    box_grow(u, cb[sl]);
  }
  bool ok = true;
  uint32_t eb = 0;
  for (int a = 0; a < 3; ++a) {
    const float org = u[a];
    const int e = quantise_exponent(org, u[3 + a]);
    uint32_t q[4] = {W[8 + 4 * a], W[9 + 4 * a], W[10 + 4 * a], W[11 + 4 * a]};  // lo, lo, hi, hi
    for (int sl = 0; sl < 8; ++sl) {
      if (!((used >> sl) & 1u)) continue;
      uint32_t qlo, qhi;
      ok = quantise_bounds(org, e, cb[sl][a], cb[sl][3 + a], &qlo, &qhi) && ok;
      const int wd = sl >> 2, sh = 8 * (sl & 3);
      q[wd] = (q[wd] & ~(255u << sh)) | (qlo << sh);
      q[2 + wd] = (q[2 + wd] & ~(255u << sh)) | (qhi << sh);
    }
    W[a] = f2u(org);
    for (int j = 0; j < 4; ++j) W[8 + 4 * a + j] = q[j];
    eb |= (uint32_t)(e & 255) << (8 * a);
  }
  W[3] = (w3 & 0xff000000u) | eb;
  for (int j = 0; j < 6; ++j) self_out[j] = self[j];
  return ok;
}

}  // namespace mtx
