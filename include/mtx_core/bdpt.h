// mtx_core/bdpt.h — connecting a camera subpath and a light subpath: the
// contribution of a strategy (s, t) and its multiple-importance weight
// (Veach 1997, ch. 10; the power heuristic with exponent 2). Per-lane
// functions shared by k_blk_bdpt_connect (blocks.hip) and its host twin
// mtx_blocks_bdpt_host (blocks_entry.cpp).
//
// A vertex store (mtx_path_planes, mtx.h) holds one subpath per lane, every
// plane coalesced over lanes: vertex k, component c of lane i of n lies at
// [(k * C + c) * n + i].
//
// Camera subpath z_0 .. z_{t-1}: z_0 is the pinhole (p = the camera origin,
//   material = -1), z_1 the first hit. beta[0] = beta[1] = 1, beta[k+1] =
//   beta[k] * (BSDF sample weight at z_k).
// Light subpath y_0 .. y_{s-1}: y_0 is the emitter point (EmitterSample.p / n,
//   `emitter` set), beta[0] = radiance / pdf_pos with pdf_pos = inv_area /
//   emitter_count, beta[1] = the weight of sample_emitter_ray, beta[k+1] =
//   beta[k] * (BSDF sample weight at y_k) * the adjoint corrections of the
//   particle tracer (the shading-normal ratio and its mask; eta^2 undone on a
//   transmitted delta sample).
// pdf_fwd[k]: the density per unit area with which vertex k was generated
//   from vertex k-1: solid-angle pdf * |cos at k, geometric normal| / d^2;
//   pdf_pos for y_0, cos / pi as the direction pdf of y_1; z_0 and z_1 are
//   never read.
// pdf_rev[k]: the density with which vertex k would have been generated from
//   vertex k+1 (evaluated at k+1 with its wi / wo exchanged). The entries of
//   the last two vertices of a strategy's subpath depend on the connection
//   and are evaluated here; the stored ones are read for k <= len - 3.
// delta[k]: the lobe sampled at vertex k was in BF_DELTA (the null lobe of a
//   mask included). A vertex is connectable if bsdf_flags(material) & BF_SMOOTH.
//
// Strategy (s, t) joins y_{s-1} and z_{t-1}; only t >= 2 (t = 1 would splat
// onto the film and is no competitor in the weights). s = 0: z_{t-1} lies on
// an area emitter and emitter_eval faces z_{t-2}; s = 1: the connection to the
// emitter point y_0; s >= 2: surface to surface. A path of s + t vertices has
// s + t - 1 segments, which max_depth bounds.
//   C_{s,t} = beta_z[t-1] * f_z * V / d^2 * f_y * beta_y[s-1]
// with f_z, f_y from bsdf_eval_pdf (the value includes the cosine at its own
// vertex), f_y times the shading-normal correction of the adjoint BSDF;
// s = 1: f_y * beta_y[0] -> beta_y[0] * cos_y on the emitter's front side;
// s = 0: C = beta_z[t-1] * Le. Either end not connectable: 0.
//
// Weight: with the vertices of the full path numbered from the light,
// v_0 .. v_{n-1}, n = s + t, let L_i be the area density of v_i generated from
// v_{i-1} (the light's side) and C_i that of v_i generated from v_{i+1} (the
// camera's side). The path density of strategy s' is prod_{i < s'} L_i *
// prod_{i >= s'} C_i, so p_{s'+1} / p_{s'} = L_{s'} / C_{s'}: the walk starts
// at the connection edge with ratio 1 and multiplies outwards, reading the
// planes (no per-lane arrays). A zero density, and one that belongs to a
// delta lobe, counts as 1 in a ratio; a hypothetical strategy s', which would
// connect v_{s'-1} and v_{s'}, adds its squared ratio only if neither is a
// delta vertex. w = 1 / (1 + the sum).
#pragma once
#include "interaction.h"

namespace mtx {

// One lane of a vertex store.
struct PathLane {
  const mtx_path_planes *pl;
  size_t n, i;   // lanes of the store, this lane
  uint32_t len;  // vertices recorded, clamped to the store's depth
};

MTX_HD PathLane path_lane(const mtx_path_planes *pl, size_t n, size_t i) {
  PathLane q;
  q.pl = pl;
  q.n = n;
  q.i = i;
  const int32_t l = pl->len[i];
  q.len = l < 0 ? 0u : ((uint32_t)l > pl->depth ? pl->depth : (uint32_t)l);
  return q;
}
MTX_HD float path_f1(const float *a, const PathLane &q, uint32_t k) { return a[(size_t)k * q.n + q.i]; }
MTX_HD V2 path_f2(const float *a, const PathLane &q, uint32_t k) {
  const float *b = a + (size_t)2 * k * q.n + q.i;
  return V2{b[0], b[q.n]};
}
MTX_HD V3 path_f3(const float *a, const PathLane &q, uint32_t k) {
  const float *b = a + (size_t)3 * k * q.n + q.i;
  return V3{b[0], b[q.n], b[2 * q.n]};
}
MTX_HD bool path_delta(const PathLane &q, uint32_t k) { return q.pl->delta[(size_t)k * q.n + q.i] != 0; }
// The material / emitter index of vertex k; one outside the scene's tables is -1.
MTX_HD int32_t path_material(const PathLane &q, uint32_t k, uint32_t n_materials) {
  const int32_t m = q.pl->material[(size_t)k * q.n + q.i];
  return (m < 0 || (uint32_t)m >= n_materials) ? -1 : m;
}
MTX_HD int32_t path_emitter(const PathLane &q, uint32_t k, uint32_t n_emitters) {
  const int32_t e = q.pl->emitter[(size_t)k * q.n + q.i];
  return (e < 0 || (uint32_t)e >= n_emitters) ? -1 : e;
}
// Vertices 0 .. len-1 whose material or emitter index lies outside the tables.
MTX_HD bool path_has_bad_index(const PathLane &q, uint32_t n_materials, uint32_t n_emitters) {
  bool bad = false;
  for (uint32_t k = 0; k < q.len; ++k) {
    const int32_t m = q.pl->material[(size_t)k * q.n + q.i], e = q.pl->emitter[(size_t)k * q.n + q.i];
    bad = bad || (m >= 0 && (uint32_t)m >= n_materials) || (e >= 0 && (uint32_t)e >= n_emitters);
  }
  return bad;
}

MTX_HD float bdpt_remap0(float x) { return x != 0.f ? x : 1.f; }

// solid-angle density -> area density at the point `to` with geometric normal n_to
MTX_HD float bdpt_to_area(float pdf, V3 from, V3 to, V3 n_to) {
  const V3 d = to - from;
  const float d2 = squared_norm(d);
  if (!(d2 > 0.f)) return 0.f;
  const float cosv = absdot(n_to, d / sqrtf(d2));
  return pdf * cosv / d2;
}

// The camera's half of the walk: strategies t' = t-1 .. 2, each connecting
// z_{t'-1} and z_{t'}. rev_last / rev_prev: the light-side densities of
// z_{t-1} and z_{t-2} under this strategy.
MTX_HD float bdpt_walk_camera(const PathLane &z, uint32_t t, float rev_last, float rev_prev) {
  float sum = 0.f, r = 1.f;
  for (uint32_t j = t - 1; j >= 2; --j) {
    float rev;
    if (j == t - 1)
      rev = rev_last;
    else if (j == t - 2)
      rev = rev_prev;
    else
      rev = path_delta(z, j + 1) ? 1.f : path_f1(z.pl->pdf_rev, z, j);
    const bool d_prev = path_delta(z, j - 1);
    const float fwd = d_prev ? 1.f : path_f1(z.pl->pdf_fwd, z, j);
    r *= bdpt_remap0(rev) / bdpt_remap0(fwd);
    const bool d_here = j == t - 1 ? false : path_delta(z, j);
    if (!d_here && !d_prev) sum = fmaf(r, r, sum);
  }
  return sum;
}

// The light's half: strategies s' = s-1 .. 0, each connecting y_{s'-1} and
// y_{s'}. rev_last / rev_prev: the camera-side densities of y_{s-1}, y_{s-2}.
MTX_HD float bdpt_walk_light(const PathLane &y, uint32_t s, float rev_last, float rev_prev) {
  float sum = 0.f, r = 1.f;
  for (uint32_t i = s; i-- > 0;) {
    float rev;
    if (i == s - 1)
      rev = rev_last;
    else if (i + 2 == s)
      rev = rev_prev;
    else
      rev = path_delta(y, i + 1) ? 1.f : path_f1(y.pl->pdf_rev, y, i);
    const bool d_prev = i >= 1 && path_delta(y, i - 1);
    const float fwd = d_prev ? 1.f : path_f1(y.pl->pdf_fwd, y, i);
    r *= bdpt_remap0(rev) / bdpt_remap0(fwd);
    const bool d_here = i == s - 1 ? false : path_delta(y, i);
    if (!d_here && !d_prev) sum = fmaf(r, r, sum);
  }
  return sum;
}

// Strategy (s, t) of one lane: the unoccluded contribution *C and its weight
// *w (1 without `mis`; 0 with a zero contribution). Returns true when the
// contribution is non-zero and crosses a connection edge, whose shadow ray
// spawn_ray_to(z.p, z.n, y.p) is then in *shadow: the caller tests it.
MTX_HD bool bdpt_strategy(const SceneView &sv, uint32_t n_materials, const PathLane &zc, const PathLane &yl, uint32_t s,
                          uint32_t t, bool mis, V3 *C, float *w, Ray *shadow) {
  *C = v3s(0.f);
  *w = 0.f;
  if (t < 2 || t > zc.len || s > yl.len) return false;
  const mtx_path_planes &Z = *zc.pl;
  const uint32_t kz = t - 1;
  const V3 zp = path_f3(Z.p, zc, kz), zn = path_f3(Z.n, zc, kz), zwi = path_f3(Z.wi, zc, kz);
  const V3 beta_z = path_f3(Z.beta, zc, kz);
  const V3 zprev_p = path_f3(Z.p, zc, kz - 1), zprev_n = path_f3(Z.n, zc, kz - 1);
  if (s == 0) {
    const int32_t e = path_emitter(zc, kz, sv.n_emitters);  // area emitters only
    if (e < 0) return false;
    const V3 c = beta_z * emitter_eval(sv, e, zwi);
    if (all_zero(c)) return false;
    *C = c;
    *w = 1.f;
    if (mis && t >= 3) {
      const float pdf_pos = sv.emitters[e].inv_area * (1.f / (float)emitter_count(sv));
      float rev_prev = 0.f;
      if (t >= 4) {
        const V3 d = zprev_p - zp;
        const float cos_e = dot(zn, d * rsqrt_(squared_norm(d)));
        rev_prev = bdpt_to_area(fmaxf(cos_e, 0.f) * kInvPi, zp, zprev_p, zprev_n);
      }
      *w = 1.f / (1.f + bdpt_walk_camera(zc, t, pdf_pos, rev_prev));
    }
    return false;
  }
  const int32_t mz = path_material(zc, kz, n_materials);
  if (mz < 0) return false;
  const mtx_material mat_z = sv.materials[mz];
  if (!(bsdf_flags(mat_z) & BF_SMOOTH)) return false;
  const mtx_path_planes &Y = *yl.pl;
  const uint32_t ky = s - 1;
  const V3 yp = path_f3(Y.p, yl, ky), yn = path_f3(Y.n, yl, ky);
  const V3 beta_y = path_f3(Y.beta, yl, ky);
  const V3 rel = zp - yp;  // from the light's end to the camera's
  const float d2 = squared_norm(rel);
  if (!(d2 > 0.f)) return false;
  const V3 dir = rel / sqrtf(d2);
  const V3 wo_z = to_local(frame_from_normal(path_f3(Z.sh_n, zc, kz)), -dir);
  const V2 zuv = path_f2(Z.uv, zc, kz);
  V3 f_z;
  float pdf_z;  // solid angle: z_{t-1} samples the direction of y_{s-1}
  bsdf_eval_pdf(sv.bsdf, mat_z, zuv, zwi, wo_z, &f_z, &pdf_z);
  V3 fy_beta;
  float pdf_y;  // solid angle: y_{s-1} samples the direction of z_{t-1}
  mtx_material mat_y = mat_z;
  V3 ywi = v3s(0.f), wo_y = v3s(0.f);
  V2 yuv = V2{0.f, 0.f};
  if (s == 1) {
    const float cos_y = dot(yn, dir);
    if (!(cos_y > 0.f)) return false;
    fy_beta = beta_y * cos_y;
    pdf_y = cos_y * kInvPi;
  } else {
    const int32_t my = path_material(yl, ky, n_materials);
    if (my < 0) return false;
    mat_y = sv.materials[my];
    if (!(bsdf_flags(mat_y) & BF_SMOOTH)) return false;
    const Frame fy = frame_from_normal(path_f3(Y.sh_n, yl, ky));
    ywi = path_f3(Y.wi, yl, ky);
    wo_y = to_local(fy, dir);
    yuv = path_f2(Y.uv, yl, ky);
    V3 f_y;
    bsdf_eval_pdf(sv.bsdf, mat_y, yuv, ywi, wo_y, &f_y, &pdf_y);
    // the adjoint BSDF's shading-normal correction (Veach, p. 155), as the particle tracer applies it
    const float wi_g = dot(yn, to_world(fy, ywi)), wo_g = dot(yn, dir);
    if (!(wi_g * ywi.z > 0.f && wo_g * wo_y.z > 0.f)) return false;
    const float corr = fabsf((ywi.z * wo_g) / (wo_y.z * wi_g));
    fy_beta = f_y * corr * beta_y;
  }
  const V3 c = beta_z * f_z * (1.f / d2) * fy_beta;
  if (all_zero(c)) return false;
  *C = c;
  *w = 1.f;
  *shadow = spawn_ray_to(zp, zn, yp);
  if (!mis) return true;
  // the reverse densities of the connection vertices and their predecessors
  const float z_last = pdf_y * absdot(zn, dir) / d2;  // z_{t-1} generated from y_{s-1}
  const float y_last = pdf_z * absdot(yn, dir) / d2;  // y_{s-1} generated from z_{t-1}
  float z_prev = 0.f, y_prev = 0.f;
  if (t >= 4) {
    V3 val;
    float pdf;
    bsdf_eval_pdf(sv.bsdf, mat_z, zuv, wo_z, zwi, &val, &pdf);
    z_prev = bdpt_to_area(pdf, zp, zprev_p, zprev_n);
  }
  if (s >= 2) {
    V3 val;
    float pdf;
    bsdf_eval_pdf(sv.bsdf, mat_y, yuv, wo_y, ywi, &val, &pdf);
    y_prev = bdpt_to_area(pdf, yp, path_f3(Y.p, yl, ky - 1), path_f3(Y.n, yl, ky - 1));
  }
  *w = 1.f / (1.f + bdpt_walk_camera(zc, t, z_last, z_prev) + bdpt_walk_light(yl, s, y_last, y_prev));
  return true;
}

// All strategies of a lane, or one (s, t >= 0): L = sum of w * C over the
// strategies with s + t - 1 <= max_depth whose shadow ray `occluded` does not
// stop. *weight (may be null): the single strategy's.
template <class Occluded>
MTX_HD V3 bdpt_connect(const SceneView &sv, uint32_t n_materials, const PathLane &zc, const PathLane &yl, int s, int t,
                       uint32_t max_depth, bool mis, Occluded &&occluded, float *weight) {
  V3 L = v3s(0.f);
  if (weight) *weight = 0.f;
  V3 c;
  float w;
  Ray sr;
  if (s >= 0) {
    if ((uint32_t)s + (uint32_t)t > max_depth + 1u) return L;
    const bool vis = bdpt_strategy(sv, n_materials, zc, yl, (uint32_t)s, (uint32_t)t, mis, &c, &w, &sr);
    if (weight) *weight = w;
    if (vis && occluded(sr)) return L;
    return c * w;
  }
  for (uint32_t tt = 2; tt <= zc.len && tt <= max_depth + 1u; ++tt) {
    const uint32_t s_max = max_depth + 1u - tt;
    for (uint32_t ss = 0; ss <= yl.len && ss <= s_max; ++ss) {
      const bool vis = bdpt_strategy(sv, n_materials, zc, yl, ss, tt, mis, &c, &w, &sr);
      if (all_zero(c) || (vis && occluded(sr))) continue;
      L = fma3(c, w, L);
    }
  }
  return L;
}

}  // namespace mtx
