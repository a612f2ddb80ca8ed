// shade_dev.h — one bounce of an integrator for one path: the five shade
// bodies (shade_path: path-mis / path / nrc; shade_simple; shade_pssmlt;
// shade_pssmlt_path; shade_nerad), the ShadeIO record they fill and the NEE
// shadow record they build. The wavefront shade loop (shade.hip) stores what a
// body returns; the path megakernels (mega.hip) keep it in registers.
//
// All arithmetic is IEEE fp32 with -ffp-contract=off; the per-lane
// primitives are the shared mtx_core headers, so every lane reproduces the
// CPU restatement in oracle/ bit for bit.
#pragma once
#include "camera_dev.h"
#include "device_common.h"
#include "shadow_dev.h"

namespace mtxd {

// Diagnostic build only (MTX_DIAG_STAMPS=1, tools/shade_stamps.py): s_memtime
// stamps between the phases of a shade step, summed per wave in scalar
// registers and added to g_shade_stamps at the kernel's end. Read shares, not
// the build's run time (cdna_hip_programming.md "In-kernel stamps"). In the
// default build Stamps is empty and the three macros expand to nothing, so
// their call sites are plain statements: MTX_STAMP_BEGIN(st) starts the clock
// at the kernel's top, MTX_STAMP(st, i) ends segment i (the segments are
// numbered in the order a step runs them; tools/shade_stamps.py names them),
// MTX_STAMP_STEP(st) is segment 0's stamp at the loop top and counts the step.
#ifndef MTX_DIAG_STAMPS
#define MTX_DIAG_STAMPS 0
#endif
#if MTX_DIAG_STAMPS
constexpr int kStampSegs = 9;
struct Stamps {
  unsigned long long prev, acc[kStampSegs], steps;
};
#define MTX_STAMP_BEGIN(st) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"((st).prev)::"memory")
#define MTX_STAMP(st, i)                                                                  \
  do {                                                                                    \
    unsigned long long t_;                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");          \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    (st).acc[i] += t_ - (st).prev;                                                        \
    (st).prev = t_;                                                                       \
  } while (0)
#define MTX_STAMP_STEP(st) \
  do {                     \
    ++(st).steps;          \
    MTX_STAMP(st, 0);      \
  } while (0)
#else
struct Stamps {};
#define MTX_STAMP_BEGIN(st) ((void)0)
#define MTX_STAMP(st, i) ((void)0)
#define MTX_STAMP_STEP(st) ((void)0)
#endif

// The shadow record as shade_* builds it in registers (make_shadow); k_shade
// stores its word groups to the planes of WaveBuffers::shadow (shadow_word),
// the megakernels apply it at once (apply_shadow_rec).
struct ShadowRec {
  float4 o;
  float4 d;
  float4 t;
  float4 x;
};

struct ShadeIO {
  ShadowRec rec;
  bool emit;
  bool em_hi;  // the shadow ray's emitter index is odd (block append: even emitters' rays first)
  bool query;  // NRC radiance-cache query at this hit (field.hip)
  float4 qp, qd, qt;
  float4 nro, nrd, nthr, nprev;  // the next ray and state: k_shade stores them at the path's append slot
  float4 nL;                     // result and sampler state: at the append slot, or by path once the path ends
  uint4 nmisc;
  float warm;                    // the next entry's shading-record word (L2 warm-up)
  Stamps st;                     // k_shade's stamps while the shade runs (empty unless MTX_DIAG_STAMPS)
  // before a step: nothing emitted, nothing queried, nothing loaded for the warm-up
  __device__ __forceinline__ void reset() {
    emit = em_hi = query = false;
    warm = 0.f;
  }
};

// Which shadow-record form an integrator's NEE must use (ShadowSrc::finish
// reads it from flag bit 4, kShadowFinal): true where k_shade itself stores
// the path's L at the queue slot / final plane after the bounce, so the L the
// record is built from is final for the bounce and the any-hit finish may
// overwrite L without reading it (final-value form); false where L lives by
// path outside k_shade's stores (the neural-radiosity RHS: k_nerad_apply adds
// to it), so the finish must read-modify-write L. make_shadow<INT> checks the
// choice at compile time: a new integrator that emits shadow rays must be
// listed here (the round-5 nerad regression was this choice made wrongly).
constexpr bool shadow_final_form(int INT) {
  return INT == MTX_INT_PATH || INT == MTX_INT_PATH_MIS || INT == MTX_INT_NRC || INT == MTX_INT_PSSMLT_PATH;
}
constexpr bool shadow_rmw_form(int INT) { return INT == MTX_INT_NERAD_RHS; }

// Builds the shadow record for an NEE contribution. fma_form: value = (T, X)
// applied as fma(T, X, L); otherwise X is added. Xo is the contribution the
// reference forms when the shadow ray is occluded (em_weight = 0). With Lcur
// (the path's L, final for this bounce: the integrators that k_shade stores
// L for add nothing to L after their NEE) the record is built in its
// final-value form (see ShadowSrc; k_shade completes x.w with L.w).
template <int INT, bool FINAL>
__device__ __forceinline__ void make_shadow(ShadeIO &io, const SurfaceInteraction &si, const DirectionSample &ds,
                                            V3 T, V3 X, V3 Xo, bool fma_form, const V3 *Lcur = nullptr) {
  static_assert(FINAL ? shadow_final_form(INT) : shadow_rmw_form(INT),
                "shadow record form does not match where this integrator's L is stored (shadow_final_form)");
  uint32_t fl = fma_form ? 1u : 0u;
  bool vis_noop, occ_noop;
  if (fma_form) {
    fl |= (Xo.x == 0.f && isfinite_(T.x)) ? 0u : 2u;
    fl |= (Xo.y == 0.f && isfinite_(T.y)) ? 0u : 4u;
    fl |= (Xo.z == 0.f && isfinite_(T.z)) ? 0u : 8u;
    vis_noop = X.x == 0.f && X.y == 0.f && X.z == 0.f && isfinite_(T.x) && isfinite_(T.y) && isfinite_(T.z);
  } else {
    fl |= (Xo.x == 0.f) ? 0u : 2u;
    fl |= (Xo.y == 0.f) ? 0u : 4u;
    fl |= (Xo.z == 0.f) ? 0u : 8u;
    vis_noop = X.x == 0.f && X.y == 0.f && X.z == 0.f;
  }
  occ_noop = (fl & 14u) == 0u;
  io.emit = !(vis_noop && occ_noop);
  if (!io.emit) return;
  io.em_hi = (ds.emitter & 1) != 0;
  const Ray sr = spawn_ray_to(si.p, si.n, ds.p);
  io.rec.o = f4(sr.o, sr.maxt);
  io.rec.d = f4(sr.d, 0.f);  // .w: the L index, set by k_shade after its append
  if constexpr (FINAL) {
    float4 lv = make_float4(Lcur->x, Lcur->y, Lcur->z, 0.f);
    apply_shadow(lv, f4(T, __uint_as_float(fl)), f4(X, 0.f), false);
    io.rec.t = make_float4(lv.x, lv.y, lv.z, __uint_as_float(fl | kShadowFinal));
    io.rec.x = make_float4(Lcur->x, Lcur->y, Lcur->z, 0.f);
  } else {
    io.rec.t = f4(T, __uint_as_float(fl));
    io.rec.x = f4(X, 0.f);
  }
}

// A shadow record applied to its path's L in registers (the path megakernels:
// the record of make_shadow, in either form).
__device__ __forceinline__ void apply_shadow_rec(float4 &L, const ShadowRec &rec, bool occluded) {
  const uint32_t fl = __float_as_uint(rec.t.w);
  if (!(fl & kShadowFinal)) {
    apply_shadow(L, rec.t, rec.x, occluded);
  } else if (!occluded) {
    L = make_float4(rec.t.x, rec.t.y, rec.t.z, L.w);
  } else {
    const float qnan = __uint_as_float(0x7fc00000u);
    if (fl & 2u) L.x = qnan;
    if (fl & 4u) L.y = qnan;
    if (fl & 8u) L.z = qnan;
  }
}

// BSDF data for one shading point: the textured colour of the diffuse and
// roughplastic lobes fetched once (and early: its latency overlaps the work
// before the first BSDF call), read by every BSDF call at this point.
__device__ __forceinline__ BsdfData bsdf_at(const SceneView &sv, const mtx_material &mat, V2 uv) {
  BsdfData bd = sv.bsdf;
  if (mat.tex >= 0 && (mat.type == MTX_MAT_DIFFUSE || mat.type == MTX_MAT_ROUGHPLASTIC)) {
    bd.col = texture_eval(sv.bsdf, mat.tex, uv);
    bd.has_col = true;
  }
  return bd;
}
// path-mis: once a path ends, L.w (its prev_bsdf_pdf until then) holds
// valid_ray as 1 / 0 (path-mis.py:155), so the film reads L and pos only,
// not the 16-B misc record for one flag.
__device__ __forceinline__ float end_w(uint32_t flags) { return (flags & PF_VALID_RAY) ? 1.f : 0.f; }
// The BSDF sample of a lane that samples nothing.
__device__ __forceinline__ BSDFSample no_bsdf_sample() {
  BSDFSample bs;
  bs.wo = v3s(0.f);
  bs.pdf = 0.f;
  bs.eta = 0.f;
  bs.type = 0;
  return bs;
}
// CAM: bounce 0 of a cam0 chunk (k_shade_cam; bounce_ is 0): no stored
// raygen, the camera ray and the sampler state of path `path` are derived.
template <int INT, bool CAM = false>
__device__ __forceinline__ bool shade_path(const DevScene &s, const SceneView &sv, const WaveBuffers &b,
                                           const ChunkParams &p, uint32_t bounce_, uint32_t path, uint32_t qi,
                                           const float4 h, ShadeIO &io, const float4 *warm = nullptr) {
  const uint32_t bounce = CAM ? 0u : bounce_;
  const uint32_t rp = (bounce + b.ray_par) & 1u;
  float4 ro, rd;
  uint4 mi;
  constexpr bool cam = CAM;
  if constexpr (CAM) {
    const CamState c = cam_state(s, p, path);
    ro = c.ro;
    rd = c.rd;
    mi = c.mi;
  } else {
    ro = ld_stream<kNtShade>(b.ray_o[rp] + qi);
    rd = ld_stream<kNtShade>(b.ray_d[rp] + qi);
  }
  // bounce 0: the state init_path / k_rs_begin would have stored (not read)
  const float4 th = bounce == 0 ? kInitThr : ld_stream<kNtShade>(b.thr[rp] + qi),
               Lr = bounce == 0 ? kInitL : ld_stream<kNtShade>(b.L[rp] + qi);
  // prev (previous vertex, NRC spread): path-mis / path read it only for the
  // emission MIS of an emitter hit (pdf_emitter_direction is 0 otherwise), so
  // they load it below once the hit's emitter is known
  constexpr bool kPrevOnEmitter = INT == MTX_INT_PATH_MIS || INT == MTX_INT_PATH;
  float4 pv = kInitPrev;
  if (!kPrevOnEmitter && bounce != 0) pv = ld_stream<kNtShade>(b.prev[rp] + qi);
  if (!cam) mi = ld_stream<kNtShade>(b.misc[rp] + qi);
  io.nL = Lr;  // an exit that changes neither keeps them
  io.nmisc = mi;
  Pcg32 rng = ld_rng(mi);
  uint32_t depth = mi.w & 0xffffu, flags = mi.w >> 16;
  V3 T = V3{th.x, th.y, th.z};
  float eta = th.w;
  V3 L = V3{Lr.x, Lr.y, Lr.z};
  float prev_pdf = Lr.w;
  const V3 ray_d = V3{rd.x, rd.y, rd.z};
  const SurfaceInteraction si = compute_si_dev(s, h.x, __float_as_uint(h.y), h.z, h.w, ray_d);
  MTX_STAMP(io.st, 1);
  // the next queue entry's shading record, one word: its line is in L2 when
  // the next iteration reads the record (k_shade)
  if (warm) io.warm = warm->x;
  if (kPrevOnEmitter && bounce != 0 && si.emitter >= 0) pv = b.prev[rp][qi];
  V3 prev_p = V3{pv.x, pv.y, pv.z};
  float spread = pv.w, a0 = rd.w;
  io.emit = false;
  io.query = false;

  // ------------------------------ head ------------------------------------
  bool active_next = true;
  if (INT == MTX_INT_PATH_MIS) {
    // Direct emission with MIS against the previous BSDF sample (:75-86)
    const bool prev_delta = (flags & PF_PREV_DELTA) != 0;
    float em_pdf = 0.f;
    if (!prev_delta && si.emitter >= 0) {
      const V3 rel = si.p - prev_p;
      const float dist = norm(rel);
      em_pdf = pdf_emitter_direction(sv, si.emitter, rel / dist, dist, si.sh.n);
    }
    const float mis_bsdf = mis_weight_b(prev_pdf, em_pdf);
    const V3 le = (prev_pdf > 0.f) ? emitter_eval(sv, si.emitter, si.wi) : v3s(0.f);
    L = fma3v(T, le * mis_bsdf, L);
    active_next = (depth + 1 < p.max_depth) && si.valid;  // :88
  } else if (bounce == 0) {
    if (INT == MTX_INT_PATH) {
      L = L + emitter_eval(sv, si.emitter, si.wi);  // path.py:239
      if (!(depth < p.max_depth)) {                // path.py:235
        io.nL = f4(L, prev_pdf);
        return false;
      }
    } else {  // NRC primary (nrc.py:117-121)
      if (si.valid) flags |= PF_PRIMARY_VALID;
      a0 = squared_norm(V3{ro.x, ro.y, ro.z} - si.p) / (kFourPi * fabsf(si.wi.z));
      spread = 0.f;
    }
  } else {
    if (INT == MTX_INT_NRC && (flags & PF_CACHE_QUERY)) {
      // the segment ended by the spread criterion (nrc.py:70-71): the radiance
      // cache replaces the rest of the path, queried at the next hit with the
      // direction back to the previous vertex (nerad.py:86-106 Field(si))
      if (si.valid) {
        io.query = true;
        io.qp = f4(si.p, 0.f);
        io.qd = make_float4(-ray_d.x, -ray_d.y, -ray_d.z, 0.f);
        io.qt = f4(T, __uint_as_float(path));
      }
      return false;
    }
    // path.py:283-300 / nrc.py:79-100: emission of the BSDF-sampled hit
    const bool bsdf_delta = (flags & PF_PREV_DELTA) != 0;
    float em_pdf = 0.f;
    if (!bsdf_delta && si.emitter >= 0) {
      const V3 rel = si.p - prev_p;
      const float dist = norm(rel);
      em_pdf = pdf_emitter_direction(sv, si.emitter, rel / dist, dist, si.sh.n);
    }
    const float mis_bsdf =
        INT == MTX_INT_PATH ? mis_weight_a(prev_pdf, em_pdf) : mis_weight_b(prev_pdf, em_pdf);
    const V3 le = (prev_pdf > 0.f) ? emitter_eval(sv, si.emitter, si.wi) : v3s(0.f);
    L = L + T * le * mis_bsdf;
    if (INT == MTX_INT_NRC) spread += sqrtf(squared_norm(si.p - prev_p) / (prev_pdf * fabsf(si.wi.z)));
    depth += 1;
  }
  // path.py:235,299-300 / nrc.py:119,272-273: the NRC primary bounce only
  // requires a valid hit (its depth test runs at the end of an iteration).
  const bool head_ok =
      (INT == MTX_INT_NRC && bounce == 0) ? si.valid : (depth < p.max_depth && si.valid);
  if (INT != MTX_INT_PATH_MIS && !head_ok) {
    io.nL = f4(L, prev_pdf);
    if (INT == MTX_INT_NRC) io.nmisc = make_uint4(mi.x, mi.y, mi.z, depth | (flags << 16));
    return false;
  }
  if (INT == MTX_INT_PATH_MIS && p.restir && bounce == 0) {
    // restirgi.py:452-455: x_s, n_s of the secondary ray's first hit
    b.rs_xs[path] = si.valid ? f4(si.p, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    b.rs_ns[path] = si.valid ? f4(si.n, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (INT == MTX_INT_PATH_MIS && !si.valid) {
    // escaped path: nothing after this point is observable (valid_ray,
    // result unchanged; throughput becomes 0 -> inactive) -- except the
    // sampler position, which ReSTIR keeps using (6 draws per iteration)
    io.nL = f4(L, end_w(flags));
    if (p.restir) {
      rng.advance(6);
      io.nmisc = st_rng(rng, depth | (flags << 16));
    }
    return false;
  }

  // ------------------------------ body ------------------------------------
  const mtx_material mat = sv.materials[si.material];
  // before the emitter sample; the NEE eval and the BSDF sample both read it
  const BsdfData bd = bsdf_at(sv, mat, si.uv);
  MTX_STAMP(io.st, 2);
  const bool smooth = (bsdf_flags(mat) & BF_SMOOTH) != 0;
  bool active_em = (INT == MTX_INT_PATH_MIS ? active_next : true) && smooth;
  const V2 u_em = rng.next_2d();
  DirectionSample ds;
  ds.p = v3s(0.f);
  ds.n = v3s(0.f);
  ds.d = v3s(0.f);
  ds.dist = 0.f;
  ds.pdf = 0.f;
  ds.emitter = -1;
  V3 em_weight = v3s(0.f);
  const bool do_nee = (INT == MTX_INT_NRC) ? true : active_em;  // nrc.py:51-53 samples with `active`
  if (do_nee) em_weight = sample_emitter_direction(sv, si.p, u_em, &ds);
  MTX_STAMP(io.st, 3);
  if (INT != MTX_INT_PATH_MIS) active_em = active_em && ds.pdf != 0.f;
  const V3 wo = to_local(si.sh, ds.d);
  const float s1 = rng.next_1d();
  const V2 s2 = rng.next_2d();
  V3 bsdf_val = v3s(0.f);
  float bsdf_pdf = 0.f;
  BSDFSample bs;
  // eval / pdf only feed the NEE contribution (no draws, no side effects)
  if (active_em) bsdf_eval_pdf(bd, mat, si.uv, si.wi, wo, &bsdf_val, &bsdf_pdf);
  const V3 bsdf_weight = bsdf_sample(bd, mat, si.uv, si.wi, s1, s2, &bs);
  MTX_STAMP(io.st, 4);

  if (INT == MTX_INT_PATH_MIS) {
    const float mi_em = mis_weight_b(ds.pdf, bsdf_pdf);
    if (active_em) {
      const V3 X = bsdf_val * em_weight * mi_em;
      const V3 Xo = bsdf_val * v3s(0.f) * mi_em;
      make_shadow<INT, true>(io, si, ds, T, X, Xo, true, &L);
    }
  } else {
    const float mis_em = INT == MTX_INT_PATH ? mis_weight_a(ds.pdf, bsdf_pdf) : mis_weight_b(ds.pdf, bsdf_pdf);
    if (active_em) {
      const V3 P = T * bsdf_val * em_weight * mis_em;
      const V3 Po = T * bsdf_val * v3s(0.f) * mis_em;
      make_shadow<INT, true>(io, si, ds, T, P, Po, false, &L);
    }
  }

  bool active;
  const Ray nray = spawn_ray(si.p, si.n, to_world(si.sh, bs.wo));
  if (INT == MTX_INT_PATH_MIS) {
    T = T * bsdf_weight;
    eta *= bs.eta;
    if (!(bs.type & BF_NULL)) flags |= PF_VALID_RAY;  // :129-133 (active & si.valid hold here)
    prev_p = si.p;
    prev_pdf = bs.pdf;
    flags = (bs.type & BF_DELTA) ? (flags | PF_PREV_DELTA) : (flags & ~PF_PREV_DELTA);
    depth += 1;  // :141 (si valid here)
    const float throughput_max = hmax(T);
    const float rr_prop = fminf(throughput_max * sqr(eta), 0.95f);
    const bool rr_active = depth >= p.rr_depth;
    const bool rr_continue = rng.next_1d() < rr_prop;
    if (rr_active) T = T * rcp(rr_prop);
    active = active_next && (!rr_active || rr_continue) && (throughput_max != 0.f);
  } else if (INT == MTX_INT_PATH) {
    T = T * bsdf_weight;  // path.py:263
    eta *= bs.eta;
    const float fmax_ = hmax(T);
    const float rr_prob = fminf(fmax_ * sqr(eta), 0.95f);
    const bool rr_active = depth >= p.rr_depth;
    const bool rr_continue = rng.next_1d() < rr_prob;
    if (rr_active) T = T * rcp(rr_prob);
    active = (fmax_ != 0.f) && (!rr_active || rr_continue);
    prev_p = si.p;
    prev_pdf = bs.pdf;
    flags = (bs.type & BF_DELTA) ? (flags | PF_PREV_DELTA) : (flags & ~PF_PREV_DELTA);
  } else {  // NRC
    T = T * bsdf_weight;
    eta *= bs.eta;
    const float a = sqr(spread);  // nrc.py:70-71
    active = a < p.nrc_c * a0;
    if (!active && p.nrc_cache) {  // trace one more segment to the cache query
      flags |= PF_CACHE_QUERY;
      active = true;
    }
    prev_p = si.p;
    prev_pdf = bs.pdf;
    flags = (bs.type & BF_DELTA) ? (flags | PF_PREV_DELTA) : (flags & ~PF_PREV_DELTA);
  }

  // ray, throughput and previous vertex travel with the queue entry (k_shade
  // stores them at the append slot, coalesced, for continuing paths only);
  // a path that ends is read afterwards through L and misc alone
  io.nro = f4(nray.o, nray.maxt);
  io.nrd = f4(nray.d, a0);
  io.nthr = f4(T, eta);
  io.nprev = f4(prev_p, spread);
  io.nL = f4(L, (INT == MTX_INT_PATH_MIS && !active) ? end_w(flags) : prev_pdf);
  io.nmisc = st_rng(rng, depth | (flags << 16));
  MTX_STAMP(io.st, 5);
  return active;
}

// Dr.Jit clamp(x, lo, hi) = maximum(minimum(x, hi), lo), NaN-ignoring (App. A).
__device__ __forceinline__ float dr_clamp(float x, float lo, float hi) { return fmaxf(fminf(x, hi), lo); }

// pssmltsimple.py:60-131 — one bounce of a PSSMLT proposal: emission without
// MIS (:74), BSDF sample masked by active_next (:84), mutation of the local
// direction against the current path's vertex (:88, mutate :135-142),
// re-evaluation (:93-96), proposed vertex write (:99), spawn, RR. Every
// executed bounce consumes 4 draws: the chain's RNG stream continues across
// the Metropolis iterations.
__device__ __forceinline__ bool shade_pssmlt(const DevScene &s, const SceneView &sv, const WaveBuffers &b,
                                             const ChunkParams &p, uint32_t bounce, uint32_t path, uint32_t qi,
                                             const float4 h, ShadeIO &io) {
  const uint32_t rp = (bounce + b.ray_par) & 1u;
  const float4 rd = b.ray_d[rp][qi], th = b.thr[rp][qi], Lr = b.L[rp][qi];
  const uint4 mi = b.misc[rp][qi];
  Pcg32 rng = ld_rng(mi);
  uint32_t depth = mi.w & 0xffffu;
  const uint32_t flags = mi.w >> 16;
  V3 T = V3{th.x, th.y, th.z};
  float eta = th.w;
  V3 L = V3{Lr.x, Lr.y, Lr.z};
  float prev_pdf = Lr.w;
  const SurfaceInteraction si = compute_si_dev(s, h.x, __float_as_uint(h.y), h.z, h.w, V3{rd.x, rd.y, rd.z});
  const V3 le = (prev_pdf > 0.f) ? emitter_eval(sv, si.emitter, si.wi) : v3s(0.f);
  L = fma3v(T, le, L);
  const bool active_next = (depth + 1 < p.max_depth) && si.valid;
  const float s1 = rng.next_1d();
  const V2 s2 = rng.next_2d();
  BSDFSample bs = no_bsdf_sample();
  V3 w = v3s(0.f);
  mtx_material mat;
  BsdfData bd = sv.bsdf;
  if (si.valid) {
    mat = sv.materials[si.material];
    bd = bsdf_at(sv, mat, si.uv);
    w = bsdf_sample(bd, mat, si.uv, si.wi, s1, s2, &bs);
  }
  if (!active_next) w = v3s(0.f);
  const float4 o4 = b.vpath[(size_t)depth * b.capacity + path];
  const V3 old = V3{o4.x, o4.y, o4.z};
  V3 vwo = p.large_step ? bs.wo : normalize(old * 0.9f + bs.wo * 0.1f);
  V3 val = v3s(0.f);
  float pdf = 0.f;
  if (si.valid) bsdf_eval_pdf(bd, mat, si.uv, si.wi, vwo, &val, &pdf);
  if (pdf <= 0.f) vwo = bs.wo;
  if (pdf > 0.f) w = val / pdf;
  b.vprop[(size_t)depth * b.capacity + path] = f4(vwo, 0.f);
  const Ray nray = spawn_ray(si.p, si.n, to_world(si.sh, vwo));
  T = T * w;
  eta *= bs.eta;
  prev_pdf = bs.pdf;
  if (si.valid) depth += 1;
  const float fmax_ = hmax(T);
  const float rr_prob = fminf(fmax_ * sqr(eta), 0.95f);
  const bool rr_active = depth >= p.rr_depth;
  const bool rr_continue = rng.next_1d() < rr_prob;
  if (rr_active) T = T * rcp(rr_prob);
  const bool active = active_next && (!rr_active || rr_continue) && (fmax_ != 0.f);
  io.nro = f4(nray.o, nray.maxt);
  io.nrd = f4(nray.d, 0.f);
  io.nthr = f4(T, eta);
  io.nL = f4(L, prev_pdf);
  io.nmisc = st_rng(rng, depth | (flags << 16));
  return active;
}

// simple.py:55-113 — one bounce of the BSDF-only path tracer: emission at
// the hit without MIS (:69-70, masked by prev_bsdf_pdf > 0), BSDF sample
// masked by active_next (:79), spawn (:84), depth on a valid hit (:102), RR
// (:104-111). 4 draws per executed bounce. The same loop as
// pssmltsimple.py:60-131 without the mutation; bounce 0 starts from the
// constant initial state (f = 1, eta = 1, L = 0, prev_bsdf_pdf = 1).
template <bool CAM = false>  // CAM: bounce 0 of a cam0 chunk, as in shade_path
__device__ __forceinline__ bool shade_simple(const DevScene &s, const SceneView &sv, const WaveBuffers &b,
                                             const ChunkParams &p, uint32_t bounce_, uint32_t path, uint32_t qi,
                                             const float4 h, ShadeIO &io) {
  const uint32_t bounce = CAM ? 0u : bounce_;
  const uint32_t rp = (bounce + b.ray_par) & 1u;
  float4 rd;
  uint4 mi;
  if constexpr (CAM) {
    const CamState c = cam_state(s, p, path);
    rd = c.rd;
    mi = c.mi;
  } else {
    rd = b.ray_d[rp][qi];
    mi = b.misc[rp][qi];
  }
  const float4 th = bounce == 0 ? kInitThr : b.thr[rp][qi], Lr = bounce == 0 ? kInitL : b.L[rp][qi];
  Pcg32 rng = ld_rng(mi);
  uint32_t depth = mi.w & 0xffffu;
  const uint32_t flags = mi.w >> 16;
  V3 T = V3{th.x, th.y, th.z};
  float eta = th.w;
  V3 L = V3{Lr.x, Lr.y, Lr.z};
  const float prev_pdf = Lr.w;
  const SurfaceInteraction si = compute_si_dev(s, h.x, __float_as_uint(h.y), h.z, h.w, V3{rd.x, rd.y, rd.z});
  const V3 le = (prev_pdf > 0.f) ? emitter_eval(sv, si.emitter, si.wi) : v3s(0.f);
  L = fma3v(T, le, L);
  const bool active_next = (depth + 1 < p.max_depth) && si.valid;
  const float s1 = rng.next_1d();
  const V2 s2 = rng.next_2d();
  BSDFSample bs = no_bsdf_sample();
  V3 w = v3s(0.f);
  if (active_next) w = bsdf_sample(sv.bsdf, sv.materials[si.material], si.uv, si.wi, s1, s2, &bs);
  const Ray nray = spawn_ray(si.p, si.n, to_world(si.sh, bs.wo));
  T = T * w;
  eta *= bs.eta;
  if (si.valid) depth += 1;
  const float fmax_ = hmax(T);
  const float rr_prob = fminf(fmax_ * sqr(eta), 0.95f);
  const bool rr_active = depth >= p.rr_depth;
  const bool rr_continue = rng.next_1d() < rr_prob;
  if (rr_active) T = T * rcp(rr_prob);
  const bool active = active_next && (!rr_active || rr_continue) && (fmax_ != 0.f);
  io.nro = f4(nray.o, nray.maxt);
  io.nrd = f4(nray.d, 0.f);
  io.nthr = f4(T, eta);
  io.nL = f4(L, bs.pdf);
  io.nmisc = st_rng(rng, depth | (flags << 16));
  return active;
}

// pssmltpath.py:17-168 — one bounce of a PSSMLT proposal with NEE + MIS:
// emission at the hit weighted against the previous BSDF sample (:71-82),
// unmasked BSDF sample (:99-101), mutation of the local direction AND of the
// emitter sample against the current path's vertex (:103-105, mutate
// :170-190), re-evaluation (:107-110), NEE from the mutated emitter sample
// (:118-134, shadow ray), proposed vertex write (:138), RR (:154-166).
// Draws per bounce: 1 + 2 (BSDF) + 2 (mutation) + 1 (RR).
__device__ __forceinline__ bool shade_pssmlt_path(const DevScene &s, const SceneView &sv, const WaveBuffers &b,
                                                  const ChunkParams &p, uint32_t bounce, uint32_t path, uint32_t qi,
                                                  const float4 h, ShadeIO &io) {
  const uint32_t rp = (bounce + b.ray_par) & 1u;
  const float4 rd = b.ray_d[rp][qi], th = b.thr[rp][qi], Lr = b.L[rp][qi], pv = b.prev[rp][qi];
  const uint4 mi = b.misc[rp][qi];
  Pcg32 rng = ld_rng(mi);
  uint32_t depth = mi.w & 0xffffu, flags = mi.w >> 16;
  V3 T = V3{th.x, th.y, th.z};
  float eta = th.w;
  V3 L = V3{Lr.x, Lr.y, Lr.z};
  float prev_pdf = Lr.w;
  const V3 prev_p = V3{pv.x, pv.y, pv.z};
  const SurfaceInteraction si = compute_si_dev(s, h.x, __float_as_uint(h.y), h.z, h.w, V3{rd.x, rd.y, rd.z});
  io.emit = false;
  io.query = false;
  // direct emission (:71-82)
  const bool prev_delta = (flags & PF_PREV_DELTA) != 0;
  const V3 rel = si.p - prev_p;
  const float dist = norm(rel);
  const float em_pdf = prev_delta ? 0.f : pdf_emitter_direction(sv, si.emitter, rel / dist, dist, si.sh.n);
  const float mis_bsdf = mis_weight_b(prev_pdf, em_pdf);
  const V3 le = (prev_pdf > 0.f) ? emitter_eval(sv, si.emitter, si.wi) : v3s(0.f);
  L = fma3v(T, le * mis_bsdf, L);
  const bool active_next = (depth + 1 < p.max_depth) && si.valid;  // :84
  // BSDF sampling (:99-101), not masked
  const float s1 = rng.next_1d();
  const V2 s2 = rng.next_2d();
  BSDFSample bs = no_bsdf_sample();
  V3 w = v3s(0.f);
  mtx_material mat;
  BsdfData bd = sv.bsdf;
  if (si.valid) {
    mat = sv.materials[si.material];
    bd = bsdf_at(sv, mat, si.uv);
    w = bsdf_sample(bd, mat, si.uv, si.wi, s1, s2, &bs);
  }
  // mutate (:170-190): a = 0.01 on the direction, sqrt(0.01) on the emitter sample
  const V2 um = rng.next_2d();
  const size_t vi = (size_t)depth * b.capacity + path;
  const float4 o4 = b.vpath[vi];
  const float2 oes = b.vpath_es[vi];
  V3 vwo;
  V2 es;
  if (p.large_step) {
    vwo = bs.wo;
    es = um;
  } else {
    vwo = normalize(V3{o4.x, o4.y, o4.z} * 0.99f + bs.wo * 0.01f);
    const V2 g = square_to_std_normal(um);
    es = V2{dr_clamp(g.x * 0.1f + oes.x, 0.f, 1.f), dr_clamp(g.y * 0.1f + oes.y, 0.f, 1.f)};
  }
  V3 val = v3s(0.f);
  float pdf = 0.f;
  if (si.valid) bsdf_eval_pdf(bd, mat, si.uv, si.wi, vwo, &val, &pdf);  // :107
  if (pdf <= 0.f) vwo = bs.wo;                                                // :109
  if (pdf > 0.f) w = val / pdf;                                               // :110
  const Ray nray = spawn_ray(si.p, si.n, to_world(si.sh, vwo));               // :114
  // emitter sampling from the mutated sample (:118-134)
  const bool active_em = active_next && (bsdf_flags(mat) & BF_SMOOTH) != 0;
  if (active_em) {
    DirectionSample ds;
    const V3 em_weight = sample_emitter_direction(sv, si.p, es, &ds);
    const V3 wo = to_local(si.sh, ds.d);
    V3 ev;
    float epdf;
    bsdf_eval_pdf(bd, mat, si.uv, si.wi, wo, &ev, &epdf);
    const float mi_em = mis_weight_b(ds.pdf, epdf);
    make_shadow<MTX_INT_PSSMLT_PATH, true>(io, si, ds, T, ev * em_weight * mi_em, ev * v3s(0.f) * mi_em, true, &L);
  }
  b.vprop[vi] = f4(vwo, 0.f);  // :138
  b.vprop_es[vi] = make_float2(es.x, es.y);
  T = T * w;
  eta *= bs.eta;
  prev_pdf = bs.pdf;
  flags = (bs.type & BF_DELTA) ? (flags | PF_PREV_DELTA) : (flags & ~PF_PREV_DELTA);
  if (si.valid) depth += 1;  // :154
  const float fmax_ = hmax(T);
  const float rr_prob = fminf(fmax_ * sqr(eta), 0.95f);
  const bool rr_active = depth >= p.rr_depth;
  const bool rr_continue = rng.next_1d() < rr_prob;
  if (rr_active) T = T * rcp(rr_prob);
  const bool active = active_next && (!rr_active || rr_continue) && (fmax_ != 0.f);
  io.nro = f4(nray.o, nray.maxt);
  io.nrd = f4(nray.d, 0.f);
  io.nthr = f4(T, eta);
  io.nL = f4(L, prev_pdf);
  io.nprev = f4(si.p, 0.f);
  io.nmisc = st_rng(rng, depth | (flags << 16));
  return active;
}

// nerad.py:174-233 Integrator.sample_rhs, one lane = one of the M samples of a
// training point (nerad.py:182-184 dr.repeat). Bounce 0 is the sampled
// surface point itself (hit record written by k_nerad_raygen): NEE with a
// visibility test (:197-200, mis_weight of mitsuba.ad.integrators.common =
// variant B) and a BSDF sample (:204-206). Bounce 1 is the BSDF ray's hit:
// f = mis_weight(bs.pdf, emitter pdf) * bsdf_weight (:208-217), then
// next_smooth_si (:124-164) follows delta / null vertices (bounces 2..11,
// f2 in prev.xyz). At the stop vertex: f *= f2, zero if invalid (:219-222);
// a valid vertex becomes a field query (Le kept in prev.xyz), L += f * (Le +
// field) is applied after the field evaluation (k_nerad_apply, :226-229).
// State: thr.xyz = f, L.w = bs.pdf of bounce 0, prev.xyz = si.p (bounce 0)
// then f2, misc.w = chain depth.
// RENDER: Integrator.sample (nerad.py:235-254) -- a camera lane runs
// next_smooth_si from its first hit (bounce 0 = chain start, no NEE), then
// L = Field(si) * f + Le(si) (applied by k_nerad_apply after the field).
template <bool RENDER>
__device__ __forceinline__ bool shade_nerad(const DevScene &s, const SceneView &sv, const WaveBuffers &b,
                                            uint32_t bounce, uint32_t path, uint32_t qi, const float4 h,
                                            ShadeIO &io) {
  const float4 rd = b.ray_d[(bounce + b.ray_par) & 1u][qi];
  // a rendered lane's bounce-0 state is the camera raygen's (nothing stored)
  const float4 Lr = (RENDER && bounce == 0) ? kInitL : b.L[kFinal][path];
  // thr / prev path-indexed in plane 0 (k_nerad_apply reads prev by path)
  const float4 pv = (RENDER && bounce == 0) ? kInitPrev : b.prev[0][path];
  const float4 th = (RENDER && bounce == 0) ? kInitThr : b.thr[0][path];
  // a rendered lane's bounce-0 sampler state is the camera raygen's (queue plane 0, identity)
  const uint4 mi = (RENDER && bounce == 0) ? b.misc[0][path] : b.misc[kFinal][path];
  Pcg32 rng = ld_rng(mi);
  uint32_t depth = mi.w & 0xffffu;
  const V3 ray_d = V3{rd.x, rd.y, rd.z};
  const SurfaceInteraction si = compute_si_dev(s, h.x, __float_as_uint(h.y), h.z, h.w, ray_d);
  io.emit = false;
  io.query = false;
  V3 L = V3{Lr.x, Lr.y, Lr.z};
  V3 f = V3{th.x, th.y, th.z};
  V3 f2 = V3{pv.x, pv.y, pv.z};
  if (RENDER && bounce == 0) {  // next_smooth_si's f = Spectrum(1) (:135)
    f = v3s(1.f);
    f2 = v3s(1.f);
    depth = 0;
  }
  if (!RENDER && bounce == 0) {
    const mtx_material mat = sv.materials[si.material];
    DirectionSample ds;
    const V3 em = sample_emitter_direction(sv, si.p, rng.next_2d(), &ds);  // :197
    V3 val;
    float pdf;
    bsdf_eval_pdf(sv.bsdf, mat, si.uv, si.wi, to_local(si.sh, ds.d), &val, &pdf);  // :198
    const float mis = mis_weight_b(ds.pdf, pdf);
    make_shadow<MTX_INT_NERAD_RHS, false>(io, si, ds, v3s(1.f), val * mis * em, val * mis * v3s(0.f), false);  // :200
    const float s1 = rng.next_1d();
    const V2 s2 = rng.next_2d();
    BSDFSample bs;
    const V3 w = bsdf_sample(sv.bsdf, mat, si.uv, si.wi, s1, s2, &bs);  // :204-206
    const Ray nray = spawn_ray(si.p, si.n, to_world(si.sh, bs.wo));   // :208
    io.nro = f4(nray.o, nray.maxt);
    io.nrd = f4(nray.d, 0.f);
    b.thr[0][path] = f4(w, 1.f);
    b.L[kFinal][path] = f4(L, bs.pdf);
    b.prev[0][path] = f4(si.p, 0.f);
    b.misc[kFinal][path] = st_rng(rng, 0u);
    return true;  // traced unconditionally (:209)
  }
  if (!RENDER && bounce == 1) {
    // emitter pdf of the BSDF-sampled hit (:213-216), f (:217)
    const V3 prev_p = f2;
    const V3 rel = si.p - prev_p;
    const float dist = norm(rel);
    const float em_pdf = pdf_emitter_direction(sv, si.emitter, rel / dist, dist, si.sh.n);
    f = f * mis_weight_b(Lr.w, em_pdf);
    f2 = v3s(1.f);
  }
  // next_smooth_si (:124-164): sample at this vertex; continue while delta
  BSDFSample bs;
  bs.type = 0;
  V3 w = v3s(0.f);
  const float s1 = rng.next_1d();
  const V2 s2 = rng.next_2d();
  if (si.valid) {
    const mtx_material mat = sv.materials[si.material];
    w = bsdf_sample(sv.bsdf, mat, si.uv, si.wi, s1, s2, &bs);
  }
  if (bounce > (RENDER ? 0u : 1u)) depth += 1;  // :160
  const bool chain = (bs.type & BF_DELTA) != 0 && depth < 10;
  if (chain) {
    f2 = f2 * w;  // :150
    const Ray nray = spawn_ray(si.p, si.n, to_world(si.sh, bs.wo));
    io.nro = f4(nray.o, nray.maxt);
    io.nrd = f4(nray.d, 0.f);
    b.thr[0][path] = f4(f, 1.f);
    b.prev[0][path] = f4(f2, 0.f);
    b.misc[kFinal][path] = st_rng(rng, depth);
    return true;
  }
  // stop vertex (:219-229; render: :250-252)
  f = f * f2;
  if (!si.valid) f = f * 0.f;
  const V3 le = emitter_eval(sv, si.emitter, si.wi);
  if (RENDER && !si.valid) {
    L = v3s(0.f) * f + le;
    b.L[kFinal][path] = f4(L, Lr.w);
  } else if (si.valid) {
    io.query = true;
    const V3 wi = to_world(si.sh, si.wi);  // Field.__call__ wi (nerad.py:100)
    io.qp = f4(si.p, 0.f);
    io.qd = f4(wi, 0.f);
    io.qt = f4(f, __uint_as_float(path));
    b.prev[0][path] = f4(le, 0.f);
  } else {
    L = L + f * (le + v3s(0.f));
    b.L[kFinal][path] = f4(L, Lr.w);
  }
  return false;
}

}  // namespace mtxd
