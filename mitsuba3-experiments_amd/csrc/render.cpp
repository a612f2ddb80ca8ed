// render.cpp — wavefront scheduling: mtx_render, the ReSTIR GI frame, the
// PSSMLT loop, mtx_sample_rays and mtx_trace.
//
// The host side of the replaced path: upstream SamplingIntegrator::render
// (transcribed at path.py:103-192) seeds the sampler over W*H*spp lanes,
// traces one Dr.Jit wavefront and splats into an ImageBlock. Here the same
// lanes are processed in chunks of whole pixels; each chunk runs
// raygen -> [trace, shade, shadow] x max_depth -> film stage 1 on one HIP
// stream with no host synchronisation (the persistent kernels read their
// queue lengths from device counters), then one film gather per call.
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "runtime.h"
#include "mtx_core/film.h"
#include "prims.h"

namespace mtxh {

// Default wavefront: up to 256 Mi paths (~328 B of state each, ~82 GB) so a
// 1280x720 spp=256 frame runs as one chunk (fewer queue tails), bounded by
// 40 % of the free HBM.
constexpr uint32_t kDefaultChunk = 1u << 28;
constexpr size_t kPathStateBytes = 328;
constexpr size_t kCacheQueryBytes = 3 * kQueryBytes + kFeatBytes + kOutBytes;  // what ensure_cache allocates
// `ways` wavefronts of the returned size are allocated (2 for a two-stream
// render), each with the NRC cache-query buffers when `cache`: the budget is
// 40 % of the free HBM for all of them together. Buffers this context already
// holds (every wavefront's) count as available.
uint32_t default_chunk(mtx_ctx *c, const mtx_render_args *a, uint32_t ways, bool cache) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 1u << 22;
  // PSSMLT chains also keep the current and proposed path vertices
  const size_t per_path =
      kPathStateBytes + (cache ? kCacheQueryBytes : 0) +
      (a->integrator == MTX_INT_PSSMLT_SIMPLE ? 32ull * std::max<uint32_t>(a->max_depth, 1) + 48
       : a->integrator == MTX_INT_PSSMLT_PATH ? 48ull * std::max<uint32_t>(a->max_depth, 1) + 48
                                              : 0);
  const size_t held =
      ways > 1 ? std::min<size_t>(c->wave[0].capacity, c->wave[1].capacity) : c->wave[0].capacity;
  const size_t fit = std::max<size_t>((size_t)((double)free_b * 0.4) / (per_path * std::max<uint32_t>(ways, 1)), held);
  return (uint32_t)std::max<size_t>(1u << 20, std::min<size_t>(kDefaultChunk, fit));
}

// Queue counters and per-XCD claim cursors of a render of `depth` bounces.
constexpr size_t counters_bytes(uint32_t depth) { return 16ull * (depth + 2); }
constexpr size_t xheads_bytes(uint32_t depth) { return 8ull * mtxd::kXSlotWords * (depth + 2); }

// Wave `w` for `cap` paths of `max_depth` bounces. Wave 1 gets its stream
// and events on first use, and a traversal spill area of its own (two trace
// launches may run at once); wave 0's was sized by mtx_scene_upload for the
// same scene, so the dalloc below leaves it alone.
int ensure_wave(mtx_ctx *c, Wave &w, uint32_t cap, uint32_t max_depth) {
  int rc;
  if (!w.stream) {
    HIP_TRY(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&w.start, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
  }
  if (cap > w.capacity) {
    for (int k = 0; k < kNumPlanes; ++k)
      if ((rc = dalloc(w.plane[k], (size_t)kPlanes[k].elem * kPlanes[k].sub * cap))) return rc;
    w.capacity = cap;
  }
  if ((rc = dalloc(w.counters, counters_bytes(max_depth)))) return rc;
  if ((rc = dalloc(w.xheads, xheads_bytes(max_depth)))) return rc;
  if ((rc = dalloc(w.stack_ovf, mtxd::stack_ovf_bytes(c->scene.dev)))) return rc;
  if ((rc = dalloc(c->stats, 8 * 8))) return rc;
  return MTX_OK;
}

// Sub-plane k of a wave's plane, typed: T is the plane's entry.
template <class T, PlaneId id>
T *plane_at(const Wave &w, uint32_t k = 0) {
  static_assert(sizeof(T) == kPlanes[id].elem, "entry type and plane description disagree");
  return (T *)w.plane[id].p + (size_t)k * w.capacity;
}

// The kernels' view of a wave. Shared by both waves: stats, the PSSMLT
// planes (single-wave renders only); rs_xs / rs_ns are set by render_restir.
mtxd::WaveBuffers views(mtx_ctx *c, const Wave &w) {
  mtxd::WaveBuffers b{};
  for (uint32_t k = 0; k < 2; ++k) {
    b.ray_o[k] = plane_at<float4, kRayO>(w, k);
    b.ray_d[k] = plane_at<float4, kRayD>(w, k);
    b.thr[k] = plane_at<float4, kThr>(w, k);
    b.prev[k] = plane_at<float4, kPrev>(w, k);
  }
  for (uint32_t k = 0; k < 3; ++k) {
    b.L[k] = plane_at<float4, kL>(w, k);
    b.misc[k] = plane_at<uint4, kMisc>(w, k);
  }
  b.pos = plane_at<float2, kPos>(w);
  b.hit = plane_at<float4, kHit>(w);
  b.queue[0] = plane_at<uint32_t, kQ0>(w);
  b.queue[1] = plane_at<uint32_t, kQ1>(w);
  b.shadow = plane_at<float4, kShadow>(w);  // the kernels place its four planes (shadow_word)
  b.counters = (uint32_t *)w.counters.p;
  b.xheads = (uint32_t *)w.xheads.p;
  b.stats = (unsigned long long *)c->stats.p;
  b.capacity = w.capacity;
  b.mlt_cur = (float4 *)c->mlt.cur.p;
  b.mlt_L = (float4 *)c->mlt.L.p;
  b.mlt_prop = (float2 *)c->mlt.prop.p;
  b.vpath = (float4 *)c->mlt.vpath.p;
  b.vprop = (float4 *)c->mlt.vprop.p;
  b.vpath_es = (float2 *)c->mlt.vpath_es.p;
  b.vprop_es = (float2 *)c->mlt.vprop_es.p;
  b.cq_p = (float4 *)w.cq_p.p;  // null unless ensure_cache
  b.cq_d = (float4 *)w.cq_d.p;
  b.cq_t = (float4 *)w.cq_t.p;
  b.cq_count = (uint32_t *)w.cq_count.p;
  return b;
}

// The scene as wave `w` traces it: the context's, with the wave's spill area.
mtxd::DevScene wave_scene(const mtx_ctx *c, const Wave &w) {
  mtxd::DevScene s = c->scene.dev;
  s.stack_ovf = w.stack_ovf.p;
  return s;
}

// Zeroes a chunk's queue counters and the per-XCD claim cursors.
hipError_t reset_counters(const mtxd::WaveBuffers &b, uint32_t depth, hipStream_t st) {
  hipError_t e = hipMemsetAsync(b.counters, 0, counters_bytes(depth), st);
  if (e != hipSuccess) return e;
  return hipMemsetAsync(b.xheads, 0, xheads_bytes(depth), st);
}

int ensure_mlt(mtx_ctx *c, uint32_t cap, uint32_t max_depth, bool emitter_samples) {
  int rc;
  const size_t wc = c->wave[0].capacity;  // the chains run on wave 0
  if (emitter_samples && (!c->mlt.vpath_es.p || c->mlt.es_capacity != wc || max_depth > c->mlt.es_depth)) {
    if ((rc = dalloc(c->mlt.vpath_es, 8 * wc * max_depth))) return rc;
    if ((rc = dalloc(c->mlt.vprop_es, 8 * wc * max_depth))) return rc;
    c->mlt.es_capacity = wc;
    c->mlt.es_depth = max_depth;
  }
  if (cap > c->mlt.capacity || max_depth > c->mlt.depth || c->mlt.capacity != wc) {
    // vertex buffers are indexed [depth * wavefront capacity + chain]
    if ((rc = dalloc(c->mlt.cur, 16 * wc))) return rc;
    if ((rc = dalloc(c->mlt.L, 16 * wc))) return rc;
    if ((rc = dalloc(c->mlt.prop, 8 * wc))) return rc;
    if ((rc = dalloc(c->mlt.vpath, 16 * wc * max_depth))) return rc;
    if ((rc = dalloc(c->mlt.vprop, 16 * wc * max_depth))) return rc;
    c->mlt.capacity = wc;
    c->mlt.depth = max_depth;
  }
  return MTX_OK;
}

// Wave `w`'s NRC radiance-cache buffers for `cap` paths (queries <= paths).
// Callers ensure wave 0's first, so a missing field is refused before
// anything is allocated for either wave.
int ensure_cache(mtx_ctx *c, Wave &w, uint32_t cap) {
  int rc;
  if (!c->field.live) {
    mtx_set_error("mtx_render: NRC cache requested but no radiance field uploaded (mtx_field_upload)");
    return MTX_E_ARG;
  }
  for (DevBuf *q : {&w.cq_p, &w.cq_d, &w.cq_t})
    if ((rc = dalloc(*q, kQueryBytes * cap))) return rc;
  if ((rc = dalloc(w.cq_count, 16))) return rc;
  if ((rc = dalloc(w.f_feat, kFeatBytes * cap))) return rc;
  if ((rc = dalloc(w.f_out, kOutBytes * cap))) return rc;
  return MTX_OK;
}

int check_args(mtx_ctx *c, const mtx_render_args *a) {
  if (!c || !a) {
    mtx_set_error("null context or args");
    return MTX_E_ARG;
  }
  if (!c->scene.live) {
    mtx_set_error("no scene uploaded");
    return MTX_E_NOSCENE;
  }
  if (a->integrator != MTX_INT_PATH && a->integrator != MTX_INT_PATH_MIS && a->integrator != MTX_INT_NRC &&
      a->integrator != MTX_INT_PSSMLT_SIMPLE && a->integrator != MTX_INT_RESTIR_GI &&
      a->integrator != MTX_INT_PSSMLT_PATH && a->integrator != MTX_INT_NERAD && a->integrator != MTX_INT_SIMPLE) {
    mtx_set_error("integrator %u is not supported by this entry point", a->integrator);
    return MTX_E_UNSUPPORTED;
  }
  if (a->max_depth > 0xfffe) {
    mtx_set_error("max_depth %u too large", a->max_depth);
    return MTX_E_ARG;
  }
  return MTX_OK;
}

constexpr uint32_t kQSlots = 4096;  // chunks whose cache-query counts one stats render records

// Encode + MLP + L += T * out for the compacted cache queries of a chunk of
// wave `w` (views `b`), on the wave's stream with the wave's buffers.
int run_cache(mtx_ctx *c, Wave &w, const mtxd::WaveBuffers &b, uint32_t cap, Timer &tm, bool nerad_render) {
  hipStream_t st = w.stream;
  DevBuf &f_feat = w.f_feat, &f_out = w.f_out;
  const uint32_t *perm = nullptr;
  int xcd_split = 0;
  hipEvent_t e = tm.begin(4, st);
  if (c->knobs.cache_sort == 2 && !nerad_render) {
    // region-grouped rows, the blocks of each XCD on one eighth of them
    // (field.hip k_field_encode xcd_split): device-only, no host round trip
    if (!dalloc(w.cq_perm, 4ull * cap) && !dalloc(w.cq_cursor, 4ull * 32768)) {
      mtxd::field_bucket_queries(c->field.enc, b.cq_p, b.cq_count, cap, (uint32_t *)w.cq_cursor.p,
                                 (uint32_t *)w.cq_perm.p, c->n_cu, st);
      perm = (const uint32_t *)w.cq_perm.p;
      xcd_split = 1;
    }
  } else if (c->knobs.cache_sort && !nerad_render && &w == &c->wave[0]) {
    // encode the queries in Morton order (a stable sort of 24-bit cell codes
    // with the hash-grid group-by): the hash-grid corner gathers of
    // neighbouring rows then share table lines. The MLP row order follows;
    // k_cache_apply maps row q back to query perm[q]. Results are unchanged
    // (every query's features and MLP column are its own). Wave 0 only (a
    // host sync per chunk; mtx_render runs such a render on one stream).
    DevBuf &keys = w.cq_cursor;
    uint32_t nq = 0;
    if (hipMemcpyAsync(&nq, b.cq_count, 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
        hipStreamSynchronize(st) == hipSuccess && nq > 0 && !dalloc(keys, 4ull * nq) &&
        !dalloc(w.cq_perm, 4ull * nq) && !dalloc(c->cq_ws, mtxd::sort24_workspace_bytes(nq))) {
      mtxd::field_morton_keys(c->field.enc, b.cq_p, nq, (uint32_t *)keys.p, st);
      if (mtxd::sort24((const uint32_t *)keys.p, nq, (uint32_t *)w.cq_perm.p, c->cq_ws.p, st) == MTX_OK)
        perm = (const uint32_t *)w.cq_perm.p;
    }
  }
  // the fused pass only when its LDS fits a workgroup (n_hidden <= 14)
  const bool fused = c->knobs.cache_fused && !nerad_render && mtxd::field_cache_fused_lds(c->field.hidden) <= c->max_lds;
  int rc = MTX_OK;
  if (fused) {
    // encode + MLP + L += T * out in one launch (field.hip k_field_cache_fused),
    // timed as the encode
    rc = mtxd::field_cache_fused(c->field.enc, b.cq_p, b.cq_d, b.cq_t, b.cq_count, cap, perm, xcd_split,
                                 c->field.frag.p, c->field.hidden, b.L[mtxd::kFinal], c->n_cu, st);
    tm.end(4, e, st);
    if (rc) return rc;
  } else {
    rc = mtxd::field_encode(c->field.enc, b.cq_p, b.cq_d, b.cq_count, cap, (uint16_t *)f_feat.p, st, perm, xcd_split,
                            (int)c->knobs.encode_lm);
    tm.end(4, e, st);
    if (rc) return rc;
    e = tm.begin(5, st);
    rc = mtxd::field_mlp((const uint16_t *)f_feat.p, b.cq_count, cap, c->field.frag.p, c->field.hidden,
                         (float *)f_out.p, c->n_cu, st);
    tm.end(5, e, st);
    if (rc) return rc;
    if (nerad_render)
      mtxd::launch_nerad_apply(b, (const float *)f_out.p, cap, 1, st);
    else
      mtxd::launch_cache_apply(b, (const float *)f_out.p, cap, st, perm);
    HIP_TRY(hipGetLastError());
  }
  if (tm.on) {  // counted after the render's final synchronisation (fill_stats): no per-chunk sync
    if (!c->q_pinned && hipHostMalloc((void **)&c->q_pinned, 4 * kQSlots) != hipSuccess) c->q_pinned = nullptr;
    if (c->q_pinned && tm.q_used < kQSlots) {
      hipMemcpyAsync(c->q_pinned + tm.q_used++, b.cq_count, 4, hipMemcpyDeviceToHost, st);
    } else {  // more chunks than pinned slots: count this one synchronously (never dropped)
      uint32_t nq = 0;
      if (hipMemcpyAsync(&nq, b.cq_count, 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipStreamSynchronize(st) == hipSuccess)
        tm.cache_queries += nq;
    }
  }
  return MTX_OK;
}

// One bounce of a chunk: closest hit, shade, NEE shadow rays.
void launch_bounce(mtx_ctx *c, const mtxd::WaveBuffers &b, const mtxd::ChunkParams &p, Timer &tm,
                   uint64_t *n_trace, uint64_t *n_shadow, const mtxd::DevScene &s, hipStream_t st, uint32_t bounce) {
  // nerad RHS lanes start at their surface point (no bounce-0 trace) and
  // trace NEE rays at that point only
  const bool nerad = p.integrator == MTX_INT_NERAD_RHS, nerad_render = p.integrator == MTX_INT_NERAD;
  hipEvent_t e;
  // past its second vertex the nerad RHS chain only continues through
  // delta surfaces (next_smooth_si): a small queue, traced and shaded by
  // an eighth of the persistent grid (dispatching the full grid of
  // immediately-exiting blocks costs more than the work)
  const int div = (nerad && bounce >= 2) ? 8 : 1;
  if (!(nerad && bounce == 0)) {
    e = tm.begin(0, st);
    if (bounce == 0 && p.cam0)  // no stored raygen: the traversal derives its camera rays
      mtxd::launch_trace_camera(s, b, p, std::max(1, c->closest_grid / div), st);
    else
      mtxd::launch_trace_closest(s, b, bounce, p.stats, std::max(1, c->closest_grid / div), st);
    tm.end(0, e, st);
    ++*n_trace;
  }
  e = tm.begin(2, st);
  mtxd::launch_shade(s, b, p, bounce, std::max(1, c->shade_grid / div), st, c->knobs.shade_classes != 0);
  tm.end(2, e, st);
  if (p.integrator != MTX_INT_PSSMLT_SIMPLE && p.integrator != MTX_INT_SIMPLE && !nerad_render &&
      !(nerad && bounce > 0)) {  // PSSMLT, simple and the nerad render trace no NEE rays
    e = tm.begin(1, st);
    mtxd::launch_trace_shadow(s, b, bounce, p.stats, c->trace_grid, st);
    tm.end(1, e, st);
    ++*n_shadow;
  }
}

// Bounces of a chunk's loop (an NRC cache query needs one more trace + shade
// after the last segment).
uint32_t bounce_iters(const mtxd::ChunkParams &p) {
  return std::max<uint32_t>(p.max_depth, 1) + (p.nrc_cache ? 1u : 0u);
}

// Paths a depth limit left queued keep their result in a queue plane.
void finish_bounces(const mtxd::WaveBuffers &b, const mtxd::ChunkParams &p, hipStream_t st) {
  if (p.integrator != MTX_INT_NERAD_RHS && p.integrator != MTX_INT_NERAD)
    mtxd::launch_flush_tail(b, bounce_iters(p), b.capacity, p.integrator, st);
}

// Runs the bounce loop of one chunk of wave `w` (views `b`; rays already
// generated, counters[0] set) on the wave's stream.
void run_bounces(mtx_ctx *c, const Wave &w, const mtxd::WaveBuffers &b, const mtxd::ChunkParams &p, Timer &tm,
                 uint64_t *n_trace, uint64_t *n_shadow) {
  const mtxd::DevScene s = wave_scene(c, w);
  hipStream_t st = w.stream;
  const uint32_t depth_iters = bounce_iters(p);
  for (uint32_t bounce = 0; bounce < depth_iters; ++bounce) {
    launch_bounce(c, b, p, tm, n_trace, n_shadow, s, st, bounce);
    // Deep paths (max_depth 65, scene.xml:6): stop launching once the queue
    // has drained (checked every 8 bounces).
    if (depth_iters > 16 && (bounce & 7) == 7 && bounce + 1 < depth_iters) {
      uint32_t cnt = 0;
      hipMemcpyAsync(&cnt, b.counters + 4 * (bounce + 1), 4, hipMemcpyDeviceToHost, st);
      hipStreamSynchronize(st);
      if (cnt == 0) return;
    }
  }
  finish_bounces(b, p, st);
}

int fill_stats(mtx_ctx *c, mtx_stats *stats, bool want_stats, Timer &tm, uint64_t n_trace, uint64_t n_shadow,
               uint64_t paths) {
  if (!stats) return MTX_OK;
  memset(stats, 0, sizeof(*stats));
  if (want_stats) {
    unsigned long long h[8];
    HIP_TRY(hipMemcpy(h, c->stats.p, 64, hipMemcpyDeviceToHost));
    stats->nodes_closest = h[0];
    stats->tris_closest = h[1];
    stats->nodes_shadow = h[2];
    stats->tris_shadow = h[3];
    stats->rays_closest = h[4];
    stats->rays_shadow = h[5];
    stats->wave_node_iters = h[6];
    stats->wave_leaf_iters = h[7];
  }
  stats->trace_launches = n_trace;
  stats->shadow_launches = n_shadow;
  stats->streams = tm.streams;
  stats->paths = paths;
  if (tm.on) {
    stats->trace_ms = tm.total(0);
    stats->shadow_ms = tm.total(1);
    stats->shade_ms = tm.total(2);
    stats->cache_encode_ms = tm.total(4);
    stats->cache_mlp_ms = tm.total(5);
    for (uint32_t i = 0; i < tm.q_used; ++i) tm.cache_queries += c->q_pinned[i];
    stats->cache_queries = tm.cache_queries;
    stats->other_ms = tm.total(3) - stats->trace_ms - stats->shadow_ms - stats->shade_ms - stats->cache_encode_ms -
                      stats->cache_mlp_ms;
  }
  return MTX_OK;
}

int ensure_restir(mtx_ctx *c, uint32_t n) {
  int rc;
  if (c->restir.n != n) {
    c->restir.valid = false;
    const size_t N = n;
    for (int k = 0; k < 2; ++k)
      if ((rc = dalloc(c->restir.samp[k], 5 * 16 * N))) return rc;
    if ((rc = dalloc(c->restir.tres, 6 * 16 * N))) return rc;
    if ((rc = dalloc(c->restir.sres, 6 * 16 * N))) return rc;
    if ((rc = dalloc(c->restir.radius, 4 * N))) return rc;
    if ((rc = dalloc(c->restir.hit, 16 * N))) return rc;
    if ((rc = dalloc(c->restir.dir, 16 * N))) return rc;
    if ((rc = dalloc(c->restir.emit, 16 * N))) return rc;
    if ((rc = dalloc(c->restir.rng, 16 * N))) return rc;
    if ((rc = dalloc(c->restir.rays, 9 * 32 * N))) return rc;
    if ((rc = dalloc(c->restir.count, 16))) return rc;
    if ((rc = dalloc(c->restir.heads, 4ull * mtxd::kXSlotWords))) return rc;
    if ((rc = dalloc(c->restir.occ, 18 * N))) return rc;
    if ((rc = dalloc(c->restir.qM, 10 * 4 * N))) return rc;
    if ((rc = dalloc(c->restir.nbr, 10 * 4 * N))) return rc;
    if ((rc = dalloc(c->restir.xs, 16 * N))) return rc;
    if ((rc = dalloc(c->restir.ns, 16 * N))) return rc;
    c->restir.n = n;
  }
  return MTX_OK;
}

// One RestirIntegrator.render() frame (restirgi.py:182-258) over the whole
// film; the kernel sequence is documented in restir.hip.
int render_restir(mtx_ctx *c, const mtx_render_args *a, float4 *film_dev, Timer &tm, uint64_t *n_trace,
                  uint64_t *n_shadow, bool want_stats) {
  const mtx_camera &cam = c->scene.dev.camera;
  const uint32_t W = cam.width, H = cam.height, spp = a->spp;
  if (a->sample_offset != 0 || a->spp_total != spp) {
    mtx_set_error("mtx_render: ReSTIR GI needs spp_total = spp and sample_offset = 0");
    return MTX_E_ARG;
  }
  if (c->scene.dev.has_env) {
    // restirgi.py's reservoirs keep the first secondary hit (x_s, n_s) and
    // its visibility; a secondary ray escaping to an environment has no such
    // point, and the reference's handling of it is not restated here
    mtx_set_error("mtx_render: ReSTIR GI with an environment emitter is not supported");
    return MTX_E_UNSUPPORTED;
  }
  const uint64_t n64 = (uint64_t)W * H * spp;
  if (n64 * 18 >= (1ull << 32)) {
    mtx_set_error("mtx_render: ReSTIR GI frame too large (%llu lanes)", (unsigned long long)n64);
    return MTX_E_ARG;
  }
  const bool only_a = (a->restir_flags & MTX_RESTIR_STAGE_A) != 0;
  const bool only_b = (a->restir_flags & MTX_RESTIR_STAGE_B) != 0;
  if (only_a && only_b) {
    mtx_set_error("mtx_render: ReSTIR stage A and stage B flags are exclusive");
    return MTX_E_ARG;
  }
  const bool run_a = !only_b, run_b = !only_a;
  const uint32_t n = (uint32_t)n64;
  const uint32_t lane0 = a->y0 * W * spp, nb = (a->y1 - a->y0) * W * spp;
  const uint32_t depth = std::max<uint32_t>(a->max_depth, 1);
  int rc;
  Wave *wv = c->wave;
  if ((rc = ensure_wave(c, wv[0], nb, depth))) return rc;
  if ((rc = ensure_restir(c, n))) return rc;
  if (run_a && a->frame != 0 && !c->restir.valid) {
    mtx_set_error("mtx_render: ReSTIR GI frame %u without the state of frame 0 (film size or scene changed?)",
                  a->frame);
    return MTX_E_ARG;
  }
  if (only_b && (!c->restir.pending_b || c->restir.pending_frame != a->frame)) {
    mtx_set_error("mtx_render: ReSTIR stage B of frame %u without its stage A", a->frame);
    return MTX_E_ARG;
  }
  hipStream_t st = c->stream;
  if (run_a && a->frame == 0) {  // restirgi.py:217-229
    HIP_TRY(hipMemsetAsync(c->restir.tres.p, 0, 6 * 16 * (size_t)n, st));
    HIP_TRY(hipMemsetAsync(c->restir.sres.p, 0, 6 * 16 * (size_t)n, st));
    HIP_TRY(hipMemsetAsync(c->restir.samp[0].p, 0, 5 * 16 * (size_t)n, st));
    HIP_TRY(hipMemsetAsync(c->restir.samp[1].p, 0, 5 * 16 * (size_t)n, st));
    uint32_t bits;
    memcpy(&bits, &a->initial_search_radius, 4);
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c->restir.radius.p, (int)bits, n, st));
    c->restir.prev_cam = cam;
    c->restir.cur = 0;
  }
  mtxd::WaveBuffers b = views(c, wv[0]);
  mtxd::RestirBuffers r{};
  r.cur = (float4 *)c->restir.samp[c->restir.cur].p;
  r.prev = a->frame == 0 ? r.cur : (const float4 *)c->restir.samp[c->restir.cur ^ 1].p;
  r.tres = (float4 *)c->restir.tres.p;
  r.sres = (float4 *)c->restir.sres.p;
  r.radius = (float *)c->restir.radius.p;
  r.prim_hit = (float4 *)c->restir.hit.p;
  r.prim_dir = (float4 *)c->restir.dir.p;
  r.emit = (float4 *)c->restir.emit.p;
  r.rng = (uint4 *)c->restir.rng.p;
  r.test_rays = (float4 *)c->restir.rays.p;
  r.test_count = (uint32_t *)c->restir.count.p;
  r.test_heads = (uint32_t *)c->restir.heads.p;
  r.occ = (uint8_t *)c->restir.occ.p;
  r.qM = (uint32_t *)c->restir.qM.p;
  r.nbr = (uint32_t *)c->restir.nbr.p;
  r.n = n;
  r.lane0 = lane0;
  r.nb = nb;
  r.prev_cam = c->restir.prev_cam;
  r.flags = a->restir_flags;
  r.xcd_remap = c->knobs.xcd_claim;
  r.max_M_temporal = a->max_M_temporal;
  r.max_M_spatial = a->max_M_spatial;
  r.initial_radius = a->initial_search_radius;
  r.minimal_radius = a->minimal_search_radius;
  r.frame = a->frame;
  b.rs_xs = (float4 *)c->restir.xs.p;
  b.rs_ns = (float4 *)c->restir.ns.p;

  mtxd::ChunkParams p{};
  p.integrator = MTX_INT_RESTIR_GI;
  p.max_depth = a->max_depth;
  p.rr_depth = a->rr_depth;
  p.seed = a->seed;
  p.spp = spp;
  p.spp_total = spp;
  p.width = W;
  p.height = H;
  p.px0 = a->y0 * W;
  p.n_px = (a->y1 - a->y0) * W;
  p.band_y0 = a->y0;
  p.band_px = (a->y1 - a->y0) * W;
  p.rfilter = a->rfilter;
  p.n_paths = nb;
  p.restir = 1;
  p.stats = want_stats ? 1 : 0;
  if (want_stats) HIP_TRY(hipMemsetAsync(c->stats.p, 0, 64, c->stream));
  hipEvent_t e;
  if (run_a) {
    // Stage A is per lane up to and including the temporal resampling (which
    // reads this frame's lane and the complete previous frame), so the band's
    // rows split into two halves traced on two wavefronts / streams: one
    // half's kernels fill the tails of the other's short (~2 M-ray)
    // persistent launches. Same lanes, same draws: bit-identical.
    // A band of at most mega_max paths (default: twice the megakernel's
    // resident lanes, 2 x mega_grid x kShadeBlock) runs all of its secondary
    // paths in the path megakernel on ONE wavefront instead (the band is not
    // split into halves then): one launch of at most the resident blocks,
    // whose waves claim the queued paths 64 at a time.
    const uint32_t rows = a->y1 - a->y0;
    const uint32_t mega_max =
        c->knobs.mega_paths == 0xffffffffu ? 2u * (uint32_t)c->mega_grid * mtxd::kShadeBlock : c->knobs.mega_paths;
    const bool mega_all = !p.stats && nb <= mega_max;
    const bool two = !mega_all && c->knobs.streams > 1 && rows >= 2 && nb >= (1u << 16);
    if (two) tm.streams = 2;
    const uint32_t ym = two ? a->y0 + rows / 2 : a->y1;
    if (two) {  // wave 1 holds the second half only
      if ((rc = ensure_wave(c, wv[1], (a->y1 - ym) * W * spp, depth))) return rc;
      HIP_TRY(hipEventRecord(wv[1].start, st));  // after the frame-0 clears
      HIP_TRY(hipStreamWaitEvent(wv[1].stream, wv[1].start, 0));
    }
    // The halves' launches are enqueued interleaved, step by step (prologue,
    // each bounce, epilogue), so the second stream starts at once instead of
    // after the host has queued all of the first half's launches.
    const int halves = two ? 2 : 1;
    const mtxd::DevScene sc[2] = {wave_scene(c, wv[0]), wave_scene(c, wv[1])};
    hipStream_t sh[2] = {st, wv[1].stream};
    if (mega_all && c->knobs.rs_fused) {
      // the whole stage A up to k_rs_collect in one per-lane launch
      // (mega.hip k_rs_stage_a), then the temporal pass
      HIP_TRY(reset_counters(b, depth, st));
      e = tm.begin(0, st);
      mtxd::launch_rs_stage_a(sc[0], b, p, r,
                              std::max(1, std::min<int>(c->mega_grid, (nb + mtxd::kShadeBlock - 1) / mtxd::kShadeBlock)),
                              st);
      tm.end(0, e, st);
      ++*n_trace;
      mtxd::launch_restir_temporal(r, p, st);
    }
    const bool fused = mega_all && c->knobs.rs_fused;
    mtxd::WaveBuffers bh[2], b1[2];
    mtxd::ChunkParams ph[2];
    mtxd::RestirBuffers rh[2];
    for (int h = 0; h < (fused ? 0 : halves); ++h) {
      const uint32_t ya = h ? ym : a->y0, yb = h ? a->y1 : ym;
      bh[h] = h ? views(c, wv[1]) : b;
      bh[h].rs_xs = b.rs_xs + (size_t)(ya - a->y0) * W * spp;  // path-indexed within the half
      bh[h].rs_ns = b.rs_ns + (size_t)(ya - a->y0) * W * spp;
      ph[h] = p;
      ph[h].px0 = ya * W;
      ph[h].n_px = (yb - ya) * W;
      ph[h].n_paths = ph[h].n_px * spp;
      rh[h] = r;
      rh[h].lane0 = ya * W * spp;
      rh[h].nb = ph[h].n_paths;
      // sample_initial: primary rays and their closest hits
      HIP_TRY(reset_counters(bh[h], depth, sh[h]));
      mtxd::launch_raygen_camera(sc[h], bh[h], ph[h], sh[h]);
      e = tm.begin(0, sh[h]);
      mtxd::launch_trace_closest(sc[h], bh[h], 0, ph[h].stats, c->closest_grid, sh[h]);
      tm.end(0, e, sh[h]);
      ++*n_trace;
      HIP_TRY(reset_counters(bh[h], depth, sh[h]));
      mtxd::launch_restir_begin(sc[h], bh[h], ph[h], rh[h], sh[h]);
      b1[h] = bh[h];  // k_rs_begin left the secondary rays in the parity-1 planes
      b1[h].ray_par = 1;
    }
    // sample_ray (the path-mis loop): with mega_all (halves == 1) the whole
    // band runs all its bounces in the path megakernel (no counters: STATS
    // renders keep the wavefront kernels)
    bool mega[2] = {false, false};
    for (int h = 0; h < (fused ? 0 : halves); ++h) {
      mega[h] = mega_all;
      if (!mega[h]) continue;
      e = tm.begin(0, sh[h]);
      mtxd::launch_path_mega(sc[h], b1[h], ph[h],
                             std::max(1, std::min<int>(c->mega_grid, (ph[h].n_paths + mtxd::kShadeBlock - 1) /
                                                                         mtxd::kShadeBlock)),
                             sh[h]);
      tm.end(0, e, sh[h]);
      ++*n_trace;
    }
    const uint32_t iters = fused ? 0u : bounce_iters(p);
    for (uint32_t bounce = 0; bounce < iters; ++bounce)
      for (int h = 0; h < halves; ++h)
        if (!mega[h]) launch_bounce(c, b1[h], ph[h], tm, n_trace, n_shadow, sc[h], sh[h], bounce);
    for (int h = 0; h < (fused ? 0 : halves); ++h) {
      if (!mega[h]) finish_bounces(b1[h], ph[h], sh[h]);
      mtxd::launch_restir_collect(bh[h], ph[h], rh[h], sh[h]);
      mtxd::launch_restir_temporal(rh[h], ph[h], sh[h]);
    }
    if (two) {  // stage B reads every lane of the band
      HIP_TRY(hipEventRecord(wv[1].done, wv[1].stream));
      HIP_TRY(hipStreamWaitEvent(st, wv[1].done, 0));
    }
  }
  if (run_b) {
    // spatial_resampling (reads samples / temporal reservoirs of rows outside
    // the band: a row-banded caller imports them between stage A and B)
    HIP_TRY(hipMemsetAsync(r.test_count, 0, 16, st));
    HIP_TRY(hipMemsetAsync(r.test_heads, 0, 4ull * mtxd::kXSlotWords, st));
    mtxd::launch_restir_spatial_rays(r, p, st);
    e = tm.begin(1);
    mtxd::launch_trace_test(c->scene.dev, r, 0, c->trace_grid, st);
    tm.end(1, e);
    ++*n_shadow;
    HIP_TRY(hipMemsetAsync(r.test_count, 0, 16, st));
    HIP_TRY(hipMemsetAsync(r.test_heads, 0, 4ull * mtxd::kXSlotWords, st));
    mtxd::launch_restir_spatial_merge(r, p, st);
    if (a->restir_flags & MTX_RESTIR_BIAS_CORRECTION) {
      e = tm.begin(1);
      mtxd::launch_trace_test(c->scene.dev, r, 9 * n, c->trace_grid, st);
      tm.end(1, e);
      ++*n_shadow;
      mtxd::launch_restir_bias_finish(r, p, st);
    }
    mtxd::launch_restir_final(c->scene.dev, b, p, r, st);
    mtxd::launch_film_src(b, p, (float4 *)c->contrib.p, st);
    mtxd::launch_film_gather((const float4 *)c->contrib.p, film_dev, W, a->y0, a->y1, 1, 1u, a->rfilter, st);
  }
  HIP_TRY(hipGetLastError());
  if (only_a) {
    c->restir.pending_b = true;
    c->restir.pending_frame = a->frame;
    c->restir.valid = a->frame != 0 ? c->restir.valid : false;
    return MTX_OK;
  }
  // restirgi.py:245-247: prev_sensor <- sensor, prev_sample <- sample
  c->restir.pending_b = false;
  c->restir.prev_cam = cam;
  c->restir.cur ^= 1;
  c->restir.valid = true;
  return MTX_OK;
}

}  // namespace mtxh

using namespace mtxh;

extern "C" {

int mtx_render(mtx_ctx *c, const mtx_render_args *a, float *film_rgbw, int film_on_device, mtx_stats *stats) {
  int rc = check_args(c, a);
  if (rc) return rc;
  const mtx_camera &cam = c->scene.dev.camera;
  const uint32_t W = cam.width, H = cam.height;
  if (!film_rgbw || a->spp == 0 || a->y1 <= a->y0 || a->y1 > H || a->spp_total < a->sample_offset + a->spp) {
    mtx_set_error("mtx_render: bad film/rows/spp arguments");
    return MTX_E_ARG;
  }
  if (a->rfilter >= mtx::kRfilterCount) {
    mtx_set_error("mtx_render: unknown reconstruction filter %u (MTX_RFILTER_TENT 0, _BOX 1, _GAUSSIAN 2)",
                  a->rfilter);
    return MTX_E_ARG;
  }
  // the film's border and the taps per source pixel follow the filter (mtx_core/film.h)
  const uint32_t fb = mtx::rfilter_reach(a->rfilter);
  const uint64_t taps = (uint64_t)(2 * fb + 1) * (2 * fb + 1);
  if ((uint64_t)W * H * a->spp_total >= (1ull << 32)) {
    mtx_set_error("mtx_render: W*H*spp_total exceeds the 32-bit sampler lane space");
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t band_px = (a->y1 - a->y0) * W;
  const bool nrc_cache = a->integrator == MTX_INT_NRC && (a->flags & 4u);
  const bool nerad_render = a->integrator == MTX_INT_NERAD;
  const bool mlt = a->integrator == MTX_INT_PSSMLT_SIMPLE || a->integrator == MTX_INT_PSSMLT_PATH;
  // two wavefronts on two streams (wave[0], wave[1]): the band splits into at least two
  // chunks that alternate between them (the caller's chunk size still caps a
  // chunk), so one chunk's kernels fill the tails of the other's persistent
  // trace launches (~0.2 ms per launch that does not shrink with the rays).
  // Renders of 2^16 .. 2^27 paths: the bench's per-rank share at N >= 2
  // (spp 32: 26.8 -> 25.9 ms per step; spp 128: 91.6 -> 90.2 ms); at spp 256
  // (2^27.8 paths) it gains 0.5 % and would blur the per-kernel event times
  // the N = 1 roofline is measured with. Path-state integrators without a
  // per-chunk cache pass only.
  const uint64_t n_paths_all = (uint64_t)band_px * a->spp;
  // (NRC + cache: each wavefront has its own query / feature buffers, so one
  // chunk's cache pass overlaps the other's bounces; not with the Morton sort)
  const bool two = c->knobs.streams > 1 && !mlt && !(nrc_cache && c->knobs.cache_sort == 1) && !nerad_render &&
                   a->integrator != MTX_INT_RESTIR_GI && n_paths_all >= (1u << 16) &&
                   n_paths_all <= (1ull << c->knobs.streams_max_log2);
  // the default chunk is sized for every wavefront the render allocates
  const uint32_t chunk_paths =
      a->chunk_paths ? a->chunk_paths : default_chunk(c, a, two ? 2u : 1u, nrc_cache || nerad_render);
  uint32_t px_per_chunk = std::min(std::max<uint32_t>(1, chunk_paths / a->spp), band_px);
  if (two) px_per_chunk = std::min(px_per_chunk, (band_px + 1) / 2);
  const uint32_t cap = px_per_chunk * a->spp;
  const uint32_t depth = std::max<uint32_t>(a->max_depth, 1);
  const int n_waves = two ? 2 : 1;
  for (int k = 0; k < n_waves; ++k) {
    if ((rc = ensure_wave(c, c->wave[k], cap, depth))) return rc;
    if ((nrc_cache || nerad_render) && (rc = ensure_cache(c, c->wave[k], cap))) return rc;
  }
  // sample-sharded film renders: 8 partial slots (GPU-count-invariant films,
  // DESIGN.md "Film"); PSSMLT splats and ReSTIR frames: one
  const uint32_t film_slots = (mlt || a->integrator == MTX_INT_RESTIR_GI) ? 1u : 8u;
  // the slots [sample_offset, sample_offset + spp) falls in (FilmSlots: slot k
  // takes global samples [end(k - 1), end(k)), slot 7 everything past end(6))
  uint32_t slot_mask = 1u;
  if (film_slots == 8) {
    slot_mask = 0;
    for (uint32_t k = 0; k < 8; ++k) {
      const uint64_t lo = k ? mtx::film_slot_end(k - 1, a->spp_total) : 0u;
      const uint64_t hi = k < 7 ? mtx::film_slot_end(k, a->spp_total) : ~0ull;
      if (std::max<uint64_t>(lo, a->sample_offset) < std::min<uint64_t>(hi, (uint64_t)a->sample_offset + a->spp))
        slot_mask |= 1u << k;
    }
  }
  if ((rc = dalloc(c->contrib, taps * 16 * band_px * film_slots))) return rc;
  const size_t film_floats = 4ull * (W + 2 * fb) * (a->y1 - a->y0 + 2 * fb);
  float4 *film_dev = (float4 *)film_rgbw;
  if (!film_on_device) {
    if ((rc = dalloc(c->film, film_floats * 4))) return rc;
    film_dev = (float4 *)c->film.p;
  }
  const bool want_stats = stats && (a->flags & 1u);
  Timer tm{c, stats && (a->flags & 2u)};
  if (two) tm.streams = 2;
  if (a->integrator == MTX_INT_RESTIR_GI) {
    hipEvent_t e_all = tm.begin(3);
    uint64_t n_trace = 0, n_shadow = 0;
    if ((rc = render_restir(c, a, film_dev, tm, &n_trace, &n_shadow, want_stats))) return rc;
    tm.end(3, e_all);
    // stage A writes no film: no copy, and no wait unless stats were asked
    // for (the caller's stage B follows on the same stream)
    const bool stage_a = (a->restir_flags & MTX_RESTIR_STAGE_A) != 0;
    if (!film_on_device && !stage_a)
      HIP_TRY(hipMemcpyAsync(film_rgbw, film_dev, film_floats * 4, hipMemcpyDeviceToHost, c->stream));
    if (!stage_a || stats) HIP_TRY(hipStreamSynchronize(c->stream));
    return fill_stats(c, stats, want_stats, tm, n_trace, n_shadow, (uint64_t)W * H * a->spp);
  }
  if (mlt) {
    if ((rc = ensure_mlt(c, cap, depth, a->integrator == MTX_INT_PSSMLT_PATH))) return rc;
    HIP_TRY(hipMemsetAsync(c->contrib.p, 0, taps * 16 * band_px, c->stream));
  }
  // every allocation is made: the views of the waves this render uses
  mtxd::WaveBuffers views_of[2];
  for (int k = 0; k < n_waves; ++k) views_of[k] = views(c, c->wave[k]);
  if (want_stats) HIP_TRY(hipMemsetAsync(c->stats.p, 0, 64, c->stream));
  uint64_t n_trace = 0, n_shadow = 0;
  hipEvent_t e_all = tm.begin(3);
  if (two) {
    // the second stream starts after everything queued on the first
    HIP_TRY(hipEventRecord(c->wave[1].start, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->wave[1].stream, c->wave[1].start, 0));
  }
  uint32_t chunk_index = 0;
  for (uint32_t px0 = a->y0 * W; px0 < a->y1 * W; px0 += px_per_chunk, ++chunk_index) {
    // chunks alternate between the waves (PSSMLT, the nerad render and the
    // Morton-sorted cache are never two-stream renders: wave 0)
    const int wi = two ? (int)(chunk_index & 1u) : 0;
    Wave &w = c->wave[wi];
    hipStream_t st = w.stream;
    const mtxd::WaveBuffers &bc = views_of[wi];
    const mtxd::DevScene sc = wave_scene(c, w);
    mtxd::ChunkParams p{};
    p.integrator = a->integrator;
    p.max_depth = a->max_depth;
    p.rr_depth = a->rr_depth;
    p.seed = a->seed;
    p.spp = a->spp;
    p.spp_total = a->spp_total;
    p.sample_offset = a->sample_offset;
    p.width = W;
    p.height = H;
    p.px0 = px0;
    p.n_px = std::min(px_per_chunk, a->y1 * W - px0);
    p.band_y0 = a->y0;
    p.band_px = (a->y1 - a->y0) * W;
    p.film_slots = film_slots;
    p.rfilter = a->rfilter;
    p.slot_mask = slot_mask;
    p.n_paths = p.n_px * a->spp;
    p.nrc_c = a->nrc_c;
    p.stats = want_stats ? 1 : 0;
      p.nrc_cache = nrc_cache ? 1u : 0u;
    // the film (and the cache apply) read an ending path's L only; PSSMLT's
    // chain kernels read its sampler state (mtx_sample_rays' k_collect and
    // ReSTIR's k_rs_collect build their own ChunkParams, which keep it)
    p.drop_end_misc = mlt ? 0u : 1u;
    p.ident0 = 1;  // raygen_camera / mlt_begin queue every path at its own position
    // path, path-mis, nrc and simple derive the camera sample where it is used
    // (no raygen launch, no bounce-0 planes, no pos). The nerad render keeps the
    // stored raygen: its bounce-0 shade reads the raygen's misc plane by path.
    p.cam0 = (!mlt && !nerad_render) ? MTX_CAM0 : 0u;
    if (mlt) {
      // Pssmlt.render (pssmlt.py:167-228): all iterations of this chunk's chains
      const uint32_t iters = a->iterations ? a->iterations : 200;
      mtxd::launch_mlt_init(bc, p, st);
      for (uint32_t it = 0; it < iters; ++it) {
        p.large_step = (it % 50 == 0) ? 1u : 0u;  // reset_interval = 50 (:209)
        HIP_TRY(reset_counters(bc, depth, st));
        mtxd::launch_mlt_begin(sc, bc, p, st);
        run_bounces(c, w, bc, p, tm, &n_trace, &n_shadow);
        mtxd::launch_mlt_end(bc, p, st);
        if (it % 50 > 40) mtxd::launch_mlt_film(bc, p, (float4 *)c->contrib.p, st);  // bootstrapping = 40
      }
      continue;
    }
    HIP_TRY(reset_counters(bc, depth, st));
    if (nrc_cache || nerad_render) HIP_TRY(hipMemsetAsync(bc.cq_count, 0, 4, st));
    if (p.cam0)  // what raygen's thread 0 did: the bounce-0 queue holds every path
      HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)bc.counters, (int)p.n_paths, 1, st));
    else
      mtxd::launch_raygen_camera(sc, bc, p, st);
    run_bounces(c, w, bc, p, tm, &n_trace, &n_shadow);
    if ((nrc_cache || nerad_render) && (rc = run_cache(c, w, bc, p.n_paths, tm, nerad_render))) return rc;
    mtxd::launch_film_src(bc, p, (float4 *)c->contrib.p, st);
  }
  if (two) {  // the film gather reads both wavefronts' contributions
    HIP_TRY(hipEventRecord(c->wave[1].done, c->wave[1].stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->wave[1].done, 0));
  }
  mtxd::launch_film_gather((const float4 *)c->contrib.p, film_dev, W, a->y0, a->y1, film_slots, slot_mask, a->rfilter,
                           c->stream);
  tm.end(3, e_all);
  HIP_TRY(hipGetLastError());
  if (!film_on_device)
    HIP_TRY(hipMemcpyAsync(film_rgbw, film_dev, film_floats * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return fill_stats(c, stats, want_stats, tm, n_trace, n_shadow, (uint64_t)band_px * a->spp);
}

int mtx_restir_rows(mtx_ctx *c, int which, uint32_t row0, uint32_t nrows, void *buf, int to_state) {
  if (!c || !buf || which < 0 || which > 2) {
    mtx_set_error("mtx_restir_rows: bad argument");
    return MTX_E_ARG;
  }
  if (!c->restir.n || !c->scene.live) {
    mtx_set_error("mtx_restir_rows: no ReSTIR GI state");
    return MTX_E_ARG;
  }
  const uint32_t W = c->scene.dev.camera.width, H = c->scene.dev.camera.height;
  if (row0 + nrows > H || nrows == 0) {
    mtx_set_error("mtx_restir_rows: rows [%u, %u) outside the film", row0, row0 + nrows);
    return MTX_E_ARG;
  }
  const size_t n = c->restir.n, per_row = n / H;  // lanes per row (W * spp)
  (void)W;
  if (which == 2 && (!c->restir.valid || c->restir.pending_b)) {
    mtx_set_error("mtx_restir_rows: the previous frame's samples exist between complete frames only");
    return MTX_E_ARG;
  }
  const int planes = which == 1 ? 6 : 5;
  // which = 0: the current frame's samples (before stage B swaps them);
  // 2: the previous frame's (what k_rs_temporal reads through prev_cam)
  char *state = (char *)(which == 0 ? c->restir.samp[c->restir.cur].p
                                    : which == 2 ? c->restir.samp[c->restir.cur ^ 1].p : c->restir.tres.p);
  char *dev = (char *)buf;
  HIP_TRY(hipSetDevice(c->device));
  for (int k = 0; k < planes; ++k) {
    char *s = state + 16 * ((size_t)k * n + (size_t)row0 * per_row);
    char *d = dev + 16 * (size_t)k * nrows * per_row;
    const size_t bytes = 16 * (size_t)nrows * per_row;
    HIP_TRY(hipMemcpyAsync(to_state ? s : d, to_state ? d : s, bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

int mtx_restir_state(mtx_ctx *c, int which, float *out, uint64_t n_floats) {
  if (!c || !out) {
    mtx_set_error("mtx_restir_state: null argument");
    return MTX_E_ARG;
  }
  if (!c->restir.valid) {
    mtx_set_error("mtx_restir_state: no ReSTIR GI frame rendered");
    return MTX_E_ARG;
  }
  const uint64_t n = c->restir.n;
  const void *src = nullptr;
  uint64_t need = 0;
  switch (which) {
    case 0: src = c->restir.samp[c->restir.cur ^ 1].p; need = 20 * n; break;  // the frame just rendered
    case 1: src = c->restir.tres.p; need = 24 * n; break;
    case 2: src = c->restir.sres.p; need = 24 * n; break;
    case 3: src = c->restir.radius.p; need = n; break;
    default:
      mtx_set_error("mtx_restir_state: which=%d not in 0..3", which);
      return MTX_E_ARG;
  }
  if (n_floats != need) {
    mtx_set_error("mtx_restir_state: need %llu floats, got %llu", (unsigned long long)need,
                  (unsigned long long)n_floats);
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(out, src, 4 * need, hipMemcpyDeviceToHost));
  return MTX_OK;
}

static int sample_rays_impl(mtx_ctx *c, const mtx_render_args *a, uint64_t n, const float *rays,
                            const uint32_t *lanes, uint32_t rng_skip, float *L, uint8_t *valid, bool dev);

int mtx_sample_rays(mtx_ctx *c, const mtx_render_args *a, uint64_t n, const float *rays, const uint32_t *lanes,
                    uint32_t rng_skip, float *L, uint8_t *valid) {
  return sample_rays_impl(c, a, n, rays, lanes, rng_skip, L, valid, false);
}

int mtx_sample_rays_dev(mtx_ctx *c, const mtx_render_args *a, uint64_t n, const float *rays, const uint32_t *lanes,
                        uint32_t rng_skip, float *L, uint8_t *valid) {
  if (c && n && (!rays || !lanes || !L || !valid)) {
    mtx_set_error("mtx_sample_rays_dev: null buffer");
    return MTX_E_ARG;
  }
  if (c && n) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = need_device(c, "mtx_sample_rays_dev", {rays, lanes, L, valid})) return rc;
  }
  return sample_rays_impl(c, a, n, rays, lanes, rng_skip, L, valid, true);
}

static int sample_rays_impl(mtx_ctx *c, const mtx_render_args *a, uint64_t n, const float *rays,
                            const uint32_t *lanes, uint32_t rng_skip, float *L, uint8_t *valid, bool dev) {
  int rc = check_args(c, a);
  if (rc) return rc;
  if (a->integrator == MTX_INT_PSSMLT_SIMPLE || a->integrator == MTX_INT_PSSMLT_PATH ||
      a->integrator == MTX_INT_RESTIR_GI) {
    mtx_set_error("mtx_sample_rays: PSSMLT / ReSTIR GI are render-level algorithms (use mtx_render)");
    return MTX_E_UNSUPPORTED;
  }
  if (n == 0) return MTX_OK;
  if (!rays || !lanes || !L || !valid) {
    mtx_set_error("mtx_sample_rays: null buffer");
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t chunk = a->chunk_paths ? a->chunk_paths : default_chunk(c, a, 1u, false);
  const uint32_t cap = (uint32_t)std::min<uint64_t>(n, chunk);
  Wave &w = c->wave[0];
  if ((rc = ensure_wave(c, w, cap, std::max<uint32_t>(a->max_depth, 1)))) return rc;
  const bool nrc_cache = a->integrator == MTX_INT_NRC && (a->flags & 4u);
  const bool nerad_render = a->integrator == MTX_INT_NERAD;
  if ((nrc_cache || nerad_render) && (rc = ensure_cache(c, w, cap))) return rc;
  if (!dev) {
    if ((rc = dalloc(c->scratch.s0, 24ull * cap))) return rc;
    if ((rc = dalloc(c->scratch.s1, 4ull * cap))) return rc;
    if ((rc = dalloc(c->scratch.s2, 12ull * cap))) return rc;
    if ((rc = dalloc(c->scratch.s3, 1ull * cap))) return rc;
  }
  mtxd::WaveBuffers b = views(c, w);
  Timer tm{c, false};
  uint64_t nt = 0, ns = 0;
  for (uint64_t off = 0; off < n; off += cap) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(cap, n - off);
    // the chunk's rays / lanes / outputs: the caller's device buffers, or the
    // context's staging copies of the host ones
    const float *d_rays = dev ? rays + 6 * off : (const float *)c->scratch.s0.p;
    const uint32_t *d_lanes = dev ? lanes + off : (const uint32_t *)c->scratch.s1.p;
    float *d_L = dev ? L + 3 * off : (float *)c->scratch.s2.p;
    uint8_t *d_valid = dev ? valid + off : (uint8_t *)c->scratch.s3.p;
    if (!dev) {
      HIP_TRY(hipMemcpyAsync(c->scratch.s0.p, rays + 6 * off, 24ull * m, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(c->scratch.s1.p, lanes + off, 4ull * m, hipMemcpyHostToDevice, c->stream));
    }
    mtxd::ChunkParams p{};
    p.integrator = a->integrator;
    p.max_depth = a->max_depth;
    p.rr_depth = a->rr_depth;
    p.seed = a->seed;
    p.spp = 1;
    p.spp_total = 1;
    p.width = c->scene.dev.camera.width;
    p.height = c->scene.dev.camera.height;
    p.n_paths = m;
    p.nrc_c = a->nrc_c;
    p.nrc_cache = nrc_cache ? 1u : 0u;
    HIP_TRY(reset_counters(b, std::max<uint32_t>(a->max_depth, 1), c->stream));
    if (nrc_cache || nerad_render) HIP_TRY(hipMemsetAsync(b.cq_count, 0, 4, c->stream));
    mtxd::launch_raygen_rays(c->scene.dev, b, p, d_rays, d_lanes, rng_skip, c->stream);
    run_bounces(c, w, b, p, tm, &nt, &ns);
    if ((nrc_cache || nerad_render) && (rc = run_cache(c, w, b, m, tm, nerad_render))) return rc;
    mtxd::launch_collect(b, p, d_L, d_valid, c->stream);
    HIP_TRY(hipGetLastError());
    if (!dev) {
      HIP_TRY(hipMemcpyAsync(L + 3 * off, c->scratch.s2.p, 12ull * m, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(valid + off, c->scratch.s3.p, m, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));  // the staging buffers are reused by the next chunk
    }
  }
  if (dev) HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

static int trace_impl(mtx_ctx *c, uint64_t n, const float *rays, int any_hit, uint32_t *hits, uint32_t *visits,
                      bool dev);

int mtx_trace(mtx_ctx *c, uint64_t n, const float *rays, int any_hit, uint32_t *hits, uint32_t *visits) {
  return trace_impl(c, n, rays, any_hit, hits, visits, false);
}

int mtx_trace_dev(mtx_ctx *c, uint64_t n, const float *rays, int any_hit, uint32_t *hits, uint32_t *visits) {
  if (c && rays && hits && n) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = need_device(c, "mtx_trace_dev", {rays, hits, visits})) return rc;
  }
  return trace_impl(c, n, rays, any_hit, hits, visits, true);
}

static int trace_impl(mtx_ctx *c, uint64_t n, const float *rays, int any_hit, uint32_t *hits, uint32_t *visits,
                      bool dev) {
  if (!c || !rays || !hits) {
    mtx_set_error("mtx_trace: null argument");
    return MTX_E_ARG;
  }
  if (!c->scene.live) {
    mtx_set_error("no scene uploaded");
    return MTX_E_NOSCENE;
  }
  if (any_hit < 0 || any_hit > 1) {
    mtx_set_error("mtx_trace: mode %d (0 closest hit, 1 any hit)", any_hit);
    return MTX_E_ARG;
  }
  if (n == 0) return MTX_OK;
  if (n >= (1ull << 31)) {
    mtx_set_error("mtx_trace: too many rays");
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  const size_t hit_words = any_hit == 1 ? n : 4 * n;
  if (dev) {
    mtxd::launch_trace_raw(c->scene.dev, (const float4 *)rays, (uint32_t)n, any_hit, hits, visits, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MTX_OK;
  }
  if ((rc = dalloc(c->scratch.s0, 32ull * n))) return rc;
  if ((rc = dalloc(c->scratch.s1, 4ull * hit_words))) return rc;
  if (visits && (rc = dalloc(c->scratch.s2, 8ull * n))) return rc;
  HIP_TRY(hipMemcpyAsync(c->scratch.s0.p, rays, 32ull * n, hipMemcpyHostToDevice, c->stream));
  mtxd::launch_trace_raw(c->scene.dev, (const float4 *)c->scratch.s0.p, (uint32_t)n, any_hit, (uint32_t *)c->scratch.s1.p,
                         visits ? (uint32_t *)c->scratch.s2.p : nullptr, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(hits, c->scratch.s1.p, 4ull * hit_words, hipMemcpyDeviceToHost, c->stream));
  if (visits) HIP_TRY(hipMemcpyAsync(visits, c->scratch.s2.p, 8ull * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

}  // extern "C"
