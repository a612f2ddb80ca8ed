// api.cpp — libmtx C ABI (include/mtx.h): device context, scene upload,
// wavefront scheduling and the primitive entry points.
//
// The host side of the replaced path: upstream SamplingIntegrator::render
// (transcribed at path.py:103-192) seeds the sampler over W*H*spp lanes,
// traces one Dr.Jit wavefront and splats into an ImageBlock. Here the same
// lanes are processed in chunks of whole pixels; each chunk runs
// raygen -> [trace, shade, shadow] x max_depth -> film stage 1 on one HIP
// stream with no host synchronisation (the persistent kernels read their
// queue lengths from device counters), then one film gather per call.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "mtx.h"
#include "mtx_core/bdpt.h"
#include "mtx_core/film.h"
#include "mtx_core/interaction.h"
#include "blocks.h"
#include "prims.h"
#include "refit.h"
#include "wavefront.h"

static thread_local char g_err[1024] = "";

void mtx_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      mtx_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return MTX_E_HIP;                                                                           \
    }                                                                                             \
  } while (0)

namespace {

// A device allocation and its owner: freed with the object that holds it
// (mtx_ctx_destroy frees every buffer of a context by deleting the context).
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() {
    if (p) hipFree(p);
  }
};

int dalloc(DevBuf &b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return MTX_OK;
  if (b.p) hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
  if (bytes == 0) return MTX_OK;
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    mtx_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    b.p = nullptr;
    return MTX_E_OOM;
  }
  b.bytes = bytes;
  return MTX_OK;
}

void dfree(DevBuf &b) {
  if (b.p) hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
}

template <class T>
int upload(DevBuf &b, const T *src, size_t count, hipStream_t st) {
  if (!src || count == 0) {
    dfree(b);
    return MTX_OK;
  }
  int rc = dalloc(b, count * sizeof(T));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(b.p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
  return MTX_OK;
}

}  // namespace

// The per-path planes of a wavefront (wavefront.h WaveBuffers): `sub`
// sub-planes of `elem`-byte entries, one wavefront capacity apart. The one
// statement of the layout: ensure_wave sizes a plane from it and plane_at
// places a sub-plane by it.
enum PlaneId { kRayO, kRayD, kThr, kL, kPrev, kMisc, kPos, kHit, kQ0, kQ1, kShadow, kNumPlanes };
struct PlaneDesc {
  uint32_t elem, sub;
};
constexpr PlaneDesc kPlanes[kNumPlanes] = {
    {16, 2},  // ray_o: bounce parity
    {16, 2},  // ray_d
    {16, 2},  // thr
    {16, 3},  // L: queue planes 0 / 1 + the per-path plane
    {16, 2},  // prev
    {16, 3},  // misc
    {8, 1},   // pos
    {16, 1},  // hit
    {4, 1},   // queue 0
    {4, 1},   // queue 1
    {16, 4},  // shadow: four planes of 16-B word groups
};

// One wavefront: its path state, queues, shadow records, counters and claim
// cursors, its traversal spill area, its NRC cache-query buffers and the
// stream its kernels run on. Wave 0 runs on the context's stream. Wave 1 is
// the second wavefront of a two-stream render (mtx_render's path / path-mis /
// nrc / simple integrators, ReSTIR GI's stage A): the film's chunks alternate
// between the two, so one chunk's kernels fill the GPU while the other's
// persistent trace launches drain their tails. Its stream and events are
// created by its first ensure_wave.
struct Wave {
  hipStream_t stream = nullptr;
  hipEvent_t start = nullptr, done = nullptr;  // wave 1: fork from / join into wave 0's stream
  DevBuf plane[kNumPlanes];
  DevBuf counters, xheads;  // queue counters, per-XCD claim cursors of the persistent trace kernels
  DevBuf stack_ovf;         // traversal stack entries beyond the LDS part (two waves' traces may run at once)
  DevBuf cq_p, cq_d, cq_t, cq_count, f_feat, f_out;  // NRC cache queries of a chunk, their features and outputs
  DevBuf cq_perm, cq_cursor;  // region-grouped query order (the Morton sort keeps its keys in cq_cursor)
  uint32_t capacity = 0;
};

struct mtx_ctx {
  int device = 0;
  int n_cu = 256;
  hipStream_t stream = nullptr;  // wave[0].stream is the same handle
  Wave wave[2];
  uint32_t *q_pinned = nullptr;  // per-chunk cache-query counts of a stats render (pinned, kQSlots)
  uint32_t streams = MTX_STREAMS;  // 1: every chunk on `stream` (MTX_STREAMS env: A/B)
  uint32_t streams_max_log2 = 27;  // two streams for renders of <= 2^this paths (MTX_STREAMS_MAX_LOG2: A/B)
  bool has_scene = false;
  // scene
  DevBuf shade_rec;  // per-triangle shading records
  // radiance field (mtx_field_upload)
  DevBuf field_table, field_frag, fq_p, fq_d;
  mtx::FieldEncoding field{};
  uint32_t field_hidden = 0;
  bool has_field = false;
  DevBuf field_w16;  // plain fp16 weights (training forward / backward)
  uint32_t field_n_in = 0, field_n_w = 0;
  uint64_t field_n_table = 0;  // fp16 table entries
  // field training (mtx_field_train_init): fp32 master parameters [table |
  // weights], Adam moments, gradients, per-batch scratch
  DevBuf tr_p, tr_m, tr_v, tr_g, tr_wpart, tr_loss, tr_out, tr_dfeat, tr_feat, tr_flag, tr_target;
  mtx_field_opt opt{};
  bool training = false;
  uint32_t adam_t = 0, good_steps = 0;
  float scale = 1.f;
  // neural radiosity surface tables (mtx_nerad_upload) and batch buffers
  DevBuf nr_shape_pmf, nr_shape_cdf, nr_tri_off, nr_tri_pmf, nr_tri_cdf, nr_tri_prim, nr_dists;
  mtx::NeradTables nr{};
  bool has_nerad = false;
  uint32_t scene_n_shapes = 0;
  uint32_t scene_n_materials = 0;  // bound of the material indices the building blocks take (blocks.hip)
  DevBuf nr_lhs, nr_qp, nr_qd, nr_Lrhs, nr_lanes;
  DevBuf nodes, tri, occ_nodes, occ_tri, tri_vidx, tri_shape, vpos, vnormal, vuv, shapes, materials, emitters, textures, texels, tables;
  mtxd::DevScene scene{};
  // vertex updates (mtx_scene_update_vertices): the occlusion tree's leaf
  // order -> scene triangle, and the levels of both trees: level l is nodes
  // [first[l], first[l + 1]) -- the builder's breadth-first layout -- or, for
  // trees whose levels are not contiguous, those entries of the device list.
  // The scratch (staged input, triangle and node boxes) is allocated by the
  // first update, not by upload.
  DevBuf occ_perm, lvl4_list, lvl8_list, rf_state, rf_tbox, rf_nbox, rf_vpos, rf_vnormal;
  std::vector<uint32_t> lvl4_first, lvl8_first;
  uint32_t scene_n_nodes = 0, scene_n_occ = 0, scene_n_verts = 0, scene_n_tables = 0;
  // mesh emitter tables of a vertex update (refit.h EmTables): lists and scratch, sized at upload
  DevBuf em_slots, em_blocks, em_state, em_pmf, em_cdf, em_bsum, em_bstat;
  mtxd::EmTables em_tables = {};
  // shared by both wavefronts
  DevBuf stats;
  DevBuf rs_heads;  // per-XCD claim cursors of k_trace_test
  DevBuf mlt_cur, mlt_L, mlt_prop, vpath, vprop;  // PSSMLT chain state
  DevBuf vpath_es, vprop_es;                       // pssmltpath emitter samples
  uint32_t mlt_capacity = 0, mlt_depth = 0, mlt_es_capacity = 0, mlt_es_depth = 0;
  // ReSTIR GI frame state (restirgi.py:217-226): kept across mtx_render calls
  DevBuf rs_samp[2], rs_tres, rs_sres, rs_radius, rs_hit, rs_dir, rs_emit, rs_rng, rs_rays, rs_count, rs_occ, rs_qM, rs_nbr, rs_xs, rs_ns;
  uint32_t rs_n = 0, rs_cur = 0, rs_pending_frame = 0;
  bool rs_valid = false, rs_pending_b = false;
  mtx_camera rs_prev_cam{};
  // film
  DevBuf contrib, film;
  // scratch for sample_rays / trace / primitives
  DevBuf s0, s1, s2, s3, s4, s5, s6;
  int trace_grid = 0, closest_grid = 0, shade_grid = 0;  // persistent grids: any hit, closest hit, shade
  size_t max_lds = 160 * 1024;  // LDS one workgroup may hold (gfx950: the CU's 160 KiB)
  // tuning knobs (environment, read at context creation): LDS stack entries
  // of the persistent traversal, chunk path order
  uint32_t lds_stack = mtxd::kLdsStack;
  uint32_t lds_top = MTX_LDS_TOP;          // closest-hit tree nodes kept in LDS per block (MTX_LDS_TOP env: A/B)
  uint32_t occ_lds_top = MTX_OCC_LDS_TOP;  // occlusion tree nodes kept in LDS per block (MTX_OCC_LDS_TOP)
  uint32_t occ_lds_stack = mtxd::kOccLdsStack;
  uint32_t trace_batch = 128;  // queue entries per claim (256: +0.6 % closest, +1 % at spp 32; 64: +5 %)
  uint32_t urefill = 24;  // refill a wave once 24 lanes are idle (16: closest +1.3 %, 32: +2 %; 4-wide BVH)
  uint32_t cam_urefill = 64;  // k_trace_camera (MTX_CAM_UREFILL): whole waves refill; a refill derives its camera rays
  uint32_t occ_urefill = 12;  // any hit on the 8-wide tree (MTX_OCC_UREFILL; 8-16 alike, 24: shadow +1 ms, 32/40: +2/+3 ms)
  uint32_t xcd_claim = 1;
  // ReSTIR GI: a band of at most this many paths runs its stage A in the
  // per-lane megakernel on one wavefront (MTX_MEGA_PATHS, 0 = off; default
  // 0xffffffff = twice the resident lanes of the megakernel's grid,
  // 2 x mega_grid x kShadeBlock)
  uint32_t mega_paths = 0xffffffffu;
  int mega_grid = 0;
  // such a band's whole stage A (raygen .. collect) in one per-lane launch
  // (kernels.hip k_rs_stage_a; MTX_RS_FUSED=0: raygen, trace, k_rs_begin, the
  // megakernel and k_rs_collect as separate launches)
  uint32_t rs_fused = 1;
  // NRC cache query order: MTX_CACHE_SORT=1 Morton-sorted (host sync; measured slower), 2 grouped
  // by region on the device with one eighth of the rows per XCD (field.hip)
  uint32_t cache_sort = MTX_CACHE_SORT;
  // NRC cache encoder: level-major lanes (field.hip k_field_encode_lm; MTX_ENCODE_LM=0: query-major)
  uint32_t encode_lm = MTX_ENCODE_LM;
  // NRC cache: encode + MLP + apply in one launch (field.hip k_field_cache_fused; MTX_CACHE_FUSED=0: three)
  uint32_t cache_fused = 1;
  DevBuf cq_ws;  // sort workspace of the Morton order
  std::vector<hipEvent_t> events;
  hipEvent_t prim_ev[2] = {nullptr, nullptr};
  double last_device_ms = 0.0;
};

extern "C" {

int mtx_abi_version(void) { return MTX_ABI_VERSION; }

// Diagnostic export (not in mtx.h): the shade kernel's per-phase stamp sums of
// an MTX_DIAG_STAMPS build (tools/shade_stamps.py); returns the segment
// count, or -1 in production builds.
int mtx_diag_shade_stamps(unsigned long long *out) { return mtxd::shade_stamps(out); }

const char *mtx_last_error(void) { return g_err; }

int mtx_ctx_create(int hip_device, mtx_ctx **out) {
  if (!out) {
    mtx_set_error("mtx_ctx_create: out is NULL");
    return MTX_E_ARG;
  }
  *out = nullptr;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (hip_device < 0 || hip_device >= n) {
    mtx_set_error("mtx_ctx_create: device %d out of range (%d devices)", hip_device, n);
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(hip_device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, hip_device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    mtx_set_error("mtx_ctx_create: device %d is %s, libmtx is built for gfx950", hip_device, prop.gcnArchName);
    return MTX_E_UNSUPPORTED;
  }
  mtx_ctx *c = new mtx_ctx();
  c->device = hip_device;
  c->n_cu = prop.multiProcessorCount;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    mtx_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
    return MTX_E_HIP;
  }
  c->wave[0].stream = c->stream;
  // Persistent grids: every CU filled to the kernels' occupancy (the trace
  // grid is recomputed per scene: its LDS stack depends on the BVH depth).
  c->trace_grid = c->closest_grid = c->n_cu * 8;
  c->shade_grid = c->n_cu * mtxd::shade_blocks_per_cu();
  {
    // a gfx950 workgroup may hold the CU's whole 160 KiB of LDS (the attribute
    // may report the 64 KiB that needs no opt-in; the kernels launch above it)
    int v = 0;
    c->max_lds = 160 * 1024;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, hip_device) == hipSuccess &&
        (size_t)v > c->max_lds)
      c->max_lds = (size_t)v;
  }
  if (const char *e = getenv("MTX_LDS_STACK")) c->lds_stack = std::max(1, std::min(MTX_BVH_MAX_DEPTH + 1, atoi(e)));
  if (const char *e = getenv("MTX_LDS_TOP")) c->lds_top = (uint32_t)std::max(0, std::min(256, atoi(e)));
  if (const char *e = getenv("MTX_OCC_LDS_TOP")) c->occ_lds_top = (uint32_t)std::max(0, std::min(192, atoi(e)));
  if (const char *e = getenv("MTX_OCC_LDS_STACK"))
    c->occ_lds_stack = std::max(1, std::min(MTX_BVH_MAX_DEPTH + 1, atoi(e)));
  if (const char *e = getenv("MTX_STREAMS_MAX_LOG2")) c->streams_max_log2 = (uint32_t)std::max(16, std::min(31, atoi(e)));
  if (const char *e = getenv("MTX_STREAMS")) c->streams = (uint32_t)std::max(1, std::min(2, atoi(e)));
  if (const char *e = getenv("MTX_TRACE_BATCH")) c->trace_batch = (uint32_t)std::max(1, std::min(1 << 16, atoi(e)));
  if (const char *e = getenv("MTX_UREFILL")) c->urefill = (uint32_t)std::max(1, std::min(64, atoi(e)));
  if (const char *e = getenv("MTX_CAM_UREFILL")) c->cam_urefill = (uint32_t)std::max(1, std::min(64, atoi(e)));
  if (const char *e = getenv("MTX_OCC_UREFILL")) c->occ_urefill = (uint32_t)std::max(1, std::min(64, atoi(e)));
  if (const char *e = getenv("MTX_XCD_CLAIM")) c->xcd_claim = atoi(e) != 0;
  if (const char *e = getenv("MTX_RS_FUSED")) c->rs_fused = atoi(e) ? 1u : 0u;
  if (const char *e = getenv("MTX_MEGA_PATHS")) c->mega_paths = (uint32_t)strtoul(e, nullptr, 0);
  if (const char *e = getenv("MTX_CACHE_FUSED")) c->cache_fused = atoi(e) ? 1u : 0u;
  if (const char *e = getenv("MTX_ENCODE_LM")) c->encode_lm = atoi(e) ? 1u : 0u;
  if (const char *e = getenv("MTX_CACHE_SORT")) c->cache_sort = (uint32_t)std::max(0, std::min(2, atoi(e)));
  *out = c;
  return MTX_OK;
}

void mtx_ctx_destroy(mtx_ctx *c) {
  if (!c) return;
  hipSetDevice(c->device);
  // both streams idle before anything they use goes; wave[0].stream is
  // c->stream and is destroyed once
  for (Wave &w : c->wave)
    if (w.stream) hipStreamSynchronize(w.stream);
  Wave &w1 = c->wave[1];
  if (w1.start) hipEventDestroy(w1.start);
  if (w1.done) hipEventDestroy(w1.done);
  if (w1.stream) hipStreamDestroy(w1.stream);
  for (hipEvent_t ev : c->events) hipEventDestroy(ev);
  if (c->q_pinned) hipHostFree(c->q_pinned);
  for (hipEvent_t ev : c->prim_ev)
    if (ev) hipEventDestroy(ev);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;  // every DevBuf member frees its memory (the device is still current)
}

// Caller-supplied occlusion trees: their triangle records must be the
// scene's (a stale pair would answer shadow rays against other geometry).
// With d->occ_perm the claimed correspondence is checked record by record
// and as a permutation; without it the records of both arrays are sorted
// and matched. perm[i] = scene triangle of occlusion triangle i.
static int occ_match(const mtx_scene_desc *d, std::vector<uint32_t> &perm) {
  const uint32_t n = d->n_tris;
  auto rec = [](const float *g, uint32_t i, int w) {
    uint32_t x;
    memcpy(&x, g + 12 * (size_t)i + 4 * (w / 3) + (w % 3), 4);
    return x;
  };
  auto same = [&](uint32_t i, uint32_t j) {
    for (int w = 0; w < 9; ++w)
      if (rec(d->occ_tri_geom, i, w) != rec(d->tri_geom, j, w)) return false;
    return true;
  };
  perm.assign(n, 0u);
  if (d->occ_perm) {
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t j = d->occ_perm[i];
      if (j >= n || seen[j] || !same(i, j)) {
        mtx_set_error("mtx_scene_upload: occ_perm[%u] = %u does not map occlusion triangle %u to an unused scene "
                      "triangle with the same record",
                      i, j, i);
        return MTX_E_ARG;
      }
      seen[j] = 1;
      perm[i] = j;
    }
    return MTX_OK;
  }
  std::vector<uint32_t> a(n), b(n);
  for (uint32_t i = 0; i < n; ++i) a[i] = b[i] = i;
  auto less = [&](const float *g) {
    return [&, g](uint32_t x, uint32_t y) {
      for (int w = 0; w < 9; ++w) {
        const uint32_t u = rec(g, x, w), v = rec(g, y, w);
        if (u != v) return u < v;
      }
      return x < y;
    };
  };
  std::sort(a.begin(), a.end(), less(d->occ_tri_geom));
  std::sort(b.begin(), b.end(), less(d->tri_geom));
  for (uint32_t k = 0; k < n; ++k) {
    if (!same(a[k], b[k])) {
      mtx_set_error("mtx_scene_upload: occ_tri_geom is not a permutation of tri_geom (occ_nodes / occ_tri_geom "
                    "must come from mtx_bvh_build_occlusion over this tri_geom)");
      return MTX_E_ARG;
    }
    perm[a[k]] = b[k];
  }
  return MTX_OK;
}

// Levels of a tree from its nodes' levels (0xffffffff: unreachable): level l
// = [first[l], first[l + 1]). The builder lays both trees out breadth-first,
// so a level is a contiguous node range and no list is kept; for any other
// tree `list` holds the reachable nodes grouped by level.
static int upload_levels(const std::vector<uint32_t> &level, uint32_t depth, std::vector<uint32_t> &first,
                         DevBuf &list, hipStream_t st) {
  first.assign((size_t)depth + 1, 0u);
  bool contiguous = true;
  uint32_t prev = 0;
  for (uint32_t l : level) {
    if (l >= depth) {
      contiguous = false;
      continue;
    }
    ++first[l + 1];
    contiguous = contiguous && l >= prev;
    prev = l;
  }
  for (uint32_t l = 0; l < depth; ++l) first[l + 1] += first[l];
  if (contiguous) {
    dfree(list);
    return MTX_OK;
  }
  std::vector<uint32_t> idx(first[depth]), cursor(first.begin(), first.end() - 1);
  for (size_t i = 0; i < level.size(); ++i)
    if (level[i] < depth) idx[cursor[level[i]]++] = (uint32_t)i;
  int rc = upload(list, idx.data(), idx.size(), st);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(st));  // idx is freed at scope exit
  return MTX_OK;
}

// Mesh area emitters (mtx.h mtx_emitter: a zero normal): the kernels index
// `tables` and the triangles from the record's words, so every word is
// checked here, on the host, before anything reaches the device. Called once
// tri_shape and the shapes' emitter references are known to be in range.
static int check_mesh_emitters(const mtx_scene_desc *d) {
  std::vector<uint32_t> listed;  // per triangle: times a mesh record lists it
  for (uint32_t i = 0; i < d->n_emitters; ++i) {
    const mtx_emitter &e = d->emitters[i];
    if (!(e.normal[0] == 0.f && e.normal[1] == 0.f && e.normal[2] == 0.f)) continue;  // a rectangle
    const uint64_t n = e.mesh_count;
    if (e.mesh_kind != MTX_EMITTER_MESH || n == 0) {
      mtx_set_error("mtx_scene_upload: emitter %u has a zero normal but is no mesh record (kind %u, %u entries)", i,
                    e.mesh_kind, e.mesh_count);
      return MTX_E_ARG;
    }
    if (!d->tables || (uint64_t)e.mesh_offset + 3 * n > d->n_tables) {
      mtx_set_error("mtx_scene_upload: mesh emitter %u: table range [%u, +3 x %u) leaves the %u table floats", i,
                    e.mesh_offset, e.mesh_count, d->n_tables);
      return MTX_E_ARG;
    }
    const float *pmf = d->tables + e.mesh_offset, *cdf = pmf + n;
    if (!(e.mesh_sum > 0.f) || !std::isfinite(e.mesh_sum) || e.mesh_sum != cdf[n - 1] || !(e.mesh_norm > 0.f) ||
        !std::isfinite(e.mesh_norm) || !(e.inv_area > 0.f) || !std::isfinite(e.inv_area)) {
      mtx_set_error("mtx_scene_upload: mesh emitter %u: sum %g (cdf ends at %g), normalization %g, inv_area %g: "
                    "need a positive finite sum equal to the last cdf entry", i, (double)e.mesh_sum,
                    (double)cdf[n - 1], (double)e.mesh_norm, (double)e.inv_area);
      return MTX_E_ARG;
    }
    uint32_t lo = 0xffffffffu, hi = 0;
    for (uint64_t k = 0; k < n; ++k) {
      if (!(pmf[k] >= 0.f) || !(cdf[k] >= (k ? cdf[k - 1] : 0.f))) {
        mtx_set_error("mtx_scene_upload: mesh emitter %u: entry %llu has a negative pmf or a decreasing cdf", i,
                      (unsigned long long)k);
        return MTX_E_ARG;
      }
      if (pmf[k] > 0.f) {
        if (lo == 0xffffffffu) lo = (uint32_t)k;
        hi = (uint32_t)k;
      }
    }
    if (lo != e.mesh_valid_lo || hi != e.mesh_valid_hi) {
      mtx_set_error("mtx_scene_upload: mesh emitter %u: valid range [%u, %u] given, the pmf's is [%u, %u]", i,
                    e.mesh_valid_lo, e.mesh_valid_hi, lo, hi);
      return MTX_E_ARG;
    }
    if (listed.empty()) listed.assign(d->n_tris, 0u);
    for (uint64_t k = 0; k < n; ++k) {
      uint32_t prim;
      memcpy(&prim, cdf + n + k, 4);
      if (prim >= d->n_tris) {
        mtx_set_error("mtx_scene_upload: mesh emitter %u: entry %llu names triangle %u of %u", i,
                      (unsigned long long)k, prim, d->n_tris);
        return MTX_E_ARG;
      }
      if (d->shapes[d->tri_shape[prim]].emitter != (int32_t)i || listed[prim]++) {
        mtx_set_error("mtx_scene_upload: mesh emitter %u: entry %llu names triangle %u, which %s", i,
                      (unsigned long long)k, prim,
                      listed[prim] > 1 ? "is listed twice" : "belongs to a shape with another emitter or none");
        return MTX_E_ARG;
      }
    }
  }
  for (uint32_t t = 0; t < d->n_tris; ++t) {
    const mtx_shape &sh = d->shapes[d->tri_shape[t]];
    if (sh.emitter < 0) continue;
    const mtx_emitter &e = d->emitters[sh.emitter];
    if (!(e.normal[0] == 0.f && e.normal[1] == 0.f && e.normal[2] == 0.f)) continue;
    if (listed.empty() || listed[t] != 1) {
      mtx_set_error("mtx_scene_upload: mesh emitter %d does not list triangle %u of its shape", sh.emitter, t);
      return MTX_E_ARG;
    }
    if (!(sh.flags & 1u)) {
      mtx_set_error("mtx_scene_upload: shape %u carries mesh emitter %d and must be shaded with face normals "
                    "(flag bit 0)", d->tri_shape[t], sh.emitter);
      return MTX_E_ARG;
    }
  }
  return MTX_OK;
}

int mtx_scene_upload(mtx_ctx *c, const mtx_scene_desc *d) {
  if (!c || !d) {
    mtx_set_error("mtx_scene_upload: null argument");
    return MTX_E_ARG;
  }
  if (!d->nodes || !d->tri_geom || !d->tri_vidx || !d->tri_shape || !d->vpos || !d->shapes || !d->materials ||
      d->n_tris == 0 || d->n_nodes == 0 || (d->n_emitters == 0 && !d->has_env) || (d->n_emitters && !d->emitters)) {
    mtx_set_error("mtx_scene_upload: incomplete scene (need geometry, BVH, shapes, materials, >=1 emitter)");
    return MTX_E_ARG;
  }
  // The occlusion BVH: given, or built here over the triangle records.
  const bool occ_given = d->occ_nodes && d->occ_tri_geom && d->n_occ_nodes > 0;
  if (!occ_given && (d->occ_nodes || d->occ_tri_geom)) {
    mtx_set_error("mtx_scene_upload: occ_nodes and occ_tri_geom go together (both NULL: built here)");
    return MTX_E_ARG;
  }
  std::vector<int32_t> occ_nodes_v;
  std::vector<float> occ_geom_v;
  std::vector<uint32_t> occ_perm_v;
  const int32_t *occ_nodes = d->occ_nodes;
  const float *occ_geom = d->occ_tri_geom;
  uint32_t n_occ = d->n_occ_nodes;
  int rc = 0;
  if (!occ_given) {
    occ_nodes_v.resize(((size_t)d->n_tris + 1) * MTX_OCC_NODE_WORDS);
    occ_geom_v.resize(12 * (size_t)d->n_tris);
    occ_perm_v.resize(d->n_tris);
    if ((rc = mtx_bvh_build_occlusion(d->tri_geom, d->n_tris, occ_nodes_v.data(), &n_occ, occ_geom_v.data(),
                                      occ_perm_v.data(), nullptr)))
      return rc;
    occ_nodes = occ_nodes_v.data();
    occ_geom = occ_geom_v.data();
  } else if ((rc = occ_match(d, occ_perm_v))) {  // given trees: their records must be this scene's
    return rc;
  }
  // Validate both trees (mtx.h) on the host so that no kernel can read out
  // of bounds, and find their depths (stack entries: a 4-wide level pushes
  // at most 3 node references, an 8-wide level one node group); also
  // rejects cycles.
  uint32_t bvh_depth = 0, occ_depth = 0;
  // level of every reachable node (vertex updates refit level by level)
  std::vector<uint32_t> level4(d->n_nodes, 0xffffffffu), level8(n_occ, 0xffffffffu);
  {
    std::vector<std::pair<int32_t, uint32_t>> todo{{0, 0u}};
    uint64_t visited = 0;
    while (!todo.empty()) {
      auto [nd, dep] = todo.back();
      todo.pop_back();
      level4[nd] = dep;
      bvh_depth = std::max(bvh_depth, dep + 1);
      if (++visited > d->n_nodes || dep >= MTX_BVH_MAX_DEPTH) {
        mtx_set_error("mtx_scene_upload: BVH is not a tree of depth <= %d", MTX_BVH_MAX_DEPTH);
        return MTX_E_ARG;
      }
      const int32_t *w = d->nodes + MTX_BVH_NODE_WORDS * (size_t)nd;
      const uint32_t nch = (uint32_t)w[3] >> 24;
      if (nch < 1 || nch > MTX_BVH_WIDTH) {
        mtx_set_error("mtx_scene_upload: node %d has %u children", nd, nch);
        return MTX_E_ARG;
      }
      for (uint32_t k = 0; k < nch; ++k) {
        const int32_t ch = w[4 + k];
        if (ch >= 0) {
          if ((uint32_t)ch >= d->n_nodes) {
            mtx_set_error("mtx_scene_upload: node %d child %d out of range", nd, ch);
            return MTX_E_ARG;
          }
          todo.push_back({ch, dep + 1});
        } else {
          uint32_t x = (uint32_t)(~ch), first = x >> 3, cnt = (x & 7u) + 1;
          if ((uint64_t)first + cnt > d->n_tris) {
            mtx_set_error("mtx_scene_upload: leaf [%u,+%u) exceeds %u triangles", first, cnt, d->n_tris);
            return MTX_E_ARG;
          }
        }
      }
    }
  }
  {
    std::vector<std::pair<uint32_t, uint32_t>> todo{{0u, 0u}};
    uint64_t visited = 0;
    while (!todo.empty()) {
      auto [nd, dep] = todo.back();
      todo.pop_back();
      level8[nd] = dep;
      occ_depth = std::max(occ_depth, dep + 1);
      if (++visited > n_occ || dep >= MTX_BVH_MAX_DEPTH) {
        mtx_set_error("mtx_scene_upload: occlusion BVH is not a tree of depth <= %d", MTX_BVH_MAX_DEPTH);
        return MTX_E_ARG;
      }
      const uint32_t *w = reinterpret_cast<const uint32_t *>(occ_nodes) + MTX_OCC_NODE_WORDS * (size_t)nd;
      const uint32_t imask = w[3] >> 24, child_base = w[4], tri_base = w[5];
      uint32_t inner = 0;
      for (uint32_t sl = 0; sl < MTX_OCC_WIDTH; ++sl) {
        const uint32_t m = (w[6 + (sl >> 2)] >> (8 * (sl & 3))) & 0xffu;
        const bool is_inner = (imask >> sl) & 1u;
        if (is_inner) {
          const uint32_t ch = child_base + inner++;
          if (m != (0x20u | (24u + sl)) || ch >= n_occ) {
            mtx_set_error("mtx_scene_upload: occlusion node %u slot %u: bad inner child", nd, sl);
            return MTX_E_ARG;
          }
          todo.push_back({ch, dep + 1});
        } else if (m != 0) {
          const uint32_t cb = m >> 5, off = m & 31u, cnt = cb == 1 ? 1u : cb == 3 ? 2u : cb == 7 ? 3u : 0u;
          if (cnt == 0 || off + cnt > 24 || (uint64_t)tri_base + off + cnt > d->n_tris) {
            mtx_set_error("mtx_scene_upload: occlusion node %u slot %u: bad leaf", nd, sl);
            return MTX_E_ARG;
          }
        }
      }
    }
  }
  for (uint64_t i = 0; i < 3ull * d->n_tris; ++i)
    if (d->tri_vidx[i] >= d->n_verts) {
      mtx_set_error("mtx_scene_upload: vertex index out of range");
      return MTX_E_ARG;
    }
  for (uint32_t i = 0; i < d->n_tris; ++i)
    if (d->tri_shape[i] >= d->n_shapes) {
      mtx_set_error("mtx_scene_upload: shape index out of range");
      return MTX_E_ARG;
    }
  for (uint32_t i = 0; i < d->n_shapes; ++i) {
    if (d->shapes[i].material >= d->n_materials ||
        (d->shapes[i].emitter >= 0 && (uint32_t)d->shapes[i].emitter >= d->n_emitters)) {
      mtx_set_error("mtx_scene_upload: shape %u references a missing material/emitter", i);
      return MTX_E_ARG;
    }
  }
  if ((rc = check_mesh_emitters(d))) return rc;
  for (uint32_t i = 0; i < d->n_materials; ++i) {
    const mtx_material &m = d->materials[i];
    if (m.tex >= 0) {
      if ((uint32_t)m.tex >= d->n_textures || !d->textures) {
        mtx_set_error("mtx_scene_upload: material %u texture out of range", i);
        return MTX_E_ARG;
      }
      const mtx_texture &t = d->textures[m.tex];
      if (t.offset + 3ull * t.width * t.height > d->n_texels || t.width == 0 || t.height == 0) {
        mtx_set_error("mtx_scene_upload: texture %d exceeds texel buffer", m.tex);
        return MTX_E_ARG;
      }
    }
    if (m.type == MTX_MAT_ROUGHPLASTIC && (m.table < 0 || (uint32_t)m.table + MTX_ROUGH_TRANSMITTANCE_RES > d->n_tables)) {
      mtx_set_error("mtx_scene_upload: roughplastic material %u has no transmittance table", i);
      return MTX_E_ARG;
    }
  }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if ((rc = upload(c->nodes, d->nodes, (size_t)MTX_BVH_NODE_WORDS * d->n_nodes, st))) return rc;
  if ((rc = upload(c->occ_nodes, occ_nodes, (size_t)MTX_OCC_NODE_WORDS * n_occ, st))) return rc;
  for (int tree = 0; tree < 2; ++tree) {
    // device triangles packed to 36 B (the ABI's 48-B records carry 3 pad
    // words): 3.6 instead of 2.7 triangles per 128-B line, same load count
    const float *src = tree ? occ_geom : d->tri_geom;
    std::vector<float> g9(9ull * d->n_tris);
    for (size_t i = 0; i < d->n_tris; ++i)
      for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) g9[9 * i + 3 * k + j] = src[12 * i + 4 * k + j];
    if ((rc = upload(tree ? c->occ_tri : c->tri, g9.data(), g9.size(), st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // g9 is freed at scope exit
  }
  if ((rc = upload(c->occ_perm, occ_perm_v.data(), (size_t)d->n_tris, st))) return rc;
  if ((rc = upload_levels(level4, bvh_depth, c->lvl4_first, c->lvl4_list, st))) return rc;
  if ((rc = upload_levels(level8, occ_depth, c->lvl8_first, c->lvl8_list, st))) return rc;
  c->scene_n_nodes = d->n_nodes;
  c->scene_n_occ = n_occ;
  c->scene_n_verts = d->n_verts;
  if ((rc = upload(c->tri_vidx, d->tri_vidx, 3ull * d->n_tris, st))) return rc;
  if ((rc = upload(c->tri_shape, d->tri_shape, (size_t)d->n_tris, st))) return rc;
  if ((rc = upload(c->vpos, d->vpos, 3ull * d->n_verts, st))) return rc;
  if ((rc = upload(c->vnormal, d->vnormal, d->vnormal ? 3ull * d->n_verts : 0, st))) return rc;
  if ((rc = upload(c->vuv, d->vuv, d->vuv ? 2ull * d->n_verts : 0, st))) return rc;
  if ((rc = upload(c->shapes, d->shapes, d->n_shapes, st))) return rc;
  c->scene_n_shapes = d->n_shapes;
  c->has_nerad = false;  // surface tables belong to the previous scene
  if ((rc = upload(c->materials, d->materials, d->n_materials, st))) return rc;
  if ((rc = upload(c->emitters, d->emitters, d->n_emitters, st))) return rc;
  if ((rc = upload(c->textures, d->textures, d->n_textures, st))) return rc;
  if ((rc = upload(c->texels, d->texels, d->n_texels, st))) return rc;
  if ((rc = upload(c->tables, d->tables, d->n_tables, st))) return rc;
  c->scene_n_tables = d->n_tables;
  {
    // what a vertex update needs to rebuild the mesh emitters' tables
    std::vector<mtxd::EmSlot> slots;
    std::vector<mtxd::EmBlock> blks;
    uint64_t flat = 0;
    for (uint32_t i = 0; i < d->n_emitters; ++i) {
      const mtx_emitter &e = d->emitters[i];
      if (!(e.normal[0] == 0.f && e.normal[1] == 0.f && e.normal[2] == 0.f)) continue;  // a rectangle
      mtxd::EmSlot sl = {};
      sl.emitter = i;
      sl.offset = e.mesh_offset;
      sl.count = e.mesh_count;
      sl.flat = (uint32_t)flat;
      sl.block = (uint32_t)blks.size();
      for (uint64_t first = 0; first < e.mesh_count; first += mtxd::kEmBlock)
        blks.push_back({(uint32_t)slots.size(), (uint32_t)first});
      slots.push_back(sl);
      flat += e.mesh_count;  // <= n_tris: every triangle is listed at most once (check_mesh_emitters)
    }
    mtxd::EmTables &t = c->em_tables;
    t = {};
    t.n_slots = (uint32_t)slots.size();
    t.n_blocks = (uint32_t)blks.size();
    if ((rc = upload(c->em_slots, slots.data(), slots.size(), st))) return rc;
    if ((rc = upload(c->em_blocks, blks.data(), blks.size(), st))) return rc;
    if ((rc = dalloc(c->em_state, 4ull * mtxd::EM_WORDS * slots.size()))) return rc;
    if ((rc = dalloc(c->em_pmf, 4ull * flat))) return rc;
    if ((rc = dalloc(c->em_cdf, 4ull * flat))) return rc;
    if ((rc = dalloc(c->em_bsum, 8ull * blks.size()))) return rc;
    if ((rc = dalloc(c->em_bstat, 16ull * blks.size()))) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // slots and blks are freed at scope exit
    t.slots = (const mtxd::EmSlot *)c->em_slots.p;
    t.blocks = (const mtxd::EmBlock *)c->em_blocks.p;
    t.state = (uint32_t *)c->em_state.p;
    t.pmf = (float *)c->em_pmf.p;
    t.cdf = (float *)c->em_cdf.p;
    t.bsum = (double *)c->em_bsum.p;
    t.bstat = (uint32_t *)c->em_bstat.p;
  }
  {
    // per-triangle shading records (compute_si_dev)
    std::vector<float> rec(32 * (size_t)d->n_tris, 0.f);
    for (uint32_t t = 0; t < d->n_tris; ++t) {
      float *r = &rec[32 * (size_t)t];
      const mtx_shape &sh = d->shapes[d->tri_shape[t]];
      const uint32_t use_n = (!(sh.flags & 1u) && d->vnormal) ? 1u : 0u;
      const uint32_t use_uv = ((sh.flags & 2u) && d->vuv) ? 2u : 0u;
      for (int k = 0; k < 3; ++k) {
        const uint32_t vi = d->tri_vidx[3 * (size_t)t + k];
        for (int a = 0; a < 3; ++a) r[4 * k + a] = d->vpos[3 * (size_t)vi + a];
        if (use_n)
          for (int a = 0; a < 3; ++a) r[12 + 4 * k + a] = d->vnormal[3 * (size_t)vi + a];
        if (use_uv) {
          r[24 + 2 * k] = d->vuv[2 * (size_t)vi];
          r[24 + 2 * k + 1] = d->vuv[2 * (size_t)vi + 1];
        }
      }
      // bits 8..12: shading class of the material (read by no kernel since
      // the block-level material sort was measured slower and removed)
      const mtx_material &m = d->materials[sh.material];
      const uint32_t cls = 1u + ((m.type & 7u) << 2 | (m.tex >= 0 ? 2u : 0u) | ((m.flags & MTX_MF_MASK) ? 1u : 0u));
      const uint32_t mat = sh.material, fl = use_n | use_uv | (cls << 8);
      const int32_t em = sh.emitter;
      memcpy(&r[3], &mat, 4);
      memcpy(&r[7], &em, 4);
      memcpy(&r[11], &fl, 4);
    }
    if ((rc = upload(c->shade_rec, rec.data(), rec.size(), st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // rec is freed at scope exit
  }
  HIP_TRY(hipStreamSynchronize(st));
  mtxd::DevScene &s = c->scene;
  s.nodes = (const int4 *)c->nodes.p;
  s.tri = (const float *)c->tri.p;
  s.occ_nodes = (const int4 *)c->occ_nodes.p;
  s.occ_tri = (const float *)c->occ_tri.p;
  s.tri_vidx = (const uint32_t *)c->tri_vidx.p;
  s.tri_shape = (const uint32_t *)c->tri_shape.p;
  s.vpos = (const float *)c->vpos.p;
  s.vnormal = (const float *)c->vnormal.p;
  s.vuv = (const float *)c->vuv.p;
  s.shapes = (const mtx_shape *)c->shapes.p;
  s.shade_rec = (const float4 *)c->shade_rec.p;
  s.materials = (const mtx_material *)c->materials.p;
  s.emitters = (const mtx_emitter *)c->emitters.p;
  s.textures = (const mtx_texture *)c->textures.p;
  s.texels = (const float *)c->texels.p;
  s.tables = (const float *)c->tables.p;
  s.n_tris = d->n_tris;
  s.n_emitters = d->n_emitters;
  c->scene_n_materials = d->n_materials;
  s.camera = d->camera;
  s.has_env = d->has_env ? 1u : 0u;
  for (int k = 0; k < 3; ++k) s.env_radiance[k] = d->env_radiance[k];
  mtx::env_bsphere(d->vpos, d->n_verts, s.env_center, &s.env_radius);
  // LDS per trace block (8 blocks of 256 threads per CU fill the 160 KB):
  // closest hit 16 x 4-B stack entries per lane + 64 nodes of 64 B,
  // occlusion 8 x 8-B entries + 48 nodes of 80 B
  s.stack_entries = 3 * bvh_depth + 1;
  s.lds_entries = std::min<uint32_t>(s.stack_entries, c->lds_stack);
  s.lds_top = std::min<uint32_t>(d->n_nodes, c->lds_top);
  s.occ_stack_entries = occ_depth + 1;
  s.occ_lds_entries = std::min<uint32_t>(s.occ_stack_entries, c->occ_lds_stack);
  s.occ_lds_top = std::min<uint32_t>(n_occ, c->occ_lds_top);
  s.trace_batch = c->trace_batch;
  s.urefill = c->urefill;
  s.cam_urefill = c->cam_urefill;
  s.occ_urefill = c->occ_urefill;
  s.xcd_claim = c->xcd_claim;
  c->trace_grid = c->n_cu * mtxd::trace_blocks_per_cu(s);
  c->closest_grid = c->n_cu * mtxd::closest_blocks_per_cu(s);
  c->mega_grid = c->n_cu * mtxd::mega_blocks_per_cu(s);
  s.ovf_threads = (uint32_t)std::max(c->trace_grid, c->closest_grid) * mtxd::kTraceBlock;
  if ((rc = dalloc(c->wave[0].stack_ovf, mtxd::stack_ovf_bytes(s)))) return rc;  // wave 1's: ensure_wave
  s.stack_ovf = c->wave[0].stack_ovf.p;
  c->has_scene = true;
  return MTX_OK;
}

}  // extern "C"

namespace {

// Default wavefront: up to 256 Mi paths (~328 B of state each, ~82 GB) so a
// 1280x720 spp=256 frame runs as one chunk (fewer queue tails), bounded by
// 40 % of the free HBM.
constexpr uint32_t kDefaultChunk = 1u << 28;
constexpr size_t kPathStateBytes = 328;
// per NRC cache / field query: each of the three query planes (p, d, T),
// the fp16 feature row, the RGB output
constexpr size_t kQueryBytes = 16, kFeatBytes = 128, kOutBytes = 12;
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
  if ((rc = dalloc(w.stack_ovf, mtxd::stack_ovf_bytes(c->scene)))) return rc;
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
  b.mlt_cur = (float4 *)c->mlt_cur.p;
  b.mlt_L = (float4 *)c->mlt_L.p;
  b.mlt_prop = (float2 *)c->mlt_prop.p;
  b.vpath = (float4 *)c->vpath.p;
  b.vprop = (float4 *)c->vprop.p;
  b.vpath_es = (float2 *)c->vpath_es.p;
  b.vprop_es = (float2 *)c->vprop_es.p;
  b.cq_p = (float4 *)w.cq_p.p;  // null unless ensure_cache
  b.cq_d = (float4 *)w.cq_d.p;
  b.cq_t = (float4 *)w.cq_t.p;
  b.cq_count = (uint32_t *)w.cq_count.p;
  return b;
}

// The scene as wave `w` traces it: the context's, with the wave's spill area.
mtxd::DevScene wave_scene(const mtx_ctx *c, const Wave &w) {
  mtxd::DevScene s = c->scene;
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
  if (emitter_samples && (!c->vpath_es.p || c->mlt_es_capacity != wc || max_depth > c->mlt_es_depth)) {
    if ((rc = dalloc(c->vpath_es, 8 * wc * max_depth))) return rc;
    if ((rc = dalloc(c->vprop_es, 8 * wc * max_depth))) return rc;
    c->mlt_es_capacity = wc;
    c->mlt_es_depth = max_depth;
  }
  if (cap > c->mlt_capacity || max_depth > c->mlt_depth || c->mlt_capacity != wc) {
    // vertex buffers are indexed [depth * wavefront capacity + chain]
    if ((rc = dalloc(c->mlt_cur, 16 * wc))) return rc;
    if ((rc = dalloc(c->mlt_L, 16 * wc))) return rc;
    if ((rc = dalloc(c->mlt_prop, 8 * wc))) return rc;
    if ((rc = dalloc(c->vpath, 16 * wc * max_depth))) return rc;
    if ((rc = dalloc(c->vprop, 16 * wc * max_depth))) return rc;
    c->mlt_capacity = wc;
    c->mlt_depth = max_depth;
  }
  return MTX_OK;
}

// Wave `w`'s NRC radiance-cache buffers for `cap` paths (queries <= paths).
// Callers ensure wave 0's first, so a missing field is refused before
// anything is allocated for either wave.
int ensure_cache(mtx_ctx *c, Wave &w, uint32_t cap) {
  int rc;
  if (!c->has_field) {
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
  if (!c->has_scene) {
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

// Event-pair timer per kernel class.
struct Timer {
  mtx_ctx *c;
  bool on;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs[6];  // trace, shadow, shade, all, encode, mlp
  uint64_t cache_queries = 0;
  uint32_t q_used = 0;  // chunk query counts copied (asynchronously) into c->q_pinned
  uint32_t streams = 1;  // wavefronts / streams of the render (mtx_stats.streams)
  size_t next = 0;
  hipEvent_t get() {
    if (next >= c->events.size()) {
      hipEvent_t e;
      hipEventCreate(&e);
      c->events.push_back(e);
    }
    return c->events[next++];
  }
  hipEvent_t begin(int k, hipStream_t st = nullptr) {
    if (!on) return nullptr;
    hipEvent_t e0 = get();
    hipEventRecord(e0, st ? st : c->stream);
    return e0;
  }
  void end(int k, hipEvent_t e0, hipStream_t st = nullptr) {
    if (!on) return;
    hipEvent_t e1 = get();
    hipEventRecord(e1, st ? st : c->stream);
    pairs[k].push_back({e0, e1});
  }
  double total(int k) {
    double ms = 0;
    for (auto &p : pairs[k]) {
      float t = 0;
      hipEventElapsedTime(&t, p.first, p.second);
      ms += t;
    }
    return ms;
  }
};

// Encode + MLP + L += T * out for the compacted cache queries of a chunk of
// wave `w` (views `b`), on the wave's stream with the wave's buffers.
int run_cache(mtx_ctx *c, Wave &w, const mtxd::WaveBuffers &b, uint32_t cap, Timer &tm, bool nerad_render) {
  hipStream_t st = w.stream;
  DevBuf &f_feat = w.f_feat, &f_out = w.f_out;
  const uint32_t *perm = nullptr;
  int xcd_split = 0;
  hipEvent_t e = tm.begin(4, st);
  if (c->cache_sort == 2 && !nerad_render) {
    // region-grouped rows, the blocks of each XCD on one eighth of them
    // (field.hip k_field_encode xcd_split): device-only, no host round trip
    if (!dalloc(w.cq_perm, 4ull * cap) && !dalloc(w.cq_cursor, 4ull * 32768)) {
      mtxd::field_bucket_queries(c->field, b.cq_p, b.cq_count, cap, (uint32_t *)w.cq_cursor.p,
                                 (uint32_t *)w.cq_perm.p, c->n_cu, st);
      perm = (const uint32_t *)w.cq_perm.p;
      xcd_split = 1;
    }
  } else if (c->cache_sort && !nerad_render && &w == &c->wave[0]) {
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
      mtxd::field_morton_keys(c->field, b.cq_p, nq, (uint32_t *)keys.p, st);
      if (mtxd::sort24((const uint32_t *)keys.p, nq, (uint32_t *)w.cq_perm.p, c->cq_ws.p, st) == MTX_OK)
        perm = (const uint32_t *)w.cq_perm.p;
    }
  }
  // the fused pass only when its LDS fits a workgroup (n_hidden <= 14)
  const bool fused = c->cache_fused && !nerad_render && mtxd::field_cache_fused_lds(c->field_hidden) <= c->max_lds;
  int rc = MTX_OK;
  if (fused) {
    // encode + MLP + L += T * out in one launch (field.hip k_field_cache_fused),
    // timed as the encode
    rc = mtxd::field_cache_fused(c->field, b.cq_p, b.cq_d, b.cq_t, b.cq_count, cap, perm, xcd_split,
                                 c->field_frag.p, c->field_hidden, b.L[mtxd::kFinal], c->n_cu, st);
    tm.end(4, e, st);
    if (rc) return rc;
  } else {
    rc = mtxd::field_encode(c->field, b.cq_p, b.cq_d, b.cq_count, cap, (uint16_t *)f_feat.p, st, perm, xcd_split,
                            (int)c->encode_lm);
    tm.end(4, e, st);
    if (rc) return rc;
    e = tm.begin(5, st);
    rc = mtxd::field_mlp((const uint16_t *)f_feat.p, b.cq_count, cap, c->field_frag.p, c->field_hidden,
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
  mtxd::launch_shade(s, b, p, bounce, std::max(1, c->shade_grid / div), st);
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
  if (c->rs_n != n) {
    c->rs_valid = false;
    const size_t N = n;
    for (int k = 0; k < 2; ++k)
      if ((rc = dalloc(c->rs_samp[k], 5 * 16 * N))) return rc;
    if ((rc = dalloc(c->rs_tres, 6 * 16 * N))) return rc;
    if ((rc = dalloc(c->rs_sres, 6 * 16 * N))) return rc;
    if ((rc = dalloc(c->rs_radius, 4 * N))) return rc;
    if ((rc = dalloc(c->rs_hit, 16 * N))) return rc;
    if ((rc = dalloc(c->rs_dir, 16 * N))) return rc;
    if ((rc = dalloc(c->rs_emit, 16 * N))) return rc;
    if ((rc = dalloc(c->rs_rng, 16 * N))) return rc;
    if ((rc = dalloc(c->rs_rays, 9 * 32 * N))) return rc;
    if ((rc = dalloc(c->rs_count, 16))) return rc;
    if ((rc = dalloc(c->rs_heads, 4ull * mtxd::kXSlotWords))) return rc;
    if ((rc = dalloc(c->rs_occ, 18 * N))) return rc;
    if ((rc = dalloc(c->rs_qM, 10 * 4 * N))) return rc;
    if ((rc = dalloc(c->rs_nbr, 10 * 4 * N))) return rc;
    if ((rc = dalloc(c->rs_xs, 16 * N))) return rc;
    if ((rc = dalloc(c->rs_ns, 16 * N))) return rc;
    c->rs_n = n;
  }
  return MTX_OK;
}

// One RestirIntegrator.render() frame (restirgi.py:182-258) over the whole
// film; the kernel sequence is documented in restir.hip.
int render_restir(mtx_ctx *c, const mtx_render_args *a, float4 *film_dev, Timer &tm, uint64_t *n_trace,
                  uint64_t *n_shadow, bool want_stats) {
  const mtx_camera &cam = c->scene.camera;
  const uint32_t W = cam.width, H = cam.height, spp = a->spp;
  if (a->sample_offset != 0 || a->spp_total != spp) {
    mtx_set_error("mtx_render: ReSTIR GI needs spp_total = spp and sample_offset = 0");
    return MTX_E_ARG;
  }
  if (c->scene.has_env) {
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
  if (run_a && a->frame != 0 && !c->rs_valid) {
    mtx_set_error("mtx_render: ReSTIR GI frame %u without the state of frame 0 (film size or scene changed?)",
                  a->frame);
    return MTX_E_ARG;
  }
  if (only_b && (!c->rs_pending_b || c->rs_pending_frame != a->frame)) {
    mtx_set_error("mtx_render: ReSTIR stage B of frame %u without its stage A", a->frame);
    return MTX_E_ARG;
  }
  hipStream_t st = c->stream;
  if (run_a && a->frame == 0) {  // restirgi.py:217-229
    HIP_TRY(hipMemsetAsync(c->rs_tres.p, 0, 6 * 16 * (size_t)n, st));
    HIP_TRY(hipMemsetAsync(c->rs_sres.p, 0, 6 * 16 * (size_t)n, st));
    HIP_TRY(hipMemsetAsync(c->rs_samp[0].p, 0, 5 * 16 * (size_t)n, st));
    HIP_TRY(hipMemsetAsync(c->rs_samp[1].p, 0, 5 * 16 * (size_t)n, st));
    uint32_t bits;
    memcpy(&bits, &a->initial_search_radius, 4);
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c->rs_radius.p, (int)bits, n, st));
    c->rs_prev_cam = cam;
    c->rs_cur = 0;
  }
  mtxd::WaveBuffers b = views(c, wv[0]);
  mtxd::RestirBuffers r{};
  r.cur = (float4 *)c->rs_samp[c->rs_cur].p;
  r.prev = a->frame == 0 ? r.cur : (const float4 *)c->rs_samp[c->rs_cur ^ 1].p;
  r.tres = (float4 *)c->rs_tres.p;
  r.sres = (float4 *)c->rs_sres.p;
  r.radius = (float *)c->rs_radius.p;
  r.prim_hit = (float4 *)c->rs_hit.p;
  r.prim_dir = (float4 *)c->rs_dir.p;
  r.emit = (float4 *)c->rs_emit.p;
  r.rng = (uint4 *)c->rs_rng.p;
  r.test_rays = (float4 *)c->rs_rays.p;
  r.test_count = (uint32_t *)c->rs_count.p;
  r.test_heads = (uint32_t *)c->rs_heads.p;
  r.occ = (uint8_t *)c->rs_occ.p;
  r.qM = (uint32_t *)c->rs_qM.p;
  r.nbr = (uint32_t *)c->rs_nbr.p;
  r.n = n;
  r.lane0 = lane0;
  r.nb = nb;
  r.prev_cam = c->rs_prev_cam;
  r.flags = a->restir_flags;
  r.xcd_remap = c->xcd_claim;
  r.max_M_temporal = a->max_M_temporal;
  r.max_M_spatial = a->max_M_spatial;
  r.initial_radius = a->initial_search_radius;
  r.minimal_radius = a->minimal_search_radius;
  r.frame = a->frame;
  b.rs_xs = (float4 *)c->rs_xs.p;
  b.rs_ns = (float4 *)c->rs_ns.p;

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
        c->mega_paths == 0xffffffffu ? 2u * (uint32_t)c->mega_grid * mtxd::kShadeBlock : c->mega_paths;
    const bool mega_all = !p.stats && nb <= mega_max;
    const bool two = !mega_all && c->streams > 1 && rows >= 2 && nb >= (1u << 16);
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
    if (mega_all && c->rs_fused) {
      // the whole stage A up to k_rs_collect in one per-lane launch
      // (kernels.hip k_rs_stage_a), then the temporal pass
      HIP_TRY(reset_counters(b, depth, st));
      e = tm.begin(0, st);
      mtxd::launch_rs_stage_a(sc[0], b, p, r,
                              std::max(1, std::min<int>(c->mega_grid, (nb + mtxd::kShadeBlock - 1) / mtxd::kShadeBlock)),
                              st);
      tm.end(0, e, st);
      ++*n_trace;
      mtxd::launch_restir_temporal(r, p, st);
    }
    const bool fused = mega_all && c->rs_fused;
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
    mtxd::launch_trace_test(c->scene, r, 0, c->trace_grid, st);
    tm.end(1, e);
    ++*n_shadow;
    HIP_TRY(hipMemsetAsync(r.test_count, 0, 16, st));
    HIP_TRY(hipMemsetAsync(r.test_heads, 0, 4ull * mtxd::kXSlotWords, st));
    mtxd::launch_restir_spatial_merge(r, p, st);
    if (a->restir_flags & MTX_RESTIR_BIAS_CORRECTION) {
      e = tm.begin(1);
      mtxd::launch_trace_test(c->scene, r, 9 * n, c->trace_grid, st);
      tm.end(1, e);
      ++*n_shadow;
      mtxd::launch_restir_bias_finish(r, p, st);
    }
    mtxd::launch_restir_final(c->scene, b, p, r, st);
    mtxd::launch_film_src(b, p, (float4 *)c->contrib.p, st);
    mtxd::launch_film_gather((const float4 *)c->contrib.p, film_dev, W, a->y0, a->y1, 1, 1u, a->rfilter, st);
  }
  HIP_TRY(hipGetLastError());
  if (only_a) {
    c->rs_pending_b = true;
    c->rs_pending_frame = a->frame;
    c->rs_valid = a->frame != 0 ? c->rs_valid : false;
    return MTX_OK;
  }
  // restirgi.py:245-247: prev_sensor <- sensor, prev_sample <- sample
  c->rs_pending_b = false;
  c->rs_prev_cam = cam;
  c->rs_cur ^= 1;
  c->rs_valid = true;
  return MTX_OK;
}

}  // namespace

extern "C" {

int mtx_render(mtx_ctx *c, const mtx_render_args *a, float *film_rgbw, int film_on_device, mtx_stats *stats) {
  int rc = check_args(c, a);
  if (rc) return rc;
  const mtx_camera &cam = c->scene.camera;
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
  const bool two = c->streams > 1 && !mlt && !(nrc_cache && c->cache_sort == 1) && !nerad_render &&
                   a->integrator != MTX_INT_RESTIR_GI && n_paths_all >= (1u << 16) &&
                   n_paths_all <= (1ull << c->streams_max_log2);
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

int mtx_rfilter_info(uint32_t rfilter, uint32_t *border_out, float *radius_out) {
  if (rfilter >= mtx::kRfilterCount) {
    mtx_set_error("mtx_rfilter_info: unknown reconstruction filter %u", rfilter);
    return MTX_E_ARG;
  }
  if (border_out) *border_out = mtx::rfilter_reach(rfilter);
  if (radius_out) *radius_out = mtx::rfilter_radius(rfilter);
  return MTX_OK;
}

int mtx_rfilter_eval(uint32_t rfilter, const float *r, float *w_out, uint64_t n) {
  if (rfilter >= mtx::kRfilterCount) {
    mtx_set_error("mtx_rfilter_eval: unknown reconstruction filter %u", rfilter);
    return MTX_E_ARG;
  }
  if (n && (!r || !w_out)) {
    mtx_set_error("mtx_rfilter_eval: null argument");
    return MTX_E_ARG;
  }
  for (uint64_t i = 0; i < n; ++i) w_out[i] = mtx::rfilter_eval(rfilter, r[i]);
  return MTX_OK;
}

int mtx_set_camera(mtx_ctx *c, const mtx_camera *cam) {
  if (!c || !cam) {
    mtx_set_error("mtx_set_camera: null argument");
    return MTX_E_ARG;
  }
  if (!c->has_scene) {
    mtx_set_error("no scene uploaded");
    return MTX_E_NOSCENE;
  }
  if (cam->width != c->scene.camera.width || cam->height != c->scene.camera.height) {
    mtx_set_error("mtx_set_camera: film size changed (%ux%u -> %ux%u)", c->scene.camera.width,
                  c->scene.camera.height, cam->width, cam->height);
    return MTX_E_ARG;
  }
  c->scene.camera = *cam;
  return MTX_OK;
}

int mtx_restir_rows(mtx_ctx *c, int which, uint32_t row0, uint32_t nrows, void *buf, int to_state) {
  if (!c || !buf || which < 0 || which > 2) {
    mtx_set_error("mtx_restir_rows: bad argument");
    return MTX_E_ARG;
  }
  if (!c->rs_n || !c->has_scene) {
    mtx_set_error("mtx_restir_rows: no ReSTIR GI state");
    return MTX_E_ARG;
  }
  const uint32_t W = c->scene.camera.width, H = c->scene.camera.height;
  if (row0 + nrows > H || nrows == 0) {
    mtx_set_error("mtx_restir_rows: rows [%u, %u) outside the film", row0, row0 + nrows);
    return MTX_E_ARG;
  }
  const size_t n = c->rs_n, per_row = n / H;  // lanes per row (W * spp)
  (void)W;
  if (which == 2 && (!c->rs_valid || c->rs_pending_b)) {
    mtx_set_error("mtx_restir_rows: the previous frame's samples exist between complete frames only");
    return MTX_E_ARG;
  }
  const int planes = which == 1 ? 6 : 5;
  // which = 0: the current frame's samples (before stage B swaps them);
  // 2: the previous frame's (what k_rs_temporal reads through prev_cam)
  char *state = (char *)(which == 0 ? c->rs_samp[c->rs_cur].p
                                    : which == 2 ? c->rs_samp[c->rs_cur ^ 1].p : c->rs_tres.p);
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
  if (!c->rs_valid) {
    mtx_set_error("mtx_restir_state: no ReSTIR GI frame rendered");
    return MTX_E_ARG;
  }
  const uint64_t n = c->rs_n;
  const void *src = nullptr;
  uint64_t need = 0;
  switch (which) {
    case 0: src = c->rs_samp[c->rs_cur ^ 1].p; need = 20 * n; break;  // the frame just rendered
    case 1: src = c->rs_tres.p; need = 24 * n; break;
    case 2: src = c->rs_sres.p; need = 24 * n; break;
    case 3: src = c->rs_radius.p; need = n; break;
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

// Device-pointer entry points (the *_dev functions of mtx.h): every buffer
// must be memory of the context's device (hipMalloc'd, e.g. a torch CUDA
// tensor's data_ptr); host memory is refused with MTX_E_ARG.
static bool on_device(const mtx_ctx *c, const void *p) {
  if (!p) return false;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // clear the sticky "invalid value" of an unregistered host pointer
    return false;
  }
  return (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) && at.device == c->device;
}
static int need_device(const mtx_ctx *c, const char *fn, std::initializer_list<const void *> ptrs) {
  int k = 0;
  for (const void *p : ptrs) {
    if (p && !on_device(c, p)) {
      mtx_set_error("%s: argument %d is not device memory of device %d", fn, k, c->device);
      return MTX_E_ARG;
    }
    ++k;
  }
  return MTX_OK;
}

// New vertex positions for the uploaded scene (refit.hip). The pre-pass reads
// only -- the mesh emitters' new tables go to scratch -- and a refusal leaves
// the scene as it was. After it every pass is stream-ordered: triangles, the
// mesh emitters' tables and records from the scratch, the closest-hit tree's
// levels from the deepest to the root, the occlusion records, the occlusion
// tree's levels.
int mtx_scene_update_vertices(mtx_ctx *c, const float *vpos, const float *vnormal, uint32_t n_verts, int dev) {
  if (!c || !vpos) {
    mtx_set_error("mtx_scene_update_vertices: null argument");
    return MTX_E_ARG;
  }
  if (!c->has_scene) {
    mtx_set_error("no scene uploaded");
    return MTX_E_NOSCENE;
  }
  if (n_verts != c->scene_n_verts) {
    mtx_set_error("mtx_scene_update_vertices: %u vertices given, the scene has %u (topology changes need a new upload)",
                  n_verts, c->scene_n_verts);
    return MTX_E_ARG;
  }
  if (vnormal && !c->vnormal.p) {
    mtx_set_error("mtx_scene_update_vertices: the scene was uploaded without vertex normals");
    return MTX_E_ARG;
  }
  int rc;
  if (dev && (rc = need_device(c, "mtx_scene_update_vertices", {vpos, vnormal}))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const mtxd::DevScene &s = c->scene;
  const uint32_t n_tris = s.n_tris;
  const size_t vbytes = 12ull * n_verts;
  if ((rc = dalloc(c->rf_state, mtxd::RF_WORDS * sizeof(uint32_t)))) return rc;
  if ((rc = dalloc(c->rf_tbox, 24ull * n_tris))) return rc;
  if ((rc = dalloc(c->rf_nbox, 24ull * std::max(c->scene_n_nodes, c->scene_n_occ)))) return rc;
  const float *vp = vpos, *vn = vnormal;
  if (!dev) {  // stage the host arrays: the scene's own copies stay until the checks pass
    if ((rc = dalloc(c->rf_vpos, vbytes))) return rc;
    HIP_TRY(hipMemcpyAsync(c->rf_vpos.p, vpos, vbytes, hipMemcpyHostToDevice, st));
    vp = (const float *)c->rf_vpos.p;
    if (vnormal) {
      if ((rc = dalloc(c->rf_vnormal, vbytes))) return rc;
      HIP_TRY(hipMemcpyAsync(c->rf_vnormal.p, vnormal, vbytes, hipMemcpyHostToDevice, st));
      vn = (const float *)c->rf_vnormal.p;
    }
  }
  uint32_t *state = (uint32_t *)c->rf_state.p;
  mtxd::refit_state_init(state, st);
  mtxd::refit_prepass(vp, n_verts, s.tri_vidx, s.tri_shape, s.shapes, s.emitters, (const float *)c->shade_rec.p,
                      n_tris, state, st);
  mtxd::refit_emitter_tables(c->em_tables, vp, s.tri_vidx, s.tables, state, st);
  uint32_t h[mtxd::RF_WORDS];
  HIP_TRY(hipMemcpyAsync(h, state, sizeof(h), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  if (h[mtxd::RF_FLAGS] & mtxd::RF_BAD_COORD) {
    mtx_set_error("mtx_scene_update_vertices: a coordinate is non-finite or beyond the magnitude bound 2^37; the "
                  "scene is unchanged");
    return MTX_E_ARG;
  }
  if (h[mtxd::RF_FLAGS] & mtxd::RF_BAD_EMITTER) {
    mtx_set_error("mtx_scene_update_vertices: a vertex of a rectangle emitter shape would move (a rectangle "
                  "emitter is an analytic record derived from to_world, not from its vertices, and cannot be "
                  "animated; mesh emitters can); the scene is unchanged");
    return MTX_E_ARG;
  }
  if (h[mtxd::RF_FLAGS] & mtxd::RF_BAD_AREA) {
    mtx_set_error("mtx_scene_update_vertices: mesh emitter %u: its triangles have no finite positive area at the new "
                  "positions; the scene is unchanged", h[mtxd::RF_EM]);
    return MTX_E_ARG;
  }
  // from here on the scene is written
  if (vp != (const float *)c->vpos.p)
    HIP_TRY(hipMemcpyAsync(c->vpos.p, vp, vbytes, hipMemcpyDeviceToDevice, st));
  if (vn && vn != (const float *)c->vnormal.p)
    HIP_TRY(hipMemcpyAsync(c->vnormal.p, vn, vbytes, hipMemcpyDeviceToDevice, st));
  float *tbox = (float *)c->rf_tbox.p, *nbox = (float *)c->rf_nbox.p;
  mtxd::refit_triangles(vp, vn, s.tri_vidx, n_tris, (float *)c->tri.p, (float *)c->shade_rec.p, tbox, st);
  mtxd::refit_emitter_commit(c->em_tables, (float *)c->tables.p, (mtx_emitter *)c->emitters.p, st);
  const float extent = mtx::u2f(h[mtxd::RF_EXTENT]), occ_extent = mtx::u2f(h[mtxd::RF_OCC_EXTENT]);
  for (size_t l = c->lvl4_first.size() - 1; l-- > 0;)
    mtxd::refit_level4((int32_t *)c->nodes.p, c->lvl4_first[l], c->lvl4_first[l + 1] - c->lvl4_first[l],
                       (const uint32_t *)c->lvl4_list.p, tbox, nbox, extent, state, st);
  mtxd::refit_occ_gather((const float *)c->tri.p, (const uint32_t *)c->occ_perm.p, n_tris, (float *)c->occ_tri.p, tbox,
                         st);
  for (size_t l = c->lvl8_first.size() - 1; l-- > 0;)
    mtxd::refit_level8((uint32_t *)c->occ_nodes.p, c->lvl8_first[l], c->lvl8_first[l + 1] - c->lvl8_first[l],
                       (const uint32_t *)c->lvl8_list.p, tbox, nbox, occ_extent, state, st);
  uint32_t flags = 0;
  hipError_t e = hipMemcpyAsync(&flags, state + mtxd::RF_FLAGS, sizeof(flags), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess || (flags & mtxd::RF_BAD_QUANT)) {
    c->has_scene = false;  // never leave a half-refit tree live
    if (e != hipSuccess) {
      mtx_set_error("mtx_scene_update_vertices: %s; the scene was dropped, upload it again", hipGetErrorString(e));
      return MTX_E_HIP;
    }
    mtx_set_error("mtx_scene_update_vertices: child box quantisation failed; the scene was dropped, upload it again");
    return MTX_E_ARG;
  }
  mtx::V3 lo, hi;
  lo.x = mtxd::refit_key_decode(h[mtxd::RF_LO]);
  lo.y = mtxd::refit_key_decode(h[mtxd::RF_LO + 1]);
  lo.z = mtxd::refit_key_decode(h[mtxd::RF_LO + 2]);
  hi.x = mtxd::refit_key_decode(h[mtxd::RF_HI]);
  hi.y = mtxd::refit_key_decode(h[mtxd::RF_HI + 1]);
  hi.z = mtxd::refit_key_decode(h[mtxd::RF_HI + 2]);
  mtx::env_bsphere_box(lo, hi, c->scene.env_center, &c->scene.env_radius);
  c->has_nerad = false;  // surface tables belong to the previous geometry
  // The ReSTIR GI reservoirs are kept: the reference has no reprojection under
  // moving geometry either; a caller restarts with frame = 0 or accepts stale reuse.
  return MTX_OK;
}

// Test / debugging hook: the device copy of one scene array.
int mtx_scene_read(mtx_ctx *c, int which, void *out, uint64_t n_bytes) {
  if (!c || !out) {
    mtx_set_error("mtx_scene_read: null argument");
    return MTX_E_ARG;
  }
  if (!c->has_scene) {
    mtx_set_error("no scene uploaded");
    return MTX_E_NOSCENE;
  }
  const uint64_t nt = c->scene.n_tris, nv = c->scene_n_verts;
  const void *src = nullptr;
  uint64_t need = 0;
  switch (which) {
    case 0: src = c->nodes.p; need = 4ull * MTX_BVH_NODE_WORDS * c->scene_n_nodes; break;
    case 1: src = c->occ_nodes.p; need = 4ull * MTX_OCC_NODE_WORDS * c->scene_n_occ; break;
    case 2: src = c->tri.p; need = 36 * nt; break;
    case 3: src = c->occ_tri.p; need = 36 * nt; break;
    case 4: src = c->shade_rec.p; need = 128 * nt; break;
    case 5: src = c->vpos.p; need = 12 * nv; break;
    case 6: src = c->vnormal.p; need = c->vnormal.p ? 12 * nv : 0; break;
    case 7: need = 16; break;
    case 8: src = c->tables.p; need = 4ull * c->scene_n_tables; break;
    case 9: src = c->emitters.p; need = sizeof(mtx_emitter) * (uint64_t)c->scene.n_emitters; break;
    default:
      mtx_set_error("mtx_scene_read: which=%d not in 0..9", which);
      return MTX_E_ARG;
  }
  if (n_bytes != need) {
    mtx_set_error("mtx_scene_read: which=%d holds %llu bytes, got room for %llu", which, (unsigned long long)need,
                  (unsigned long long)n_bytes);
    return MTX_E_ARG;
  }
  if (which == 7) {
    float sph[4] = {c->scene.env_center[0], c->scene.env_center[1], c->scene.env_center[2], c->scene.env_radius};
    memcpy(out, sph, sizeof(sph));
    return MTX_OK;
  }
  if (need == 0) return MTX_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
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
    if ((rc = dalloc(c->s0, 24ull * cap))) return rc;
    if ((rc = dalloc(c->s1, 4ull * cap))) return rc;
    if ((rc = dalloc(c->s2, 12ull * cap))) return rc;
    if ((rc = dalloc(c->s3, 1ull * cap))) return rc;
  }
  mtxd::WaveBuffers b = views(c, w);
  Timer tm{c, false};
  uint64_t nt = 0, ns = 0;
  for (uint64_t off = 0; off < n; off += cap) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(cap, n - off);
    // the chunk's rays / lanes / outputs: the caller's device buffers, or the
    // context's staging copies of the host ones
    const float *d_rays = dev ? rays + 6 * off : (const float *)c->s0.p;
    const uint32_t *d_lanes = dev ? lanes + off : (const uint32_t *)c->s1.p;
    float *d_L = dev ? L + 3 * off : (float *)c->s2.p;
    uint8_t *d_valid = dev ? valid + off : (uint8_t *)c->s3.p;
    if (!dev) {
      HIP_TRY(hipMemcpyAsync(c->s0.p, rays + 6 * off, 24ull * m, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(c->s1.p, lanes + off, 4ull * m, hipMemcpyHostToDevice, c->stream));
    }
    mtxd::ChunkParams p{};
    p.integrator = a->integrator;
    p.max_depth = a->max_depth;
    p.rr_depth = a->rr_depth;
    p.seed = a->seed;
    p.spp = 1;
    p.spp_total = 1;
    p.width = c->scene.camera.width;
    p.height = c->scene.camera.height;
    p.n_paths = m;
    p.nrc_c = a->nrc_c;
    p.nrc_cache = nrc_cache ? 1u : 0u;
    HIP_TRY(reset_counters(b, std::max<uint32_t>(a->max_depth, 1), c->stream));
    if (nrc_cache || nerad_render) HIP_TRY(hipMemsetAsync(b.cq_count, 0, 4, c->stream));
    mtxd::launch_raygen_rays(c->scene, b, p, d_rays, d_lanes, rng_skip, c->stream);
    run_bounces(c, w, b, p, tm, &nt, &ns);
    if ((nrc_cache || nerad_render) && (rc = run_cache(c, w, b, m, tm, nerad_render))) return rc;
    mtxd::launch_collect(b, p, d_L, d_valid, c->stream);
    HIP_TRY(hipGetLastError());
    if (!dev) {
      HIP_TRY(hipMemcpyAsync(L + 3 * off, c->s2.p, 12ull * m, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(valid + off, c->s3.p, m, hipMemcpyDeviceToHost, c->stream));
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
  if (!c->has_scene) {
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
    mtxd::launch_trace_raw(c->scene, (const float4 *)rays, (uint32_t)n, any_hit, hits, visits, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MTX_OK;
  }
  if ((rc = dalloc(c->s0, 32ull * n))) return rc;
  if ((rc = dalloc(c->s1, 4ull * hit_words))) return rc;
  if (visits && (rc = dalloc(c->s2, 8ull * n))) return rc;
  HIP_TRY(hipMemcpyAsync(c->s0.p, rays, 32ull * n, hipMemcpyHostToDevice, c->stream));
  mtxd::launch_trace_raw(c->scene, (const float4 *)c->s0.p, (uint32_t)n, any_hit, (uint32_t *)c->s1.p,
                         visits ? (uint32_t *)c->s2.p : nullptr, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(hits, c->s1.p, 4ull * hit_words, hipMemcpyDeviceToHost, c->stream));
  if (visits) HIP_TRY(hipMemcpyAsync(visits, c->s2.p, 8ull * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

}  // extern "C"

// ------------------------------- primitives -------------------------------

// Runs the device work of one primitive call: `launch` enqueues the
// primitive's kernels on the context's stream and returns an MTX code. The
// event pair encloses those kernels only -- callers stage, range-check and
// copy back outside it -- and their time is what mtx_last_device_ms reports.
// The stream is idle on return.
template <class Launch>
static int prim_run(mtx_ctx *c, Launch launch) {
  for (int k = 0; k < 2; ++k)
    if (!c->prim_ev[k]) HIP_TRY(hipEventCreate(&c->prim_ev[k]));
  HIP_TRY(hipEventRecord(c->prim_ev[0], c->stream));
  if (int rc = launch()) return rc;
  HIP_TRY(hipEventRecord(c->prim_ev[1], c->stream));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c->prim_ev[0], c->prim_ev[1]) == hipSuccess) c->last_device_ms = ms;
  return MTX_OK;
}

extern "C" {

double mtx_last_device_ms(mtx_ctx *c) { return c ? c->last_device_ms : 0.0; }

int mtx_field_upload(mtx_ctx *c, const mtx_field_desc *f) {
  if (!c || !f || !f->table || !f->weights) {
    mtx_set_error("mtx_field_upload: null argument");
    return MTX_E_ARG;
  }
  if (f->n_levels == 0 || f->n_levels > mtx::kFieldMaxLevels || f->n_features < 1 || f->n_features > 2 ||
      f->log2_table < 4 || f->log2_table > 26 || f->n_hidden > 16 ||
      f->n_in != 3 + f->n_levels * f->n_features + 3 + 16 || f->n_in > 64 || f->base_res < 1 ||
      !(f->per_level_scale >= 1.f)) {
    mtx_set_error("mtx_field_upload: unsupported field shape (n_in must be 3 + L*F + 19 <= 64)");
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  const size_t table_halfs = (size_t)f->n_levels * ((size_t)1 << f->log2_table) * f->n_features;
  if ((rc = upload(c->field_table, f->table, table_halfs, c->stream))) return rc;
  const uint32_t n_frag = mtxd::field_frag_count(f->n_hidden);
  std::vector<uint16_t> frag((size_t)n_frag * 64 * 8);
  mtxd::field_prepack(f->weights, f->n_in, f->n_hidden, frag.data());
  if ((rc = upload(c->field_frag, frag.data(), frag.size(), c->stream))) return rc;
  const uint32_t n_w = 64u * f->n_in + f->n_hidden * 4096u + 3u * 64u;
  if ((rc = upload(c->field_w16, f->weights, n_w, c->stream))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->field_n_in = f->n_in;
  c->field_n_w = n_w;
  c->field_n_table = table_halfs;
  c->training = false;  // a new field: mtx_field_train_init starts over
  mtx::FieldEncoding &e = c->field;
  e.table = (const uint16_t *)c->field_table.p;
  e.n_levels = f->n_levels;
  e.n_features = f->n_features;
  e.log2_table = f->log2_table;
  for (uint32_t l = 0; l < f->n_levels; ++l) {
    const double scale = std::exp2((double)l * std::log2((double)f->per_level_scale)) * f->base_res - 1.0;
    e.level_scale[l] = (float)scale;
    e.level_res[l] = (uint32_t)std::ceil((double)(float)scale) + 1u;
  }
  for (int k = 0; k < 3; ++k) {
    e.bbox_min[k] = f->bbox_min[k];
    e.bbox_max[k] = f->bbox_max[k];
  }
  c->field_hidden = f->n_hidden;
  c->has_field = true;
  return MTX_OK;
}

static int field_stage_queries(mtx_ctx *c, uint64_t n, const float *p, const float *wi) {
  int rc;
  if ((rc = dalloc(c->fq_p, 16 * n))) return rc;
  if ((rc = dalloc(c->fq_d, 16 * n))) return rc;
  std::vector<float> tp(4 * n), td(4 * n);
  for (uint64_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      tp[4 * i + k] = p[3 * i + k];
      td[4 * i + k] = wi[3 * i + k];
    }
  HIP_TRY(hipMemcpy(c->fq_p.p, tp.data(), 16 * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->fq_d.p, td.data(), 16 * n, hipMemcpyHostToDevice));
  return MTX_OK;
}

static int field_check(mtx_ctx *c, uint64_t n) {
  if (!c || !c->has_field) {
    mtx_set_error("no radiance field uploaded (mtx_field_upload)");
    return MTX_E_ARG;
  }
  if (n >= (1ull << 31)) {
    mtx_set_error("too many field queries");
    return MTX_E_ARG;
  }
  return MTX_OK;
}

// The encoder over the n staged queries and the MLP over n feature rows;
// wave 0's feature and output buffers are the field entry points' scratch.
static int field_encode_staged(mtx_ctx *c, uint64_t n) {
  return mtxd::field_encode(c->field, (const float4 *)c->fq_p.p, (const float4 *)c->fq_d.p, nullptr, (uint32_t)n,
                            (uint16_t *)c->wave[0].f_feat.p, c->stream);
}
static int field_mlp_staged(mtx_ctx *c, uint64_t n) {
  return mtxd::field_mlp((const uint16_t *)c->wave[0].f_feat.p, nullptr, (uint32_t)n, c->field_frag.p,
                         c->field_hidden, (float *)c->wave[0].f_out.p, c->n_cu, c->stream);
}

// A scratch slot of `bytes` for a host entry point, filled from `src` if given.
static int stage(mtx_ctx *c, DevBuf &slot, size_t bytes, const void *src = nullptr) {
  if (int rc = dalloc(slot, bytes)) return rc;
  if (src) HIP_TRY(hipMemcpyAsync(slot.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  return MTX_OK;
}
// Copies results back to the host arrays; returns once they have landed.
struct Unstage {
  void *dst;
  const DevBuf &slot;
  size_t bytes;
};
static int unstage(mtx_ctx *c, std::initializer_list<Unstage> outs) {
  for (const Unstage &o : outs) HIP_TRY(hipMemcpyAsync(o.dst, o.slot.p, o.bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

int mtx_field_features(mtx_ctx *c, uint64_t n, const float *p, const float *wi, uint16_t *feat) {
  int rc = field_check(c, n);
  if (rc) return rc;
  if (n == 0) return MTX_OK;
  if (!p || !wi || !feat) {
    mtx_set_error("mtx_field_features: null buffer");
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = field_stage_queries(c, n, p, wi))) return rc;
  if ((rc = dalloc(c->wave[0].f_feat, kFeatBytes * n))) return rc;
  if ((rc = prim_run(c, [&] { return field_encode_staged(c, n); }))) return rc;
  return unstage(c, {{feat, c->wave[0].f_feat, kFeatBytes * n}});
}

int mtx_field_mlp(mtx_ctx *c, uint64_t n, const uint16_t *feat, float *out) {
  int rc = field_check(c, n);
  if (rc) return rc;
  if (n == 0) return MTX_OK;
  if (!feat || !out) {
    mtx_set_error("mtx_field_mlp: null buffer");
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = stage(c, c->wave[0].f_feat, kFeatBytes * n, feat))) return rc;
  if ((rc = dalloc(c->wave[0].f_out, kOutBytes * n))) return rc;
  if ((rc = prim_run(c, [&] { return field_mlp_staged(c, n); }))) return rc;
  return unstage(c, {{out, c->wave[0].f_out, kOutBytes * n}});
}

int mtx_field_eval(mtx_ctx *c, uint64_t n, const float *p, const float *wi, float *out) {
  int rc = field_check(c, n);
  if (rc) return rc;
  if (n == 0) return MTX_OK;
  if (!p || !wi || !out) {
    mtx_set_error("mtx_field_eval: null buffer");
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = field_stage_queries(c, n, p, wi))) return rc;
  if ((rc = dalloc(c->wave[0].f_feat, kFeatBytes * n))) return rc;
  if ((rc = dalloc(c->wave[0].f_out, kOutBytes * n))) return rc;
  if ((rc = prim_run(c, [&] {
         const int e = field_encode_staged(c, n);
         return e ? e : field_mlp_staged(c, n);
       })))
    return rc;
  return unstage(c, {{out, c->wave[0].f_out, kOutBytes * n}});
}

// The five primitives, one function each for the host entry (dev = false:
// host arrays, staged in the scratch slots and copied back) and the _dev
// entry (device arrays, used in place). `fn` is the entry the caller used.
// Order: argument and size checks; for device arrays need_device on every
// pointer before anything touches them, for host arrays the index range
// loop; workspace and staging; the device-side range check of device
// indices; the timed launch.

// Host indices: every v[i] < bound.
static int host_in_range(const char *fn, const char *what, const uint32_t *v, uint64_t n, uint64_t bound) {
  for (uint64_t i = 0; i < n; ++i)
    if (v[i] >= bound) {
      mtx_set_error("%s: %s[%llu] = %u out of range", fn, what, (unsigned long long)i, v[i]);
      return MTX_E_ARG;
    }
  return MTX_OK;
}
// Device indices: checked on the device before any kernel indexes with them.
static int dev_in_range(mtx_ctx *c, const uint32_t *v, uint64_t n, uint32_t bound, uint32_t *bad) {
  int rc;
  if ((rc = dalloc(c->s6, 64))) return rc;
  HIP_TRY(hipMemsetAsync(c->s6.p, 0, 4, c->stream));
  if ((rc = mtxd::keys_in_range(v, n, bound, (uint32_t *)c->s6.p, c->stream))) return rc;
  HIP_TRY(hipMemcpyAsync(bad, c->s6.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

static int prefix_sum_u32_impl(mtx_ctx *c, const char *fn, bool dev, const uint32_t *in, uint32_t *out, uint64_t n,
                               int inclusive) {
  if (!c || (n && (!in || !out))) {
    mtx_set_error("%s: null argument", fn);
    return MTX_E_ARG;
  }
  if (n == 0) return MTX_OK;
  if (n >= (1ull << 32)) {
    mtx_set_error("%s: n >= 2^32", fn);
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if (dev && (rc = need_device(c, fn, {in, out}))) return rc;
  if ((rc = dalloc(c->s2, mtxd::scan_workspace_bytes(n)))) return rc;
  if (!dev) {
    if ((rc = stage(c, c->s0, 4 * n, in)) || (rc = stage(c, c->s1, 4 * n))) return rc;
    in = (const uint32_t *)c->s0.p;
  }
  uint32_t *d_out = dev ? out : (uint32_t *)c->s1.p;
  if ((rc = prim_run(c, [&] { return mtxd::scan_u32(in, d_out, n, inclusive, c->s2.p, c->stream); }))) return rc;
  return dev ? MTX_OK : unstage(c, {{out, c->s1, 4 * n}});
}

static int prefix_sum_f32_hs_impl(mtx_ctx *c, const char *fn, bool dev, const float *in, float *out, uint64_t n) {
  if (!c || (n && (!in || !out))) {
    mtx_set_error("%s: null argument", fn);
    return MTX_E_ARG;
  }
  if (n == 0) return MTX_OK;
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if (dev && (rc = need_device(c, fn, {in, out}))) return rc;
  if ((rc = dalloc(c->s1, 4 * n))) return rc;  // ping-pong partner of the output
  if (!dev) {
    if ((rc = stage(c, c->s0, 4 * n, in)) || (rc = stage(c, c->s2, 4 * n))) return rc;
    in = (const float *)c->s0.p;
  }
  float *d_out = dev ? out : (float *)c->s2.p;
  if ((rc = prim_run(c, [&] { return mtxd::scan_f32_hs_to(in, d_out, (float *)c->s1.p, n, c->stream); })))
    return rc;
  return dev ? MTX_OK : unstage(c, {{out, c->s2, 4 * n}});
}

static int hashgrid_build_impl(mtx_ctx *c, const char *fn, bool dev, const float *p, uint64_t n, uint32_t resolution,
                               uint32_t n_cells, uint32_t *cell, uint32_t *cell_size, uint32_t *cell_offset,
                               uint32_t *sample_idx) {
  if (!c || !p || !cell || !cell_size || !cell_offset || !sample_idx || n == 0 || n_cells == 0) {
    mtx_set_error("%s: bad argument", fn);
    return MTX_E_ARG;
  }
  if (n >= (1ull << 31)) {
    mtx_set_error("%s: n too large", fn);
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if (dev && (rc = need_device(c, fn, {p, cell, cell_size, cell_offset, sample_idx}))) return rc;
  if ((rc = dalloc(c->s5, mtxd::hashgrid_workspace_bytes(n, n_cells)))) return rc;
  uint32_t *d_cell = cell, *d_size = cell_size, *d_offset = cell_offset, *d_idx = sample_idx;
  if (!dev) {
    if ((rc = stage(c, c->s0, 12 * n, p)) || (rc = stage(c, c->s1, 4 * n)) ||
        (rc = stage(c, c->s2, 4ull * n_cells)) || (rc = stage(c, c->s3, 4ull * n_cells)) ||
        (rc = stage(c, c->s4, 4 * n)))
      return rc;
    p = (const float *)c->s0.p;
    d_cell = (uint32_t *)c->s1.p;
    d_size = (uint32_t *)c->s2.p;
    d_offset = (uint32_t *)c->s3.p;
    d_idx = (uint32_t *)c->s4.p;
  }
  if ((rc = prim_run(c, [&] {
         return mtxd::hashgrid_build(p, n, resolution, n_cells, d_cell, d_size, d_offset, d_idx, c->s5.p, c->stream);
       })))
    return rc;
  return dev ? MTX_OK
             : unstage(c, {{cell, c->s1, 4 * n},
                           {cell_size, c->s2, 4ull * n_cells},
                           {cell_offset, c->s3, 4ull * n_cells},
                           {sample_idx, c->s4, 4 * n}});
}

static int group_by_u32_impl(mtx_ctx *c, const char *fn, bool dev, const uint32_t *keys, uint64_t n, uint32_t n_keys,
                             uint32_t *key_size, uint32_t *key_offset, uint32_t *order) {
  if (!c || !keys || !key_size || !key_offset || !order || n == 0 || n_keys == 0) {
    mtx_set_error("%s: bad argument", fn);
    return MTX_E_ARG;
  }
  if (n >= (1ull << 31)) {
    mtx_set_error("%s: n too large", fn);
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if (dev ? (rc = need_device(c, fn, {keys, key_size, key_offset, order}))
          : (rc = host_in_range(fn, "keys", keys, n, n_keys)))
    return rc;
  if ((rc = dalloc(c->s5, mtxd::hashgrid_workspace_bytes(n, n_keys)))) return rc;
  uint32_t *d_size = key_size, *d_offset = key_offset, *d_order = order;
  if (dev) {
    uint32_t bad = 0;
    if ((rc = dev_in_range(c, keys, n, n_keys, &bad))) return rc;
    if (bad) {
      mtx_set_error("%s: a key is >= n_keys (%u)", fn, n_keys);
      return MTX_E_ARG;
    }
  } else {
    if ((rc = stage(c, c->s1, 4 * n, keys)) || (rc = stage(c, c->s2, 4ull * n_keys)) ||
        (rc = stage(c, c->s3, 4ull * n_keys)) || (rc = stage(c, c->s4, 4 * n)))
      return rc;
    keys = (const uint32_t *)c->s1.p;
    d_size = (uint32_t *)c->s2.p;
    d_offset = (uint32_t *)c->s3.p;
    d_order = (uint32_t *)c->s4.p;
  }
  if ((rc = prim_run(c, [&] {
         return mtxd::group_by_u32(keys, n, n_keys, d_size, d_offset, d_order, c->s5.p, c->stream);
       })))
    return rc;
  return dev ? MTX_OK
             : unstage(c, {{key_size, c->s2, 4ull * n_keys}, {key_offset, c->s3, 4ull * n_keys}, {order, c->s4, 4 * n}});
}

static int scatter_reduce_f32_impl(mtx_ctx *c, const char *fn, bool dev, int op, float *target, uint64_t n_target,
                                   const float *value, const uint32_t *index, uint64_t n_value) {
  if (!c || !target || (n_value && (!value || !index)) || op < 0 || op > 3) {
    mtx_set_error("%s: bad argument", fn);
    return MTX_E_ARG;
  }
  if (n_value == 0 || n_target == 0) return MTX_OK;
  if (n_value >= (1ull << 31) || n_target >= (1ull << 31)) {
    mtx_set_error("%s: size too large", fn);
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if (dev ? (rc = need_device(c, fn, {target, value, index}))
          : (rc = host_in_range(fn, "index", index, n_value, n_target)))
    return rc;
  if ((rc = dalloc(c->s3, mtxd::scatter_workspace_bytes(n_target, n_value)))) return rc;
  float *d_target = target;
  if (dev) {
    uint32_t bad = 0;
    if ((rc = dev_in_range(c, index, n_value, (uint32_t)n_target, &bad))) return rc;
    if (bad) {
      mtx_set_error("%s: an index is >= n_target (%llu)", fn, (unsigned long long)n_target);
      return MTX_E_ARG;
    }
  } else {
    if ((rc = stage(c, c->s0, 4 * n_target, target)) || (rc = stage(c, c->s1, 4 * n_value, value)) ||
        (rc = stage(c, c->s2, 4 * n_value, index)))
      return rc;
    d_target = (float *)c->s0.p;
    value = (const float *)c->s1.p;
    index = (const uint32_t *)c->s2.p;
  }
  if ((rc = prim_run(c, [&] {
         return mtxd::scatter_reduce_f32(op, d_target, n_target, value, index, n_value, c->s3.p, c->stream);
       })))
    return rc;
  return dev ? MTX_OK : unstage(c, {{target, c->s0, 4 * n_target}});
}

int mtx_prefix_sum_u32(mtx_ctx *c, const uint32_t *in, uint32_t *out, uint64_t n, int inclusive) {
  return prefix_sum_u32_impl(c, "mtx_prefix_sum_u32", false, in, out, n, inclusive);
}
int mtx_prefix_sum_u32_dev(mtx_ctx *c, const uint32_t *in, uint32_t *out, uint64_t n, int inclusive) {
  return prefix_sum_u32_impl(c, "mtx_prefix_sum_u32_dev", true, in, out, n, inclusive);
}

int mtx_prefix_sum_f32_hs(mtx_ctx *c, const float *in, float *out, uint64_t n) {
  return prefix_sum_f32_hs_impl(c, "mtx_prefix_sum_f32_hs", false, in, out, n);
}
int mtx_prefix_sum_f32_hs_dev(mtx_ctx *c, const float *in, float *out, uint64_t n) {
  return prefix_sum_f32_hs_impl(c, "mtx_prefix_sum_f32_hs_dev", true, in, out, n);
}

int mtx_hashgrid_build(mtx_ctx *c, const float *p, uint64_t n, uint32_t resolution, uint32_t n_cells, uint32_t *cell,
                       uint32_t *cell_size, uint32_t *cell_offset, uint32_t *sample_idx) {
  return hashgrid_build_impl(c, "mtx_hashgrid_build", false, p, n, resolution, n_cells, cell, cell_size, cell_offset,
                             sample_idx);
}
int mtx_hashgrid_build_dev(mtx_ctx *c, const float *p, uint64_t n, uint32_t resolution, uint32_t n_cells,
                           uint32_t *cell, uint32_t *cell_size, uint32_t *cell_offset, uint32_t *sample_idx) {
  return hashgrid_build_impl(c, "mtx_hashgrid_build_dev", true, p, n, resolution, n_cells, cell, cell_size,
                             cell_offset, sample_idx);
}

int mtx_group_by_u32(mtx_ctx *c, const uint32_t *keys, uint64_t n, uint32_t n_keys, uint32_t *key_size,
                     uint32_t *key_offset, uint32_t *order) {
  return group_by_u32_impl(c, "mtx_group_by_u32", false, keys, n, n_keys, key_size, key_offset, order);
}
int mtx_group_by_u32_dev(mtx_ctx *c, const uint32_t *keys, uint64_t n, uint32_t n_keys, uint32_t *key_size,
                         uint32_t *key_offset, uint32_t *order) {
  return group_by_u32_impl(c, "mtx_group_by_u32_dev", true, keys, n, n_keys, key_size, key_offset, order);
}

int mtx_scatter_reduce_f32(mtx_ctx *c, int op, float *target, uint64_t n_target, const float *value,
                           const uint32_t *index, uint64_t n_value) {
  return scatter_reduce_f32_impl(c, "mtx_scatter_reduce_f32", false, op, target, n_target, value, index, n_value);
}
int mtx_scatter_reduce_f32_dev(mtx_ctx *c, int op, float *target, uint64_t n_target, const float *value,
                               const uint32_t *index, uint64_t n_value) {
  return scatter_reduce_f32_impl(c, "mtx_scatter_reduce_f32_dev", true, op, target, n_target, value, index, n_value);
}

}  // extern "C"

// ============================================================================
// Radiance-field training and neural radiosity samples (nerad.py:121-375)
// ============================================================================
static int train_check(mtx_ctx *c) {
  if (!c || !c->has_field) {
    mtx_set_error("no radiance field uploaded (mtx_field_upload)");
    return MTX_E_ARG;
  }
  if (!c->training) {
    mtx_set_error("field training not initialised (mtx_field_train_init)");
    return MTX_E_ARG;
  }
  return MTX_OK;
}

// k_field_train keeps every layer's activation tile in LDS: a field whose
// tiles exceed what one workgroup may hold (n_hidden >= 14 on gfx950's
// 160 KiB) cannot be trained. Refused here, on the host, before any launch.
static int train_fits(mtx_ctx *c) {
  const size_t lds = mtxd::field_train_lds(c->field_hidden);
  if (lds > c->max_lds) {
    mtx_set_error("field training: n_hidden %u needs %zu B of LDS per workgroup, the device allows %zu B "
                  "(inference of this field still works)",
                  c->field_hidden, lds, c->max_lds);
    return MTX_E_ARG;
  }
  return MTX_OK;
}

// Forward + backward of the field for n points (queries qp / qd on the
// device, targets 3n floats on the device): gradients of scale * loss in
// tr_g = [table | weights], network outputs in tr_out, loss (unscaled) on
// the host.
static int field_backward(mtx_ctx *c, const float4 *qp, const float4 *qd, const float *target, uint32_t n,
                          float scale, double *loss) {
  int rc;
  const uint32_t LF = c->field.n_levels * c->field.n_features;
  const uint32_t blocks = (n + 63) / 64;
  const uint64_t n_params = c->field_n_table + c->field_n_w;
  if ((rc = train_fits(c))) return rc;
  if ((rc = dalloc(c->tr_feat, 128ull * n))) return rc;
  if ((rc = dalloc(c->tr_out, 12ull * n))) return rc;
  if ((rc = dalloc(c->tr_loss, 4ull * blocks))) return rc;
  if ((rc = dalloc(c->tr_wpart, 4ull * blocks * c->field_n_w))) return rc;
  if ((rc = dalloc(c->tr_dfeat, 4ull * n * LF))) return rc;
  if ((rc = dalloc(c->tr_g, 4 * n_params))) return rc;
  if ((rc = mtxd::field_encode(c->field, qp, qd, nullptr, n, (uint16_t *)c->tr_feat.p, c->stream))) return rc;
  HIP_TRY(hipMemsetAsync(c->tr_g.p, 0, 4 * c->field_n_table, c->stream));
  float *g = (float *)c->tr_g.p;
  rc = mtxd::field_train_launch((const uint16_t *)c->tr_feat.p, n, (const uint16_t *)c->field_w16.p,
                                c->field_n_in, c->field_hidden, target, (float)(2.0 * scale / (3.0 * n)),
                                (float *)c->tr_out.p, (float *)c->tr_loss.p, (float *)c->tr_wpart.p,
                                g + c->field_n_table, (float *)c->tr_dfeat.p, LF, c->stream);
  if (rc) return rc;
  mtxd::field_encode_bwd_launch(c->field, qp, n, (const float *)c->tr_dfeat.p, g, c->stream);
  HIP_TRY(hipGetLastError());
  if (loss) {
    std::vector<float> part(blocks);
    HIP_TRY(hipMemcpyAsync(part.data(), c->tr_loss.p, 4ull * blocks, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    double sq = 0.0;
    for (float x : part) sq += x;
    *loss = sq / (3.0 * n);
  }
  return MTX_OK;
}

// GradScaler.step(opt): finite check of the scaled gradients, Adam on the
// unscaled ones (skipped on inf / NaN), scale update; the fp16 table and
// weights are rewritten by the Adam kernel and re-packed for the MFMA MLP.
static int field_opt_step(mtx_ctx *c, mtx_train_stats *st) {
  const uint64_t n_params = c->field_n_table + c->field_n_w;
  int rc;
  if ((rc = dalloc(c->tr_flag, 16))) return rc;
  HIP_TRY(hipMemsetAsync(c->tr_flag.p, 0, 4, c->stream));
  mtxd::grad_check_launch((const float *)c->tr_g.p, n_params, (uint32_t *)c->tr_flag.p, c->stream);
  uint32_t found = 0;
  HIP_TRY(hipMemcpyAsync(&found, c->tr_flag.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const mtx_field_opt &o = c->opt;
  if (!found) {
    ++c->adam_t;
    const double t = c->adam_t;
    const float lr_t = (float)(o.lr * std::sqrt(1.0 - std::pow((double)o.beta_2, t)) /
                               (1.0 - std::pow((double)o.beta_1, t)));
    mtxd::adam_launch((float *)c->tr_p.p, (float *)c->tr_m.p, (float *)c->tr_v.p, (const float *)c->tr_g.p, n_params,
                      lr_t, o.beta_1, o.beta_2, o.epsilon, 1.f / c->scale, (const uint32_t *)c->tr_flag.p,
                      (uint16_t *)c->field_table.p, c->field_n_table, (uint16_t *)c->field_w16.p, c->stream);
    mtxd::field_prepack_launch((const uint16_t *)c->field_w16.p, c->field_n_in, c->field_hidden,
                               (uint16_t *)c->field_frag.p, c->stream);
    HIP_TRY(hipGetLastError());
    if (++c->good_steps >= o.growth_interval) {
      c->scale *= o.growth_factor;
      c->good_steps = 0;
    }
  } else {
    c->scale *= o.backoff_factor;
    c->good_steps = 0;
  }
  if (st) {
    st->found_inf = found;
    st->scale = c->scale;
    st->step = c->adam_t;
  }
  return MTX_OK;
}

struct PhaseTimer {
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t st;
  explicit PhaseTimer(hipStream_t s) : st(s) {
    for (auto &e : ev) hipEventCreate(&e);
  }
  ~PhaseTimer() {
    for (auto &e : ev) hipEventDestroy(e);
  }
  void mark(int i) { hipEventRecord(ev[i], st); }
  double ms(int a, int b) {
    float t = 0.f;
    hipEventElapsedTime(&t, ev[a], ev[b]);
    return t;
  }
};

static int nerad_check(mtx_ctx *c, const mtx_nerad_args *a, bool need_field = true) {
  if (!c || !a) {
    mtx_set_error("null context or args");
    return MTX_E_ARG;
  }
  if (!c->has_scene || !c->has_nerad) {
    mtx_set_error("nerad: upload a scene and its surface tables (mtx_nerad_upload) first");
    return MTX_E_NOSCENE;
  }
  if (need_field && !c->has_field) {
    mtx_set_error("nerad: no radiance field uploaded (mtx_field_upload)");
    return MTX_E_ARG;
  }
  if (a->batch == 0 || a->M == 0 || (uint64_t)a->batch * a->M >= (1ull << 31)) {
    mtx_set_error("nerad: bad batch %u / M %u", a->batch, a->M);
    return MTX_E_ARG;
  }
  return MTX_OK;
}

static int nerad_lhs_dev(mtx_ctx *c, const mtx_nerad_args *a) {
  int rc;
  if ((rc = dalloc(c->nr_lhs, 48ull * a->batch))) return rc;
  if ((rc = dalloc(c->nr_qp, 16ull * a->batch))) return rc;
  if ((rc = dalloc(c->nr_qd, 16ull * a->batch))) return rc;
  mtxd::launch_nerad_lhs(c->scene, c->nr, a->lhs_seed, a->batch, (float4 *)c->nr_lhs.p, (float4 *)c->nr_qp.p,
                         (float4 *)c->nr_qd.p, c->stream);
  HIP_TRY(hipGetLastError());
  return MTX_OK;
}

// sample_rhs (nerad.py:174-233) for the points in nr_lhs: L_rhs in nr_Lrhs.
static int nerad_rhs_dev(mtx_ctx *c, const mtx_nerad_args *a, float *lanes_dev, uint32_t *queries,
                         mtx_train_stats *st = nullptr) {
  int rc;
  const uint32_t n = a->batch * a->M;
  const uint32_t bounces = 12;  // first vertex, its BSDF hit, <= 10 next_smooth_si traces (:146)
  Wave &w = c->wave[0];
  if ((rc = ensure_wave(c, w, n, bounces))) return rc;
  if ((rc = ensure_cache(c, w, n))) return rc;
  if ((rc = dalloc(c->nr_Lrhs, 12ull * a->batch))) return rc;
  mtxd::WaveBuffers b = views(c, w);
  mtxd::ChunkParams p{};
  p.integrator = MTX_INT_NERAD_RHS;
  p.max_depth = bounces;
  p.seed = a->rhs_seed;
  p.spp = p.spp_total = 1;
  p.n_paths = n;
  p.n_px = n;
  const bool counters = st && (a->flags & 1u);
  p.stats = counters ? 1u : 0u;
  HIP_TRY(reset_counters(b, bounces, c->stream));
  HIP_TRY(hipMemsetAsync(b.cq_count, 0, 4, c->stream));
  if (counters) HIP_TRY(hipMemsetAsync(b.stats, 0, 64, c->stream));
  mtxd::launch_nerad_raygen(b, p, (const float4 *)c->nr_lhs.p, a->M, c->stream);
  Timer tm{c, st != nullptr};
  uint64_t nt = 0, ns = 0;
  run_bounces(c, w, b, p, tm, &nt, &ns);
  if ((rc = mtxd::field_encode(c->field, b.cq_p, b.cq_d, b.cq_count, n, (uint16_t *)w.f_feat.p, c->stream))) return rc;
  if ((rc = mtxd::field_mlp((const uint16_t *)w.f_feat.p, b.cq_count, n, c->field_frag.p, c->field_hidden,
                            (float *)w.f_out.p, c->n_cu, c->stream)))
    return rc;
  mtxd::launch_nerad_apply(b, (const float *)w.f_out.p, n, 0, c->stream);
  mtxd::launch_nerad_mean(b, a->batch, a->M, (float *)c->nr_Lrhs.p, lanes_dev, c->stream);
  HIP_TRY(hipGetLastError());
  if (queries) HIP_TRY(hipMemcpyAsync(queries, b.cq_count, 4, hipMemcpyDeviceToHost, c->stream));
  if (st) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    st->ms_trace = tm.total(0);
    if (counters) {
      unsigned long long h[8];
      HIP_TRY(hipMemcpy(h, b.stats, 64, hipMemcpyDeviceToHost));
      st->nodes_closest = h[0];
      st->tris_closest = h[1];
      st->rays_closest = h[4];
    }
  }
  return MTX_OK;
}

extern "C" {

int mtx_field_train_init(mtx_ctx *c, const mtx_field_opt *opt) {
  if (!c || !opt || !c->has_field) {
    mtx_set_error("mtx_field_train_init: null argument or no field uploaded");
    return MTX_E_ARG;
  }
  if (!(opt->lr > 0.f) || !(opt->init_scale > 0.f) || opt->growth_interval == 0) {
    mtx_set_error("mtx_field_train_init: bad optimiser settings");
    return MTX_E_ARG;
  }
  int rc;
  if ((rc = train_fits(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t n_params = c->field_n_table + c->field_n_w;
  if ((rc = dalloc(c->tr_p, 4 * n_params))) return rc;
  if ((rc = dalloc(c->tr_m, 4 * n_params))) return rc;
  if ((rc = dalloc(c->tr_v, 4 * n_params))) return rc;
  mtxd::half_to_float_launch((const uint16_t *)c->field_table.p, c->field_n_table, (float *)c->tr_p.p, c->stream);
  mtxd::half_to_float_launch((const uint16_t *)c->field_w16.p, c->field_n_w, (float *)c->tr_p.p + c->field_n_table,
                             c->stream);
  HIP_TRY(hipMemsetAsync(c->tr_m.p, 0, 4 * n_params, c->stream));
  HIP_TRY(hipMemsetAsync(c->tr_v.p, 0, 4 * n_params, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->opt = *opt;
  c->adam_t = 0;
  c->good_steps = 0;
  c->scale = opt->init_scale;
  c->training = true;
  return MTX_OK;
}

int mtx_field_grad(mtx_ctx *c, uint64_t n, const float *p, const float *wi, const float *target, float scale,
                   float *out, double *loss, float *grad_table, float *grad_weights) {
  int rc = field_check(c, n);
  if (rc) return rc;
  if (n == 0 || !p || !wi || !target) {
    mtx_set_error("mtx_field_grad: empty batch or null input");
    return MTX_E_ARG;
  }
  if ((rc = train_fits(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = field_stage_queries(c, n, p, wi))) return rc;
  if ((rc = upload(c->tr_target, target, 3 * n, c->stream))) return rc;
  if ((rc = field_backward(c, (const float4 *)c->fq_p.p, (const float4 *)c->fq_d.p, (const float *)c->tr_target.p,
                           (uint32_t)n, scale, loss)))
    return rc;
  const float *g = (const float *)c->tr_g.p;
  if (out) HIP_TRY(hipMemcpyAsync(out, c->tr_out.p, 12 * n, hipMemcpyDeviceToHost, c->stream));
  if (grad_table) HIP_TRY(hipMemcpyAsync(grad_table, g, 4 * c->field_n_table, hipMemcpyDeviceToHost, c->stream));
  if (grad_weights)
    HIP_TRY(hipMemcpyAsync(grad_weights, g + c->field_n_table, 4ull * c->field_n_w, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

int mtx_field_train_step(mtx_ctx *c, uint64_t n, const float *p, const float *wi, const float *target,
                         mtx_train_stats *stats) {
  int rc = field_check(c, n);
  if (rc || (rc = train_check(c)) || (rc = train_fits(c))) return rc;
  if (n == 0 || !p || !wi || !target) {
    mtx_set_error("mtx_field_train_step: empty batch or null input");
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = field_stage_queries(c, n, p, wi))) return rc;
  if ((rc = upload(c->tr_target, target, 3 * n, c->stream))) return rc;
  double loss = 0.0;
  if ((rc = field_backward(c, (const float4 *)c->fq_p.p, (const float4 *)c->fq_d.p, (const float *)c->tr_target.p,
                           (uint32_t)n, c->scale, &loss)))
    return rc;
  mtx_train_stats st{};
  st.loss = loss;
  if ((rc = field_opt_step(c, &st))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (stats) *stats = st;
  return MTX_OK;
}

int mtx_field_params(mtx_ctx *c, float *table, float *weights, float *m, float *v) {
  int rc = train_check(c);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t nt = c->field_n_table, nw = c->field_n_w;
  if (table) HIP_TRY(hipMemcpy(table, c->tr_p.p, 4 * nt, hipMemcpyDeviceToHost));
  if (weights) HIP_TRY(hipMemcpy(weights, (const float *)c->tr_p.p + nt, 4 * nw, hipMemcpyDeviceToHost));
  if (m) HIP_TRY(hipMemcpy(m, c->tr_m.p, 4 * (nt + nw), hipMemcpyDeviceToHost));
  if (v) HIP_TRY(hipMemcpy(v, c->tr_v.p, 4 * (nt + nw), hipMemcpyDeviceToHost));
  return MTX_OK;
}

int mtx_nerad_upload(mtx_ctx *c, const mtx_nerad_tables *t) {
  if (!c || !t || !c->has_scene) {
    mtx_set_error("mtx_nerad_upload: null argument or no scene");
    return MTX_E_ARG;
  }
  const uint32_t S = t->n_shapes, E = t->n_entries;
  if (S != c->scene_n_shapes || !t->shape_pmf || !t->shape_cdf || !t->tri_off || !t->tri_pmf || !t->tri_cdf ||
      !t->tri_prim || !t->tri_sum || !t->tri_norm || !t->tri_valid || t->tri_off[S] != E ||
      t->shape_valid[0] > t->shape_valid[1] || t->shape_valid[1] >= S) {
    mtx_set_error("mtx_nerad_upload: tables do not match the scene (%u shapes)", c->scene_n_shapes);
    return MTX_E_ARG;
  }
  for (uint32_t k = 0; k < S; ++k) {
    const uint32_t cnt = t->tri_off[k + 1] - t->tri_off[k];
    if (t->tri_off[k + 1] < t->tri_off[k] || cnt == 0 || t->tri_valid[2 * k] > t->tri_valid[2 * k + 1] ||
        t->tri_valid[2 * k + 1] >= cnt) {
      mtx_set_error("mtx_nerad_upload: bad triangle range of shape %u", k);
      return MTX_E_ARG;
    }
  }
  for (uint32_t i = 0; i < E; ++i)
    if (t->tri_prim[i] >= c->scene.n_tris) {
      mtx_set_error("mtx_nerad_upload: tri_prim[%u] out of range", i);
      return MTX_E_ARG;
    }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if ((rc = upload(c->nr_shape_pmf, t->shape_pmf, S, c->stream))) return rc;
  if ((rc = upload(c->nr_shape_cdf, t->shape_cdf, S, c->stream))) return rc;
  if ((rc = upload(c->nr_tri_off, t->tri_off, S + 1, c->stream))) return rc;
  if ((rc = upload(c->nr_tri_pmf, t->tri_pmf, E, c->stream))) return rc;
  if ((rc = upload(c->nr_tri_cdf, t->tri_cdf, E, c->stream))) return rc;
  if ((rc = upload(c->nr_tri_prim, t->tri_prim, E, c->stream))) return rc;
  std::vector<mtx::DiscreteDist> d(S);
  for (uint32_t k = 0; k < S; ++k) {
    const uint32_t off = t->tri_off[k];
    d[k].pmf = (const float *)c->nr_tri_pmf.p + off;
    d[k].cdf = (const float *)c->nr_tri_cdf.p + off;
    d[k].n = t->tri_off[k + 1] - off;
    d[k].valid_lo = t->tri_valid[2 * k];
    d[k].valid_hi = t->tri_valid[2 * k + 1];
    d[k].sum = t->tri_sum[k];
    d[k].normalization = t->tri_norm[k];
  }
  if ((rc = upload(c->nr_dists, d.data(), S, c->stream))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  mtx::NeradTables &n = c->nr;
  n.shape.pmf = (const float *)c->nr_shape_pmf.p;
  n.shape.cdf = (const float *)c->nr_shape_cdf.p;
  n.shape.n = S;
  n.shape.valid_lo = t->shape_valid[0];
  n.shape.valid_hi = t->shape_valid[1];
  n.shape.sum = t->shape_sum;
  n.shape.normalization = t->shape_norm;
  n.tri_dist = (const mtx::DiscreteDist *)c->nr_dists.p;
  n.tri_off = (const uint32_t *)c->nr_tri_off.p;
  n.tri_prim = (const uint32_t *)c->nr_tri_prim.p;
  c->has_nerad = true;
  return MTX_OK;
}

int mtx_nerad_lhs(mtx_ctx *c, const mtx_nerad_args *a, float *out) {
  int rc = nerad_check(c, a, false);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = nerad_lhs_dev(c, a))) return rc;
  if (out) {
    std::vector<float> raw(12ull * a->batch);
    HIP_TRY(hipMemcpyAsync(raw.data(), c->nr_lhs.p, 48ull * a->batch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < a->batch; ++i) {
      const float *r = raw.data() + 12 * i;
      float *o = out + 9 * i;
      o[0] = r[3];  // prim bits
      o[1] = r[7];
      o[2] = r[8];
      o[3] = r[0];
      o[4] = r[1];
      o[5] = r[2];
      o[6] = r[4];
      o[7] = r[5];
      o[8] = r[6];
    }
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

int mtx_nerad_rhs(mtx_ctx *c, const mtx_nerad_args *a, float *L_rhs, float *lanes) {
  int rc = nerad_check(c, a);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = nerad_lhs_dev(c, a))) return rc;
  float *lanes_dev = nullptr;
  if (lanes) {
    if ((rc = dalloc(c->nr_lanes, 12ull * a->batch * a->M))) return rc;
    lanes_dev = (float *)c->nr_lanes.p;
  }
  if ((rc = nerad_rhs_dev(c, a, lanes_dev, nullptr))) return rc;
  if (L_rhs) HIP_TRY(hipMemcpyAsync(L_rhs, c->nr_Lrhs.p, 12ull * a->batch, hipMemcpyDeviceToHost, c->stream));
  if (lanes) HIP_TRY(hipMemcpyAsync(lanes, lanes_dev, 12ull * a->batch * a->M, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

int mtx_nerad_step(mtx_ctx *c, const mtx_nerad_args *a, mtx_train_stats *stats) {
  int rc = nerad_check(c, a);
  if (rc || (rc = train_check(c)) || (rc = train_fits(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  PhaseTimer pt(c->stream);
  pt.mark(0);
  if ((rc = nerad_lhs_dev(c, a))) return rc;  // si_lhs = isampler.sample(sampler_lhs) (:365)
  pt.mark(1);
  uint32_t nq = 0;
  mtx_train_stats st{};
  if ((rc = nerad_rhs_dev(c, a, nullptr, &nq, &st))) return rc;  // L_rhs = sample_rhs(si_lhs) (:368)
  pt.mark(2);
  double loss = 0.0;  // L_lhs = Field(si_lhs), loss, backward (:367-372)
  if ((rc = field_backward(c, (const float4 *)c->nr_qp.p, (const float4 *)c->nr_qd.p, (const float *)c->nr_Lrhs.p,
                           a->batch, c->scale, &loss)))
    return rc;
  st.loss = loss;
  if ((rc = field_opt_step(c, &st))) return rc;  // scaler.step(opt) (:373)
  pt.mark(3);
  HIP_TRY(hipStreamSynchronize(c->stream));
  st.rhs_queries = nq;
  st.ms_lhs = pt.ms(0, 1);
  st.ms_rhs = pt.ms(1, 2);
  st.ms_train = pt.ms(2, 3);
  st.ms_total = pt.ms(0, 3);
  if (stats) *stats = st;
  return MTX_OK;
}

}  // extern "C"

// ----------------------------- building blocks -----------------------------
// One entry per kernel group of blocks.hip. Order: argument checks,
// need_device on every pointer before anything touches it, the launch on the
// context's stream, the stream drained, then the device counter of lanes
// whose index lay outside the scene's tables (the kernels treat those as
// invalid and never index with them).

static int blk_begin(mtx_ctx *c, const char *fn, uint64_t n, bool scene, std::initializer_list<const void *> need) {
  if (!c) {
    mtx_set_error("%s: null context", fn);
    return MTX_E_ARG;
  }
  if (scene && !c->has_scene) {
    mtx_set_error("no scene uploaded");
    return MTX_E_NOSCENE;
  }
  if (n >= (1ull << 31)) {
    mtx_set_error("%s: n >= 2^31", fn);
    return MTX_E_ARG;
  }
  if (n == 0) return MTX_OK;
  for (const void *p : need)
    if (!p) {
      mtx_set_error("%s: null argument", fn);
      return MTX_E_ARG;
    }
  HIP_TRY(hipSetDevice(c->device));
  return MTX_OK;
}
static int blk_bad_reset(mtx_ctx *c) {
  if (int rc = dalloc(c->s6, 64)) return rc;
  HIP_TRY(hipMemsetAsync(c->s6.p, 0, 4, c->stream));
  return MTX_OK;
}
static int blk_end(mtx_ctx *c, const char *fn, const char *what) {
  HIP_TRY(hipGetLastError());
  uint32_t bad = 0;
  if (what) HIP_TRY(hipMemcpyAsync(&bad, c->s6.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (bad) {
    mtx_set_error("%s: %u lanes with %s (handled as invalid)", fn, bad, what);
    return MTX_E_ARG;
  }
  return MTX_OK;
}
static int si_need_device(mtx_ctx *c, const char *fn, const mtx_si_planes *si) {
  if (!si->p || !si->n || !si->sh_n || !si->uv || !si->wi || !si->t || !si->prim || !si->material || !si->emitter) {
    mtx_set_error("%s: null interaction plane", fn);
    return MTX_E_ARG;
  }
  return need_device(c, fn, {si->p, si->n, si->sh_n, si->uv, si->wi, si->t, si->prim, si->material, si->emitter,
                             si->bary});
}

extern "C" {

int mtx_blocks_sampler_seed_dev(mtx_ctx *c, uint64_t n, uint32_t seed, const uint32_t *lanes, uint32_t skip,
                                uint64_t *state) {
  const char *fn = "mtx_blocks_sampler_seed_dev";
  int rc = blk_begin(c, fn, n, false, {lanes, state});
  if (rc || n == 0) return rc;
  if ((rc = need_device(c, fn, {lanes, state}))) return rc;
  mtxd::launch_blk_seed((uint32_t)n, seed, lanes, skip, state, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_sampler_next_dev(mtx_ctx *c, uint64_t n, uint64_t *state, int dims, float *out) {
  const char *fn = "mtx_blocks_sampler_next_dev";
  int rc = blk_begin(c, fn, n, false, {state, out});
  if (rc) return rc;
  if (dims != 1 && dims != 2) {
    mtx_set_error("%s: dims %d (1 or 2)", fn, dims);
    return MTX_E_ARG;
  }
  if (n == 0) return MTX_OK;
  if ((rc = need_device(c, fn, {state, out}))) return rc;
  mtxd::launch_blk_next((uint32_t)n, state, dims, out, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_ray_intersect_dev(mtx_ctx *c, uint64_t n, const float *o, const float *d, const float *maxt,
                                 const uint8_t *active, const mtx_si_planes *si) {
  const char *fn = "mtx_blocks_ray_intersect_dev";
  int rc = blk_begin(c, fn, n, true, {o, d, si});
  if (rc || n == 0) return rc;
  if ((rc = need_device(c, fn, {o, d, maxt, active})) || (rc = si_need_device(c, fn, si))) return rc;
  // the traversal yields its own prim: nothing to range-check, no counter
  mtxd::launch_blk_interact(c->scene, (uint32_t)n, 1, o, d, maxt, nullptr, nullptr, nullptr, nullptr, active, *si,
                            nullptr, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_ray_test_dev(mtx_ctx *c, uint64_t n, const float *o, const float *d, const float *maxt,
                            const uint8_t *active, uint8_t *out) {
  const char *fn = "mtx_blocks_ray_test_dev";
  int rc = blk_begin(c, fn, n, true, {o, d, maxt, out});
  if (rc || n == 0) return rc;
  if ((rc = need_device(c, fn, {o, d, maxt, active, out}))) return rc;
  mtxd::launch_blk_ray_test(c->scene, (uint32_t)n, o, d, maxt, active, out, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_interact_dev(mtx_ctx *c, uint64_t n, const float *d, const float *t, const uint32_t *prim,
                            const float *u, const float *v, const uint8_t *active, const mtx_si_planes *si) {
  const char *fn = "mtx_blocks_interact_dev";
  int rc = blk_begin(c, fn, n, true, {d, t, prim, u, v, si});
  if (rc || n == 0) return rc;
  if ((rc = need_device(c, fn, {d, t, prim, u, v, active})) || (rc = si_need_device(c, fn, si)) ||
      (rc = blk_bad_reset(c)))
    return rc;
  mtxd::launch_blk_interact(c->scene, (uint32_t)n, 0, nullptr, d, nullptr, t, prim, u, v, active, *si,
                            (uint32_t *)c->s6.p, c->stream);
  return blk_end(c, fn, "a prim that is neither a triangle of the scene nor 0xffffffff");
}

int mtx_blocks_spawn_dev(mtx_ctx *c, uint64_t n, const float *p, const float *nrm, const float *x, int to, float *o,
                         float *d, float *maxt) {
  const char *fn = "mtx_blocks_spawn_dev";
  int rc = blk_begin(c, fn, n, false, {p, nrm, x, o, d, maxt});
  if (rc || n == 0) return rc;
  if ((rc = need_device(c, fn, {p, nrm, x, o, d, maxt}))) return rc;
  mtxd::launch_blk_spawn((uint32_t)n, p, nrm, x, to != 0, o, d, maxt, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_sample_emitter_dev(mtx_ctx *c, uint64_t n, const float *p, const float *nrm, const float *u,
                                  const uint8_t *active, int test_visibility, const mtx_ds_planes *ds,
                                  float *weight) {
  const char *fn = "mtx_blocks_sample_emitter_dev";
  int rc = blk_begin(c, fn, n, true, {p, u, ds, weight});
  if (rc || n == 0) return rc;
  if (!ds->p || !ds->n || !ds->d || !ds->dist || !ds->pdf || !ds->emitter || (test_visibility && !nrm)) {
    mtx_set_error("%s: null argument", fn);
    return MTX_E_ARG;
  }
  if ((rc = need_device(c, fn, {p, nrm, u, active, ds->p, ds->n, ds->d, ds->dist, ds->pdf, ds->emitter, weight})))
    return rc;
  mtxd::launch_blk_sample_emitter(c->scene, (uint32_t)n, p, nrm, u, active, test_visibility != 0, *ds, weight,
                                  c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_emitter_dev(mtx_ctx *c, uint64_t n, const int32_t *emitter, const float *d, const float *dist,
                           const float *nrm, const float *wi, const uint8_t *active, float *pdf, float *le) {
  const char *fn = "mtx_blocks_emitter_dev";
  int rc = blk_begin(c, fn, n, true, {emitter});
  if (rc || n == 0) return rc;
  if ((!pdf && !le) || (pdf && (!d || !dist || !nrm)) || (le && !wi)) {
    mtx_set_error("%s: null argument", fn);
    return MTX_E_ARG;
  }
  if ((rc = need_device(c, fn, {emitter, d, dist, nrm, wi, active, pdf, le})) || (rc = blk_bad_reset(c))) return rc;
  mtxd::launch_blk_emitter(c->scene, (uint32_t)n, emitter, d, dist, nrm, wi, active, pdf, le, (uint32_t *)c->s6.p,
                           c->stream);
  return blk_end(c, fn, "an emitter index past the scene's emitters");
}

int mtx_blocks_bsdf_dev(mtx_ctx *c, uint64_t n, const int32_t *material, const float *uv, const float *wi,
                        const float *wo, const float *u1, const float *u2, const uint8_t *active,
                        const mtx_bsdf_planes *out, uint32_t *flags) {
  const char *fn = "mtx_blocks_bsdf_dev";
  int rc = blk_begin(c, fn, n, true, {material});
  if (rc || n == 0) return rc;
  mtx_bsdf_planes o{};
  if (out) {
    o = *out;
    if (!uv || !wi || !wo || !u1 || !u2 || !o.value || !o.pdf || !o.s_wo || !o.s_pdf || !o.s_eta || !o.s_type ||
        !o.weight) {
      mtx_set_error("%s: null argument", fn);
      return MTX_E_ARG;
    }
  } else if (!flags) {
    mtx_set_error("%s: neither outputs nor flags", fn);
    return MTX_E_ARG;
  }
  if ((rc = need_device(c, fn, {material, uv, wi, wo, u1, u2, active, o.value, o.pdf, o.s_wo, o.s_pdf, o.s_eta,
                                o.s_type, o.weight, flags})) ||
      (rc = blk_bad_reset(c)))
    return rc;
  mtxd::launch_blk_bsdf(c->scene, c->scene_n_materials, (uint32_t)n, material, uv, wi, wo, u1, u2, active, o, flags,
                        (uint32_t *)c->s6.p, c->stream);
  return blk_end(c, fn, "a material index past the scene's materials");
}

int mtx_blocks_math_dev(mtx_ctx *c, int op, uint64_t n, const float *a, const float *b, const float *cc, float *out) {
  const char *fn = "mtx_blocks_math_dev";
  int rc = blk_begin(c, fn, n, false, {a, out});
  if (rc) return rc;
  const bool need_b = op != MTX_MATH_RCP && op != MTX_MATH_SQRT && op != MTX_MATH_NORM3 && op != MTX_MATH_NORMALIZE3;
  if (op < MTX_MATH_FMA || op > MTX_MATH_MIS_B) {
    mtx_set_error("%s: unknown op %d", fn, op);
    return MTX_E_ARG;
  }
  if (n == 0) return MTX_OK;
  if ((need_b && !b) || (op == MTX_MATH_FMA && !cc)) {
    mtx_set_error("%s: null argument", fn);
    return MTX_E_ARG;
  }
  if ((rc = need_device(c, fn, {a, b, cc, out}))) return rc;
  mtxd::launch_blk_math(op, (uint32_t)n, a, b, cc, out, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_sensor_ray_dev(mtx_ctx *c, uint64_t n, const float *pos, const uint8_t *active, float *o, float *d,
                              float *maxt) {
  const char *fn = "mtx_blocks_sensor_ray_dev";
  int rc = blk_begin(c, fn, n, true, {pos, o, d});
  if (rc || n == 0) return rc;
  if ((rc = need_device(c, fn, {pos, active, o, d, maxt}))) return rc;
  mtxd::launch_blk_sensor_ray(c->scene.camera, (uint32_t)n, pos, active, o, d, maxt, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_sample_emitter_ray_dev(mtx_ctx *c, uint64_t n, const float *u_pos, const float *u_dir,
                                      const uint8_t *active, float *o, float *d, float *maxt, float *weight, float *p,
                                      float *nrm, int32_t *emitter) {
  const char *fn = "mtx_blocks_sample_emitter_ray_dev";
  int rc = blk_begin(c, fn, n, true, {u_pos, u_dir, o, d, maxt, weight, p, nrm, emitter});
  if (rc || n == 0) return rc;
  if ((rc = need_device(c, fn, {u_pos, u_dir, active, o, d, maxt, weight, p, nrm, emitter}))) return rc;
  mtxd::launch_blk_sample_emitter_ray(c->scene, (uint32_t)n, u_pos, u_dir, active,
                                      mtxd::EmitterRayPlanes{o, d, maxt, weight, p, nrm, emitter}, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_sensor_direction_dev(mtx_ctx *c, uint64_t n, const float *p, const float *nrm, const uint8_t *active,
                                    int test_visibility, float *pos, float *d, float *dist, float *weight,
                                    uint8_t *valid) {
  const char *fn = "mtx_blocks_sensor_direction_dev";
  int rc = blk_begin(c, fn, n, true, {p, pos, d, dist, weight, valid});
  if (rc || n == 0) return rc;
  if (test_visibility && !nrm) {
    mtx_set_error("%s: null argument", fn);
    return MTX_E_ARG;
  }
  if ((rc = need_device(c, fn, {p, nrm, active, pos, d, dist, weight, valid}))) return rc;
  mtxd::launch_blk_sensor_direction(c->scene, (uint32_t)n, p, nrm, active, test_visibility != 0,
                                    mtxd::SensorDirPlanes{pos, d, dist, weight, valid}, c->stream);
  return blk_end(c, fn, nullptr);
}

// The host twin of the two kernels above: the same per-lane functions over a
// host scene description, one item after the other.
int mtx_blocks_light_host(const mtx_scene_desc *d, int op, uint64_t n, const float *in, float *out) {
  const char *fn = "mtx_blocks_light_host";
  if (!d || (n && (!in || !out))) {
    mtx_set_error("%s: null argument", fn);
    return MTX_E_ARG;
  }
  if (n >= (1ull << 31)) {
    mtx_set_error("%s: n >= 2^31", fn);
    return MTX_E_ARG;
  }
  const auto in_at = [&](int c, uint64_t i) { return in[(size_t)c * n + i]; };
  const auto put = [&](int c, uint64_t i, float v) { out[(size_t)c * n + i] = v; };
  const auto put3 = [&](int c, uint64_t i, mtx::V3 v) {
    put(c, i, v.x);
    put(c + 1, i, v.y);
    put(c + 2, i, v.z);
  };
  if (op == MTX_LIGHT_EMITTER_RAY) {
    if (d->n_emitters && (!d->emitters || !d->vpos || !d->tri_vidx || !d->tri_shape || !d->shapes)) {
      mtx_set_error("%s: the emitters need the scene's emitter, shape and vertex arrays", fn);
      return MTX_E_ARG;
    }
    if (d->n_emitters)  // no table or triangle index is trusted
      if (int rc = check_mesh_emitters(d)) return rc;
    for (uint32_t e = 0; e < d->n_emitters; ++e)
      if (mtx::emitter_is_mesh(d->emitters[e]))
        for (uint32_t k = 0; k < d->emitters[e].mesh_count; ++k) {
          uint32_t prim;
          memcpy(&prim, d->tables + d->emitters[e].mesh_offset + 2 * (size_t)d->emitters[e].mesh_count + k, 4);
          for (int j = 0; j < 3; ++j)
            if (d->tri_vidx[3 * (size_t)prim + j] >= d->n_verts) {
              mtx_set_error("%s: triangle %u names vertex %u of %u", fn, prim, d->tri_vidx[3 * (size_t)prim + j],
                            d->n_verts);
              return MTX_E_ARG;
            }
        }
    mtx::SceneView s{};
    s.tri_vidx = d->tri_vidx;
    s.tri_shape = d->tri_shape;
    s.vpos = d->vpos;
    s.shapes = d->shapes;
    s.emitters = d->emitters;
    s.bsdf.tables = d->tables;
    s.n_tris = d->n_tris;
    s.n_emitters = d->n_emitters;
    s.has_env = d->has_env ? 1u : 0u;
    for (int k = 0; k < 3; ++k) s.env_radiance[k] = d->env_radiance[k];
    if (s.has_env) mtx::env_bsphere(d->vpos, d->vpos ? d->n_verts : 0, s.env_center, &s.env_radius);
    for (uint64_t i = 0; i < n; ++i) {
      mtx::EmitterRaySample es;
      mtx::sample_emitter_ray(s, mtx::V2{in_at(0, i), in_at(1, i)}, mtx::V2{in_at(2, i), in_at(3, i)}, &es);
      put3(0, i, es.ray.o);
      put3(3, i, es.ray.d);
      put(6, i, es.ray.maxt);
      put3(7, i, es.weight);
      put3(10, i, es.p);
      put3(13, i, es.n);
      put(16, i, mtx::u2f((uint32_t)es.emitter));
    }
    return MTX_OK;
  }
  if (op == MTX_LIGHT_SENSOR_DIRECTION || op == MTX_LIGHT_PROJECT) {
    for (uint64_t i = 0; i < n; ++i) {
      const mtx::V3 p = mtx::V3{in_at(0, i), in_at(1, i), in_at(2, i)};
      if (op == MTX_LIGHT_PROJECT) {
        float ux = 0.f, uy = 0.f;
        const bool ok = mtx::project_prev(d->camera, p, &ux, &uy);
        put(0, i, ok ? ux : 0.f);
        put(1, i, ok ? uy : 0.f);
        put(2, i, mtx::u2f(ok ? 1u : 0u));
        continue;
      }
      mtx::SensorDirectionSample sd;
      mtx::camera_sample_direction(d->camera, p, &sd);
      put(0, i, sd.pos.x);
      put(1, i, sd.pos.y);
      put3(2, i, sd.d);
      put(5, i, sd.dist);
      put(6, i, sd.weight);
      put(7, i, mtx::u2f(sd.valid ? 1u : 0u));
    }
    return MTX_OK;
  }
  mtx_set_error("%s: unknown op %d", fn, op);
  return MTX_E_ARG;
}

}  // extern "C"

// The arguments the two bdpt entries share: both stores complete and of one
// depth, the strategy inside it.
static int bdpt_check(const char *fn, const mtx_path_planes *cam, const mtx_path_planes *lit, int s, int t,
                      uint32_t max_depth, uint32_t flags, const float *L, const float *weight) {
  if (!cam || !lit || !L) {
    mtx_set_error("%s: null argument", fn);
    return MTX_E_ARG;
  }
  for (const mtx_path_planes *q : {cam, lit})
    if (!q->len || !q->p || !q->n || !q->sh_n || !q->wi || !q->uv || !q->material || !q->emitter || !q->beta ||
        !q->pdf_fwd || !q->pdf_rev || !q->delta) {
      mtx_set_error("%s: null plane in the %s store", fn, q == cam ? "camera" : "light");
      return MTX_E_ARG;
    }
  if (cam->depth != lit->depth || cam->depth < 2 || cam->depth > (1u << 16)) {
    mtx_set_error("%s: depth mismatch: the camera store holds %u vertices per lane, the light store %u (one depth in "
                  "[2, 65536] expected)", fn, cam->depth, lit->depth);
    return MTX_E_ARG;
  }
  if (max_depth == 0) {
    mtx_set_error("%s: max_depth = 0 (a path has at least one segment)", fn);
    return MTX_E_ARG;
  }
  if (flags & ~(uint32_t)(MTX_BDPT_MIS | MTX_BDPT_VISIBILITY)) {
    mtx_set_error("%s: unknown flags 0x%x", fn, flags);
    return MTX_E_ARG;
  }
  const bool all = s == -1 && t == -1;
  if (all && weight) {
    mtx_set_error("%s: weight requested with s = t = -1 (a weight belongs to one strategy)", fn);
    return MTX_E_ARG;
  }
  if (!all) {
    if (t == 0 || t == 1) {
      mtx_set_error("%s: t = %d: only strategies with t >= 2 exist (t = 1 splats onto the film, t = 0 needs a sensor "
                    "with an area)", fn, t);
      return MTX_E_ARG;
    }
    if (s < 0 || t < 0 || (uint32_t)s > cam->depth || (uint32_t)t > cam->depth) {
      mtx_set_error("%s: strategy (s = %d, t = %d) outside the stores' depth %u", fn, s, t, cam->depth);
      return MTX_E_ARG;
    }
  }
  return MTX_OK;
}

extern "C" {

int mtx_blocks_bdpt_connect_dev(mtx_ctx *c, uint64_t n, const mtx_path_planes *cam, const mtx_path_planes *lit, int s,
                                int t, uint32_t max_depth, uint32_t flags, const uint8_t *active, float *L,
                                float *weight) {
  const char *fn = "mtx_blocks_bdpt_connect_dev";
  int rc = blk_begin(c, fn, n, true, {cam, lit, L});
  if (rc || n == 0) return rc;
  if ((rc = bdpt_check(fn, cam, lit, s, t, max_depth, flags, L, weight))) return rc;
  if ((uint64_t)cam->depth * 3 * n >= (1ull << 40)) {
    mtx_set_error("%s: store too large", fn);
    return MTX_E_ARG;
  }
  for (const mtx_path_planes *q : {cam, lit})
    if ((rc = need_device(c, fn, {q->len, q->p, q->n, q->sh_n, q->wi, q->uv, q->material, q->emitter, q->beta,
                                  q->pdf_fwd, q->pdf_rev, q->delta})))
      return rc;
  if ((rc = need_device(c, fn, {active, L, weight})) || (rc = blk_bad_reset(c))) return rc;
  mtxd::launch_blk_bdpt_connect(c->scene, c->scene_n_materials, (uint32_t)n, *cam, *lit, s, t, max_depth, flags,
                                active, L, weight, (uint32_t *)c->s6.p, c->stream);
  return blk_end(c, fn, "a vertex whose material or emitter index lies past the scene's tables");
}

int mtx_blocks_bdpt_host(const mtx_scene_desc *d, uint64_t n, const mtx_path_planes *cam, const mtx_path_planes *lit,
                         int s, int t, uint32_t max_depth, uint32_t flags, float *L, float *weight) {
  const char *fn = "mtx_blocks_bdpt_host";
  if (!d) {
    mtx_set_error("%s: null argument", fn);
    return MTX_E_ARG;
  }
  if (n >= (1ull << 31)) {
    mtx_set_error("%s: n >= 2^31", fn);
    return MTX_E_ARG;
  }
  if (flags & MTX_BDPT_VISIBILITY) {
    mtx_set_error("%s: MTX_BDPT_VISIBILITY: the host twin has no traversal; test visibility on the device", fn);
    return MTX_E_ARG;
  }
  if (n == 0) return MTX_OK;
  if (int rc = bdpt_check(fn, cam, lit, s, t, max_depth, flags, L, weight)) return rc;
  if ((d->n_materials && !d->materials) || (d->n_emitters && !d->emitters)) {
    mtx_set_error("%s: the description lacks its material or emitter array", fn);
    return MTX_E_ARG;
  }
  for (uint32_t i = 0; i < d->n_materials; ++i) {  // what a BSDF evaluation reads, as mtx_scene_upload checks it
    const mtx_material &m = d->materials[i];
    if (m.tex >= 0) {
      if ((uint32_t)m.tex >= d->n_textures || !d->textures || !d->texels ||
          d->textures[m.tex].offset + 3ull * d->textures[m.tex].width * d->textures[m.tex].height > d->n_texels ||
          d->textures[m.tex].width == 0 || d->textures[m.tex].height == 0) {
        mtx_set_error("%s: material %u texture out of range", fn, i);
        return MTX_E_ARG;
      }
    }
    if (m.type == MTX_MAT_ROUGHPLASTIC &&
        (m.table < 0 || !d->tables || (uint32_t)m.table + MTX_ROUGH_TRANSMITTANCE_RES > d->n_tables)) {
      mtx_set_error("%s: roughplastic material %u has no transmittance table", fn, i);
      return MTX_E_ARG;
    }
  }
  mtx::SceneView sv{};
  sv.materials = d->materials;
  sv.emitters = d->emitters;
  sv.bsdf.textures = d->textures;
  sv.bsdf.texels = d->texels;
  sv.bsdf.tables = d->tables;
  sv.n_tris = d->n_tris;
  sv.n_emitters = d->n_emitters;
  sv.has_env = d->has_env ? 1u : 0u;
  const auto never = [](const mtx::Ray &) { return false; };
  for (uint64_t i = 0; i < n; ++i) {
    const mtx::PathLane zc = mtx::path_lane(cam, n, i), yl = mtx::path_lane(lit, n, i);
    float w = 0.f;
    const mtx::V3 l = mtx::bdpt_connect(sv, d->n_materials, zc, yl, s, t, max_depth, (flags & MTX_BDPT_MIS) != 0, never,
                                        &w);
    L[i] = l.x;
    L[n + i] = l.y;
    L[2 * n + i] = l.z;
    if (weight) weight[i] = w;
  }
  return MTX_OK;
}

}  // extern "C"

// The band and filter of a caller-owned film: checked, never trusted.
static int film_band(const char *fn, uint32_t width, uint32_t y0, uint32_t y1, uint32_t rfilter, mtxd::FilmBand *g) {
  if (mtx::rfilter_reach(rfilter) == 0xffffffffu) {
    mtx_set_error("%s: unknown reconstruction filter %u", fn, rfilter);
    return MTX_E_ARG;
  }
  if (width == 0 || y1 <= y0 || (uint64_t)(y1 - y0) * width >= (1ull << 31) || (uint64_t)y1 * width >= (1ull << 31) ||
      width >= (1u << 24) || y1 >= (1u << 24)) {
    mtx_set_error("%s: bad film band (width %u, rows [%u, %u))", fn, width, y0, y1);
    return MTX_E_ARG;
  }
  *g = mtxd::FilmBand{width, y0, y1, (y1 - y0) * width, rfilter};
  return MTX_OK;
}

extern "C" {

int mtx_blocks_film_put_dev(mtx_ctx *c, float *planes, uint32_t width, uint32_t y0, uint32_t y1, uint32_t rfilter,
                            uint64_t n, const float *pos, const float *L, const uint8_t *active, uint32_t spp_total,
                            uint32_t sample_offset, uint32_t pixel_major_spp, uint32_t px0, uint64_t *dropped) {
  const char *fn = "mtx_blocks_film_put_dev";
  if (dropped) *dropped = 0;
  int rc = blk_begin(c, fn, n, false, {planes, pos, L});
  if (rc) return rc;
  mtxd::FilmBand g;
  if ((rc = film_band(fn, width, y0, y1, rfilter, &g))) return rc;
  if (n == 0) return MTX_OK;
  if (sample_offset + n >= (1ull << 32)) {
    mtx_set_error("%s: sample_offset + n >= 2^32", fn);
    return MTX_E_ARG;
  }
  const uint32_t s = pixel_major_spp;
  if (s) {
    if (n % s || px0 < y0 * width || (uint64_t)px0 + n / s > (uint64_t)y1 * width) {
      mtx_set_error("%s: pixel-major layout: n = %llu is not a multiple of %u samples, or the pixels [%u, %llu) leave "
                    "the band", fn, (unsigned long long)n, s, px0, (unsigned long long)px0 + n / s);
      return MTX_E_ARG;
    }
    if (spp_total && (uint64_t)sample_offset + s > spp_total) {
      mtx_set_error("%s: sample_offset %u + %u samples > spp_total %u", fn, sample_offset, s, spp_total);
      return MTX_E_ARG;
    }
  }
  if ((rc = need_device(c, fn, {planes, pos, L, active})) || (rc = dalloc(c->s0, 64))) return rc;
  uint32_t *counts = (uint32_t *)c->s0.p;
  uint32_t h[mtxd::kPutCounters] = {0, 0, 0};
  HIP_TRY(hipMemsetAsync(counts, 0, sizeof h, c->stream));
  if (s) {
    mtxd::launch_blk_film_claim(g, (uint32_t)n, pos, active, s, px0, counts, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, counts, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h[mtxd::kPutViolations]) {
      mtx_set_error("%s: %u lanes whose position lies outside the pixel the pixel-major layout gives them (%u "
                    "samples per pixel from pixel %u); the planes are unchanged", fn, h[mtxd::kPutViolations], s, px0);
      return MTX_E_ARG;
    }
    mtxd::launch_blk_film_put_staged(g, (uint32_t)n, pos, L, active, s, px0, spp_total, sample_offset,
                                     h[mtxd::kPutOff] != 0, (float4 *)planes, c->stream);
  } else {
    const uint32_t n_keys = g.band_px + 1;  // the last key: inactive and dropped lanes
    if ((rc = dalloc(c->s1, 4 * n)) || (rc = dalloc(c->s2, 4ull * n_keys)) || (rc = dalloc(c->s3, 4ull * n_keys)) ||
        (rc = dalloc(c->s4, 4 * n)) || (rc = dalloc(c->s5, mtxd::hashgrid_workspace_bytes(n, n_keys))))
      return rc;
    uint32_t *keys = (uint32_t *)c->s1.p, *ksize = (uint32_t *)c->s2.p, *koff = (uint32_t *)c->s3.p;
    uint32_t *order = (uint32_t *)c->s4.p;
    mtxd::launch_blk_film_keys(g, (uint32_t)n, pos, active, keys, counts, c->stream);
    HIP_TRY(hipGetLastError());
    if ((rc = mtxd::group_by_u32(keys, n, n_keys, ksize, koff, order, c->s5.p, c->stream))) return rc;
    mtxd::launch_blk_film_put(g, (uint32_t)n, pos, L, ksize, koff, order, spp_total, sample_offset, (float4 *)planes,
                              c->stream);
    HIP_TRY(hipMemcpyAsync(h, counts, sizeof h, hipMemcpyDeviceToHost, c->stream));
  }
  if ((rc = blk_end(c, fn, nullptr))) return rc;
  if (dropped) *dropped = h[mtxd::kPutDropped];
  return MTX_OK;
}

int mtx_blocks_film_gather_dev(mtx_ctx *c, const float *planes, uint32_t width, uint32_t y0, uint32_t y1,
                               uint32_t rfilter, float *film) {
  const char *fn = "mtx_blocks_film_gather_dev";
  int rc = blk_begin(c, fn, 1, false, {planes, film});
  if (rc) return rc;
  mtxd::FilmBand g;
  if ((rc = film_band(fn, width, y0, y1, rfilter, &g))) return rc;
  const uint64_t b = mtx::rfilter_reach(rfilter);
  if ((width + 2 * b) * (y1 - y0 + 2 * b) >= (1ull << 31)) {
    mtx_set_error("%s: film too large", fn);
    return MTX_E_ARG;
  }
  if ((rc = need_device(c, fn, {planes, film}))) return rc;
  mtxd::launch_film_gather((const float4 *)planes, (float4 *)film, width, y0, y1, 8, 0xffu, rfilter, c->stream);
  return blk_end(c, fn, nullptr);
}

}  // extern "C"
