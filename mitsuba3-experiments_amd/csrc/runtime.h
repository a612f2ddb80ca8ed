// runtime.h — what the host translation units of libmtx share (internal, host
// only): the HIP error macro, device buffers, the wavefront, the context and
// its per-subsystem state, and the helpers more than one file calls. Which
// file holds what: DESIGN.md "Host runtime layout".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <utility>
#include <vector>

#include "mtx.h"
#include "mtx_core/field.h"
#include "mtx_core/nerad.h"
#include "refit.h"
#include "wavefront.h"

void mtx_set_error(const char *fmt, ...);  // error.cpp

#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      mtx_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return MTX_E_HIP;                                                                           \
    }                                                                                             \
  } while (0)

namespace mtxh {

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

int dalloc(DevBuf &b, size_t bytes);  // grows only: a buffer that is large enough stays
void dfree(DevBuf &b);

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

// Tuning knobs. Filled once, from the environment, by read_knobs
// (context.cpp) at context creation; nothing changes them afterwards. The
// scene's copies (DevScene::trace_batch, ...) are taken at upload.
struct Knobs {
  uint32_t streams = MTX_STREAMS;  // 1: every chunk on the context's stream (MTX_STREAMS env: A/B)
  uint32_t streams_max_log2 = 27;  // two streams for renders of <= 2^this paths (MTX_STREAMS_MAX_LOG2: A/B)
  // LDS stack entries of the persistent traversal, chunk path order
  uint32_t lds_stack = mtxd::kLdsStack;
  uint32_t lds_top = MTX_LDS_TOP;          // closest-hit tree nodes kept in LDS per block (MTX_LDS_TOP env: A/B)
  uint32_t occ_lds_top = MTX_OCC_LDS_TOP;  // occlusion tree nodes kept in LDS per block (MTX_OCC_LDS_TOP)
  uint32_t occ_lds_stack = mtxd::kOccLdsStack;
  uint32_t trace_batch = 128;  // queue entries per claim (256: +0.6 % closest, +1 % at spp 32; 64: +5 %)
  uint32_t urefill = 24;  // refill a wave once 24 lanes are idle (16: closest +1.3 %, 32: +2 %; 4-wide BVH)
  uint32_t cam_urefill = 64;  // k_trace_camera (MTX_CAM_UREFILL): whole waves refill; a refill derives its camera rays
  uint32_t occ_urefill = 12;  // any hit on the 8-wide tree (MTX_OCC_UREFILL; 8-16 alike, 24: shadow +1 ms, 32/40: +2/+3 ms)
  // k_trace_closest: prepared rays per wave in LDS (MTX_TRACE_RING: 0 = none, urefill refills; 16; 32). The
  // rings take their bytes from that kernel's LDS stack entries (wavefront.h split_trace_lds).
  uint32_t trace_ring = MTX_TRACE_RING;
  // k_shade<path-mis / path>: class-uniform block steps from per-block LDS class queues (MTX_SHADE_CLASSES:
  // 0 = the mixed loop, kept as the form the class queues are tested and measured against; 1)
  uint32_t shade_classes = MTX_SHADE_CLASSES;
  uint32_t xcd_claim = 1;
  // ReSTIR GI: a band of at most this many paths runs its stage A in the
  // per-lane megakernel on one wavefront (MTX_MEGA_PATHS, 0 = off; default
  // 0xffffffff = twice the resident lanes of the megakernel's grid,
  // 2 x mega_grid x kShadeBlock)
  uint32_t mega_paths = 0xffffffffu;
  // such a band's whole stage A (raygen .. collect) in one per-lane launch
  // (mega.hip k_rs_stage_a; MTX_RS_FUSED=0: raygen, trace, k_rs_begin, the
  // megakernel and k_rs_collect as separate launches)
  uint32_t rs_fused = 1;
  // NRC cache query order: MTX_CACHE_SORT=1 Morton-sorted (host sync; measured slower), 2 grouped
  // by region on the device with one eighth of the rows per XCD (field.hip)
  uint32_t cache_sort = MTX_CACHE_SORT;
  // NRC cache encoder: level-major lanes (field.hip k_field_encode_lm; MTX_ENCODE_LM=0: query-major)
  uint32_t encode_lm = MTX_ENCODE_LM;
  // NRC cache: encode + MLP + apply in one launch (field.hip k_field_cache_fused; MTX_CACHE_FUSED=0: three)
  uint32_t cache_fused = 1;
};

// The uploaded scene. Filled by mtx_scene_upload's device phase (scene.cpp)
// from a description scene_check accepted; mtx_scene_update_vertices rewrites
// the geometry in place and mtx_set_camera the camera. `live` is false from
// the first device write of an upload (or a refit that failed midway) until
// an upload completes: mtx_ctx::scene_dropped.
struct SceneState {
  DevBuf shade_rec;  // per-triangle shading records
  DevBuf nodes, tri, occ_nodes, occ_tri, tri_vidx, tri_shape, vpos, vnormal, vuv, shapes, materials, emitters, textures,
      texels, tables;
  mtxd::DevScene dev{};  // the kernels' view of the buffers above
  uint32_t n_shapes = 0;
  uint32_t n_materials = 0;  // bound of the material indices the building blocks take (blocks.hip)
  uint32_t n_nodes = 0, n_occ = 0, n_verts = 0, n_tables = 0;
  bool live = false;
};

// What mtx_scene_update_vertices needs beyond the scene: the occlusion tree's
// leaf order -> scene triangle, and the levels of both trees: level l is nodes
// [first[l], first[l + 1]) -- the builder's breadth-first layout -- or, for
// trees whose levels are not contiguous, those entries of the device list.
// Lists, levels and the em_* tables are written by every upload and belong to
// that scene; the scratch (staged input, triangle and node boxes) is
// allocated by the first update and only ever grows.
struct RefitState {
  DevBuf occ_perm, lvl4_list, lvl8_list;
  std::vector<uint32_t> lvl4_first, lvl8_first;
  DevBuf state, tbox, nbox, vpos, vnormal;  // scratch of an update
  // mesh emitter tables of a vertex update (refit.h EmTables): lists and scratch, sized at upload
  DevBuf em_slots, em_blocks, em_state, em_pmf, em_cdf, em_bsum, em_bstat;
  mtxd::EmTables em_tables = {};
};

// The radiance field. Filled by mtx_field_upload (field_entry.cpp); a training
// step rewrites table, w16 and frag in place. Independent of the scene.
struct FieldState {
  DevBuf table, frag, fq_p, fq_d;  // fp16 table, MFMA-packed weights, the field entry points' staged queries
  DevBuf w16;                      // plain fp16 weights (training forward / backward)
  mtx::FieldEncoding enc{};
  uint32_t hidden = 0;
  uint32_t n_in = 0, n_w = 0;
  uint64_t n_table = 0;  // fp16 table entries
  bool live = false;
};

// Field training. Started by mtx_field_train_init for the field then
// uploaded: fp32 master parameters [table | weights], Adam moments,
// gradients, per-batch scratch. A new field ends it: mtx_ctx::field_replaced.
struct TrainState {
  DevBuf p, m, v, g, wpart, loss, out, dfeat, feat, flag, target;
  mtx_field_opt opt{};
  bool on = false;
  uint32_t adam_t = 0, good_steps = 0;
  float scale = 1.f;
};

// Neural radiosity: surface tables (mtx_nerad_upload) of the scene's shapes
// and triangles at their current positions, and the batch buffers. The tables
// go with a new scene and with moved vertices: mtx_ctx::scene_dropped,
// geometry_moved.
struct NeradState {
  DevBuf shape_pmf, shape_cdf, tri_off, tri_pmf, tri_cdf, tri_prim, dists;
  mtx::NeradTables tables{};
  bool live = false;
  DevBuf lhs, qp, qd, Lrhs, lanes;
};

// ReSTIR GI frame state (restirgi.py:217-226): kept across mtx_render calls.
// Sized by ensure_restir (render.cpp) for a frame's lane count; another count
// invalidates it, frame 0 restarts it. A new scene or moved vertices keep it:
// the reference has no reprojection under moving geometry either; a caller
// restarts with frame = 0 or accepts stale reuse.
struct RestirState {
  DevBuf samp[2], tres, sres, radius, hit, dir, emit, rng, rays, count, occ, qM, nbr, xs, ns;
  DevBuf heads;  // per-XCD claim cursors of k_trace_test
  uint32_t n = 0, cur = 0, pending_frame = 0;
  bool valid = false, pending_b = false;
  mtx_camera prev_cam{};
};

// PSSMLT chain state. Sized by ensure_mlt (render.cpp) for wave 0's capacity
// and the render's depth; every render starts its chains anew (k_mlt_init).
struct MltState {
  DevBuf cur, L, prop, vpath, vprop;
  DevBuf vpath_es, vprop_es;  // pssmltpath emitter samples
  uint32_t capacity = 0, depth = 0, es_capacity = 0, es_depth = 0;
};

// Scratch of the host-pointer entry points (sample_rays, trace, the
// primitives, film put): each call sizes what it uses and leaves nothing
// another call relies on.
struct Scratch {
  DevBuf s0, s1, s2, s3, s4, s5, s6;
};

}  // namespace mtxh

struct mtx_ctx {
  int device = 0;
  int n_cu = 256;
  hipStream_t stream = nullptr;  // wave[0].stream is the same handle
  mtxh::Wave wave[2];
  uint32_t *q_pinned = nullptr;  // per-chunk cache-query counts of a stats render (pinned, kQSlots)
  mtxh::Knobs knobs;
  mtxh::SceneState scene;
  mtxh::RefitState refit;
  mtxh::FieldState field;
  mtxh::TrainState train;
  mtxh::NeradState nerad;
  mtxh::RestirState restir;
  mtxh::MltState mlt;
  mtxh::Scratch scratch;
  // shared by both wavefronts
  mtxh::DevBuf stats;
  // film
  mtxh::DevBuf contrib, film;
  int trace_grid = 0, closest_grid = 0, shade_grid = 0;  // persistent grids: any hit, closest hit, shade
  int mega_grid = 0;
  size_t max_lds = 160 * 1024;  // LDS one workgroup may hold (gfx950: the CU's 160 KiB)
  mtxh::DevBuf cq_ws;  // sort workspace of the Morton order
  std::vector<hipEvent_t> events;
  hipEvent_t prim_ev[2] = {nullptr, nullptr};
  double last_device_ms = 0.0;

  // What an event invalidates, each in one place.
  // The scene's buffers are about to be rewritten (mtx_scene_upload's device
  // phase) or were left half refit: no scene until an upload completes. Drops
  // the kernels' view with its pointers, and the nerad surface tables, which
  // belong to the previous scene.
  void scene_dropped() {
    scene.live = false;
    scene.dev = {};
    nerad.live = false;
  }
  // Vertices moved (mtx_scene_update_vertices): the nerad surface tables
  // belong to the previous geometry. The ReSTIR reservoirs are kept
  // (RestirState).
  void geometry_moved() { nerad.live = false; }
  // A new field (mtx_field_upload): mtx_field_train_init starts over.
  void field_replaced() { train.on = false; }
};

namespace mtxh {

// Device-pointer entry points (the *_dev functions of mtx.h): every buffer
// must be memory of the context's device (hipMalloc'd, e.g. a torch CUDA
// tensor's data_ptr); host memory is refused with MTX_E_ARG.
bool on_device(const mtx_ctx *c, const void *p);
int need_device(const mtx_ctx *c, const char *fn, std::initializer_list<const void *> ptrs);

// A scratch slot of `bytes` for a host entry point, filled from `src` if given.
int stage(mtx_ctx *c, DevBuf &slot, size_t bytes, const void *src = nullptr);
// Copies results back to the host arrays; returns once they have landed.
struct Unstage {
  void *dst;
  const DevBuf &slot;
  size_t bytes;
};
int unstage(mtx_ctx *c, std::initializer_list<Unstage> outs);

// Runs the device work of one primitive call: `launch` enqueues the
// primitive's kernels on the context's stream and returns an MTX code. The
// event pair encloses those kernels only -- callers stage, range-check and
// copy back outside it -- and their time is what mtx_last_device_ms reports.
// The stream is idle on return.
template <class Launch>
int prim_run(mtx_ctx *c, Launch launch) {
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

// per NRC cache / field query: each of the three query planes (p, d, T),
// the fp16 feature row, the RGB output
constexpr size_t kQueryBytes = 16, kFeatBytes = 128, kOutBytes = 12;

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

// render.cpp: what the nerad RHS (field_entry.cpp) shares with mtx_render
int ensure_wave(mtx_ctx *c, Wave &w, uint32_t cap, uint32_t max_depth);
int ensure_cache(mtx_ctx *c, Wave &w, uint32_t cap);
mtxd::WaveBuffers views(mtx_ctx *c, const Wave &w);
hipError_t reset_counters(const mtxd::WaveBuffers &b, uint32_t depth, hipStream_t st);
void run_bounces(mtx_ctx *c, const Wave &w, const mtxd::WaveBuffers &b, const mtxd::ChunkParams &p, Timer &tm,
                 uint64_t *n_trace, uint64_t *n_shadow);

}  // namespace mtxh
