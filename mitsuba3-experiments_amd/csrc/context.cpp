// context.cpp — the device context: creation with its environment knobs,
// destruction, and the buffer, pointer and staging helpers every host file
// uses (runtime.h).
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "runtime.h"

namespace mtxh {

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

bool on_device(const mtx_ctx *c, const void *p) {
  if (!p) return false;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // clear the sticky "invalid value" of an unregistered host pointer
    return false;
  }
  return (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) && at.device == c->device;
}
int need_device(const mtx_ctx *c, const char *fn, std::initializer_list<const void *> ptrs) {
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

int stage(mtx_ctx *c, DevBuf &slot, size_t bytes, const void *src) {
  if (int rc = dalloc(slot, bytes)) return rc;
  if (src) HIP_TRY(hipMemcpyAsync(slot.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  return MTX_OK;
}
int unstage(mtx_ctx *c, std::initializer_list<Unstage> outs) {
  for (const Unstage &o : outs) HIP_TRY(hipMemcpyAsync(o.dst, o.slot.p, o.bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MTX_OK;
}

}  // namespace mtxh

using namespace mtxh;

// MTX_SHADE_CLASSES: "0" or "1". False (and the error set) for anything else.
static bool shade_classes_knob(const char *e, uint32_t *out) {
  if (!e || !(e[0] == '0' || e[0] == '1') || e[1]) {
    mtx_set_error("MTX_SHADE_CLASSES=%s: 0 (the mixed shade loop) or 1 (class queues)", e ? e : "(null)");
    return false;
  }
  *out = (uint32_t)(e[0] - '0');
  return true;
}

// Every environment knob, with its clamp. Read once per context. False (and
// the error set): a value that has no clamp to fall back on.
static bool read_knobs(Knobs &k) {
  if (const char *e = getenv("MTX_LDS_STACK")) k.lds_stack = std::max(1, std::min(MTX_BVH_MAX_DEPTH + 1, atoi(e)));
  if (const char *e = getenv("MTX_LDS_TOP")) k.lds_top = (uint32_t)std::max(0, std::min(256, atoi(e)));
  if (const char *e = getenv("MTX_OCC_LDS_TOP")) k.occ_lds_top = (uint32_t)std::max(0, std::min(192, atoi(e)));
  if (const char *e = getenv("MTX_OCC_LDS_STACK"))
    k.occ_lds_stack = std::max(1, std::min(MTX_BVH_MAX_DEPTH + 1, atoi(e)));
  if (const char *e = getenv("MTX_STREAMS_MAX_LOG2")) k.streams_max_log2 = (uint32_t)std::max(16, std::min(31, atoi(e)));
  if (const char *e = getenv("MTX_STREAMS")) k.streams = (uint32_t)std::max(1, std::min(2, atoi(e)));
  if (const char *e = getenv("MTX_TRACE_BATCH")) k.trace_batch = (uint32_t)std::max(1, std::min(1 << 16, atoi(e)));
  if (const char *e = getenv("MTX_UREFILL")) k.urefill = (uint32_t)std::max(1, std::min(64, atoi(e)));
  if (const char *e = getenv("MTX_CAM_UREFILL")) k.cam_urefill = (uint32_t)std::max(1, std::min(64, atoi(e)));
  if (const char *e = getenv("MTX_OCC_UREFILL")) k.occ_urefill = (uint32_t)std::max(1, std::min(64, atoi(e)));
  if (const char *e = getenv("MTX_TRACE_RING")) {
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || *end || !mtxd::ring_size_ok(v)) {
      mtx_set_error("MTX_TRACE_RING=%s: the ring holds 0 (none), 16 or 32 rays", e);
      return false;
    }
    k.trace_ring = (uint32_t)v;
  }
  if (const char *e = getenv("MTX_SHADE_CLASSES")) {
    if (!shade_classes_knob(e, &k.shade_classes)) return false;
  }
  if (const char *e = getenv("MTX_XCD_CLAIM")) k.xcd_claim = atoi(e) != 0;
  if (const char *e = getenv("MTX_RS_FUSED")) k.rs_fused = atoi(e) ? 1u : 0u;
  if (const char *e = getenv("MTX_MEGA_PATHS")) k.mega_paths = (uint32_t)strtoul(e, nullptr, 0);
  if (const char *e = getenv("MTX_CACHE_FUSED")) k.cache_fused = atoi(e) ? 1u : 0u;
  if (const char *e = getenv("MTX_ENCODE_LM")) k.encode_lm = atoi(e) ? 1u : 0u;
  if (const char *e = getenv("MTX_CACHE_SORT")) k.cache_sort = (uint32_t)std::max(0, std::min(2, atoi(e)));
  return true;
}

extern "C" {

// Diagnostic export (not in mtx.h): the shade kernel's per-phase stamp sums of
// an MTX_DIAG_STAMPS build (tools/shade_stamps.py); returns the segment
// count, or -1 in production builds.
int mtx_diag_shade_stamps(unsigned long long *out) { return mtxd::shade_stamps(out); }

// Diagnostic export (not in mtx.h): the mixed shade loop's class mix of an
// MTX_DIAG_CLASSES build run with MTX_SHADE_CLASSES=0 (tools/shade_class_mix.py):
// 16 bounces x (wave-steps holding 1, 2, 3 classes | entries of class 0, 1, 2);
// returns the words per bounce, or -1 in production builds.
int mtx_diag_shade_class_mix(unsigned long long *out) { return mtxd::shade_class_mix(out); }

// Diagnostic export (not in mtx.h; needs no device): the LDS bytes of a
// k_trace_closest block with rings of `ring` rays, for a tree deeper and
// larger than the knobs ask for: out[0], and out[1] the stack entries it
// keeps in LDS -- mtx_scene_upload's split (scene.cpp) on the knobs' values.
int mtx_diag_trace_lds(uint32_t ring, uint32_t lds_stack, uint32_t lds_top, uint32_t *out) {
  if (!out || !mtxd::ring_size_ok(ring) || !lds_stack) return MTX_E_ARG;
  mtxd::DevScene s{};
  s.lds_entries = lds_stack;
  s.lds_top = lds_top;
  mtxd::split_trace_lds(s, ring);
  out[0] = (uint32_t)mtxd::ring_stack_bytes(s);
  out[1] = s.ring_lds_entries;
  return MTX_OK;
}

// Diagnostic exports (not in mtx.h; need no device). The shading class of a
// material type (mtx_core/shade_class.h):
uint32_t mtx_diag_shade_class_of_type(uint32_t type) { return mtx::shade_class_of_type(type); }
// how a context would read MTX_SHADE_CLASSES=`value` (out[0]: the knob), and
// the dynamic LDS of a class-queue shade block with the ring's entries
// (out[1] bytes, out[2] entries per ring, out[3] classes). MTX_E_ARG for a
// value a context refuses.
int mtx_diag_shade_classes_knob(const char *value, uint32_t *out) {
  if (!out || !shade_classes_knob(value, &out[0])) return MTX_E_ARG;
  out[1] = mtxd::shade_class_lds_bytes();
  out[2] = mtxd::kClassRing;
  out[3] = mtx::kShadeClasses;
  return MTX_OK;
}

// Diagnostic export (not in mtx.h): the context's persistent shade grid and
// its device's CUs (out[0] blocks, out[1] CUs): the grid is the occupancy
// query's blocks per CU (with the class rings' LDS when they are on) x CUs.
int mtx_diag_shade_grid(const mtx_ctx *c, uint32_t *out) {
  if (!c || !out) return MTX_E_ARG;
  out[0] = (uint32_t)c->shade_grid;
  out[1] = (uint32_t)c->n_cu;
  return MTX_OK;
}

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
  {
    // a gfx950 workgroup may hold the CU's whole 160 KiB of LDS (the attribute
    // may report the 64 KiB that needs no opt-in; the kernels launch above it)
    int v = 0;
    c->max_lds = 160 * 1024;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, hip_device) == hipSuccess &&
        (size_t)v > c->max_lds)
      c->max_lds = (size_t)v;
  }
  if (!read_knobs(c->knobs)) {
    mtx_ctx_destroy(c);
    return MTX_E_ARG;
  }
  // the class rings are the shade block's dynamic LDS: the occupancy query counts them
  c->shade_grid = c->n_cu * mtxd::shade_blocks_per_cu(c->knobs.shade_classes != 0);
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

double mtx_last_device_ms(mtx_ctx *c) { return c ? c->last_device_ms : 0.0; }

}  // extern "C"
