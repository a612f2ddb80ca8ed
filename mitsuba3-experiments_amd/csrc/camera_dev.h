// camera_dev.h — the camera sample of a chunk and a path's initial state:
// what raygen stores (shade.hip k_raygen_camera) and what a cam0 chunk derives
// instead where it is used (trace.hip CameraSrc, the bounce-0 shades of
// shade_dev.h, the film source kernels of film.hip).
#pragma once
#include "device_common.h"

namespace mtxd {

// A path's initial depth | flags << 16 word (misc.w).
__device__ __forceinline__ uint32_t init_word(const ChunkParams &p, bool env) {
  uint32_t depth = 0, flags = 0;
  if (p.integrator == MTX_INT_PATH_MIS) {
    depth = 0;
    // prev_bsdf_delta = True (path-mis.py:46); valid_ray = scene.environment() is not None (:41)
    flags = PF_PREV_DELTA | (env ? PF_VALID_RAY : 0u);
  } else if (p.integrator == MTX_INT_SIMPLE) {
    depth = 0;  // simple.py:27
  } else {
    depth = 1;  // path.py:230, nrc.py:39
  }
  return depth | (flags << 16);
}

// The camera sample of a chunk: everything k_raygen_camera stores for a path
// is a function of the path's index, ChunkParams and the camera. The stored
// form (k_raygen_camera) and the derived form (ChunkParams::cam0: CameraSrc,
// the bounce-0 shades, the film source kernels) both come from these two
// helpers, so they cannot drift.
// Film position of sample `smp` of film pixel pix = (x, y); returns the
// sampler after the two jitter draws (path.py:45).
__device__ __forceinline__ Pcg32 camera_film_pos(const ChunkParams &p, uint32_t pix, uint32_t x, uint32_t y,
                                                 uint32_t smp, float2 &pos) {
  const uint32_t lane = pix * p.spp_total + p.sample_offset + smp;
  Pcg32 rng = sampler_lane(p.seed, lane);
  const V2 u = rng.next_2d();  // film jitter (path.py:45)
  pos = make_float2((float)x + u.x, (float)y + u.y);
  return rng;
}
struct CamPath {
  Ray ray;
  float2 pos;     // film position (sx, sy)
  Pcg32 rng;      // after the jitter draws
  uint32_t word;  // depth | flags << 16
};
// Path i of the chunk (pixel-major: the samples of one pixel share a wave,
// coherent traversal).
__device__ __forceinline__ CamPath camera_path(const mtx_camera &cam, bool env, const ChunkParams &p, uint32_t i) {
  const uint32_t px_local = i / p.spp, smp = i - px_local * p.spp;
  const uint32_t pix = p.px0 + px_local;
  const uint32_t y = pix / p.width, x = pix - y * p.width;
  CamPath cp;
  cp.rng = camera_film_pos(p, pix, x, y, smp, cp.pos);
  const V2 adj = V2{cp.pos.x / (float)p.width, cp.pos.y / (float)p.height};
  cp.ray = camera_ray(cam, adj);  // path.py:60-62
  cp.word = init_word(p, env);
  return cp;
}

// The records init_path would have stored for camera path i (ray_o, ray_d,
// misc), for the bounce-0 shade of a cam0 chunk (k_shade_cam).
struct CamState {
  float4 ro, rd;
  uint4 mi;
};
__device__ __forceinline__ CamState cam_state(const DevScene &s, const ChunkParams &p, uint32_t i) {
  const CamPath cp = camera_path(s.camera, s.has_env != 0, p, i);
  CamState c;
  c.ro = make_float4(cp.ray.o.x, cp.ray.o.y, cp.ray.o.z, cp.ray.maxt);
  c.rd = make_float4(cp.ray.d.x, cp.ray.d.y, cp.ray.d.z, 0.f);
  c.mi = make_uint4((uint32_t)cp.rng.state, (uint32_t)(cp.rng.state >> 32), cp.rng.seq, cp.word);
  return c;
}

__device__ __forceinline__ void init_path(const WaveBuffers &b, const ChunkParams &p, uint32_t i, const Ray &ray,
                                          const Pcg32 &rng, float2 pos, bool env) {
  const uint32_t word = init_word(p, env);
  // throughput = 1, eta = 1, L = 0, prev_bsdf_pdf = 1 (path-mis.py:45), prev_p = 0 are
  // not stored: the bounce-0 shade uses these constants (kInitThr / kInitL / kInitPrev)
  st_stream<kNtRaygen>(b.ray_o[0] + i, make_float4(ray.o.x, ray.o.y, ray.o.z, ray.maxt));  // queue position i (identity)
  st_stream<kNtRaygen>(b.ray_d[0] + i, make_float4(ray.d.x, ray.d.y, ray.d.z, 0.f));
  st_stream<kNtRaygen>(b.misc[0] + i,
                       make_uint4((uint32_t)rng.state, (uint32_t)(rng.state >> 32), rng.seq, word));
  b.pos[i] = pos;
  if (!p.ident0) b.queue[0][i] = i;
}

// Initial path state (init_path, k_rs_begin): throughput 1 / eta 1, L 0 /
// prev_bsdf_pdf 1, prev_p 0 / spread 0. Never stored: bounce-0 shades use it.
// (register constants: a select between a __device__ constant and the state
// plane compiled to a pointer select + flat load per plane)
#define kInitThr make_float4(1.f, 1.f, 1.f, 1.f)
#define kInitL make_float4(0.f, 0.f, 0.f, 1.f)
#define kInitPrev make_float4(0.f, 0.f, 0.f, 0.f)

}  // namespace mtxd
