// blocks.h — launch wrappers of the device-tensor building blocks
// (blocks.hip): wavefront-wide kernels over the per-lane functions of
// mtx_core, on SoA planes ((C, N) contiguous, plane c of item i at [c * N + i]).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mtx.h"
#include "wavefront.h"

namespace mtxd {

// `n` lanes; pointers are device memory, laid out as mtx.h states for the
// entry of the same name. `bad`: device counter of lanes whose material /
// emitter / prim index lay outside the scene's tables (treated as invalid,
// never dereferenced). `op` of launch_blk_math: MTX_MATH_* (mtx.h).
void launch_blk_seed(uint32_t n, uint32_t seed, const uint32_t *lanes, uint32_t skip, uint64_t *state, hipStream_t st);
void launch_blk_next(uint32_t n, uint64_t *state, int dims, float *out, hipStream_t st);
// trace != 0: closest-hit traversal of (o, d, maxt) first; else the hit
// records (t, prim, u, v) are given.
void launch_blk_interact(const DevScene &s, uint32_t n, int trace, const float *o, const float *d, const float *maxt,
                         const float *t, const uint32_t *prim, const float *u, const float *v, const uint8_t *active,
                         const mtx_si_planes &si, uint32_t *bad, hipStream_t st);
void launch_blk_ray_test(const DevScene &s, uint32_t n, const float *o, const float *d, const float *maxt,
                         const uint8_t *active, uint8_t *out, hipStream_t st);
void launch_blk_spawn(uint32_t n, const float *p, const float *nrm, const float *x, int to, float *o, float *d,
                      float *maxt, hipStream_t st);
void launch_blk_sample_emitter(const DevScene &s, uint32_t n, const float *p, const float *nrm, const float *u,
                               const uint8_t *active, int test_visibility, const mtx_ds_planes &ds, float *weight,
                               hipStream_t st);
void launch_blk_emitter(const DevScene &s, uint32_t n, const int32_t *emitter, const float *d, const float *dist,
                        const float *nrm, const float *wi, const uint8_t *active, float *pdf, float *le,
                        uint32_t *bad, hipStream_t st);
void launch_blk_bsdf(const DevScene &s, uint32_t n_materials, uint32_t n, const int32_t *material, const float *uv,
                     const float *wi, const float *wo, const float *u1, const float *u2, const uint8_t *active,
                     const mtx_bsdf_planes &out, uint32_t *flags, uint32_t *bad, hipStream_t st);
void launch_blk_math(int op, uint32_t n, const float *a, const float *b, const float *c, float *out, hipStream_t st);
// o, d (3, n) and maxt (n, may be null) of camera_ray(cam, pos / size); masked-off lanes: zeros.
void launch_blk_sensor_ray(const mtx_camera &cam, uint32_t n, const float *pos, const uint8_t *active, float *o,
                           float *d, float *maxt, hipStream_t st);
// scene.sample_emitter_ray: the ray o, d (3, n), maxt (n), its weight (3, n),
// the unoffset position and normal p, nrm (3, n) and the emitter index (n).
struct EmitterRayPlanes {
  float *o, *d, *maxt, *weight, *p, *n;
  int32_t *emitter;
};
void launch_blk_sample_emitter_ray(const DevScene &s, uint32_t n, const float *u_pos, const float *u_dir,
                                   const uint8_t *active, const EmitterRayPlanes &out, hipStream_t st);
// sensor.sample_direction of s.camera from p (3, n); nrm (3, n) is read only
// with test_visibility (the connection ray's offset side).
struct SensorDirPlanes {
  float *pos, *d, *dist, *weight;
  uint8_t *valid;
};
void launch_blk_sensor_direction(const DevScene &s, uint32_t n, const float *p, const float *nrm,
                                 const uint8_t *active, int test_visibility, const SensorDirPlanes &out,
                                 hipStream_t st);
// mtx_blocks_bdpt_connect_dev: strategy (ss, tt) or all (-1, -1) of the two
// vertex stores per lane; flags MTX_BDPT_*; weight may be null.
void launch_blk_bdpt_connect(const DevScene &s, uint32_t n_materials, uint32_t n, const mtx_path_planes &camera,
                             const mtx_path_planes &light, int ss, int tt, uint32_t max_depth, uint32_t flags,
                             const uint8_t *active, float *L, float *weight, uint32_t *bad, hipStream_t st);

// Film put (mtx_blocks_film_put_dev): the band [y0, y1) of a film `width`
// wide, its filter, and the contribution planes [slot 8][K][band_px] float4.
struct FilmBand {
  uint32_t width, y0, y1, band_px, rfilter;
};
// Words of the put's device counters.
enum { kPutViolations = 0, kPutDropped = 1, kPutOff = 2, kPutCounters = 3 };
// General path: keys (n) for the group-by with n_keys = band_px + 1 (the last
// is the trash cell); then one lane per source pixel over the groups.
void launch_blk_film_keys(const FilmBand &g, uint32_t n, const float *pos, const uint8_t *active, uint32_t *keys,
                          uint32_t *counts, hipStream_t st);
void launch_blk_film_put(const FilmBand &g, uint32_t n, const float *pos, const float *L, const uint32_t *key_size,
                         const uint32_t *key_offset, const uint32_t *order, uint32_t spp_total,
                         uint32_t sample_offset, float4 *planes, hipStream_t st);
// Pixel-major path: the claim check (counts only), then the staged put;
// `ragged`: the check found lanes that are off or dropped.
void launch_blk_film_claim(const FilmBand &g, uint32_t n, const float *pos, const uint8_t *active, uint32_t s,
                           uint32_t px0, uint32_t *counts, hipStream_t st);
void launch_blk_film_put_staged(const FilmBand &g, uint32_t n, const float *pos, const float *L,
                                const uint8_t *active, uint32_t s, uint32_t px0, uint32_t spp_total,
                                uint32_t sample_offset, int ragged, float4 *planes, hipStream_t st);

}  // namespace mtxd
