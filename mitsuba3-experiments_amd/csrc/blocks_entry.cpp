// blocks_entry.cpp — the building blocks (blocks.hip) behind mtx.blocks: the
// device-pointer entries, the film put / gather and the host twins.
#include <string.h>

#include <initializer_list>

#include "runtime.h"
#include "blocks.h"
#include "photon.h"
#include "mtx_core/bdpt.h"
#include "mtx_core/film.h"
#include "mtx_core/interaction.h"
#include "prims.h"
#include "scene_check.h"

using namespace mtxh;

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
  if (scene && !c->scene.live) {
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
  if (int rc = dalloc(c->scratch.s6, 64)) return rc;
  HIP_TRY(hipMemsetAsync(c->scratch.s6.p, 0, 4, c->stream));
  return MTX_OK;
}
static int blk_end(mtx_ctx *c, const char *fn, const char *what) {
  HIP_TRY(hipGetLastError());
  uint32_t bad = 0;
  if (what) HIP_TRY(hipMemcpyAsync(&bad, c->scratch.s6.p, 4, hipMemcpyDeviceToHost, c->stream));
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
  mtxd::launch_blk_interact(c->scene.dev, (uint32_t)n, 1, o, d, maxt, nullptr, nullptr, nullptr, nullptr, active, *si,
                            nullptr, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_ray_test_dev(mtx_ctx *c, uint64_t n, const float *o, const float *d, const float *maxt,
                            const uint8_t *active, uint8_t *out) {
  const char *fn = "mtx_blocks_ray_test_dev";
  int rc = blk_begin(c, fn, n, true, {o, d, maxt, out});
  if (rc || n == 0) return rc;
  if ((rc = need_device(c, fn, {o, d, maxt, active, out}))) return rc;
  mtxd::launch_blk_ray_test(c->scene.dev, (uint32_t)n, o, d, maxt, active, out, c->stream);
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
  mtxd::launch_blk_interact(c->scene.dev, (uint32_t)n, 0, nullptr, d, nullptr, t, prim, u, v, active, *si,
                            (uint32_t *)c->scratch.s6.p, c->stream);
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
  mtxd::launch_blk_sample_emitter(c->scene.dev, (uint32_t)n, p, nrm, u, active, test_visibility != 0, *ds, weight,
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
  mtxd::launch_blk_emitter(c->scene.dev, (uint32_t)n, emitter, d, dist, nrm, wi, active, pdf, le, (uint32_t *)c->scratch.s6.p,
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
  mtxd::launch_blk_bsdf(c->scene.dev, c->scene.n_materials, (uint32_t)n, material, uv, wi, wo, u1, u2, active, o, flags,
                        (uint32_t *)c->scratch.s6.p, c->stream);
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
  mtxd::launch_blk_sensor_ray(c->scene.dev.camera, (uint32_t)n, pos, active, o, d, maxt, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_sample_emitter_ray_dev(mtx_ctx *c, uint64_t n, const float *u_pos, const float *u_dir,
                                      const uint8_t *active, float *o, float *d, float *maxt, float *weight, float *p,
                                      float *nrm, int32_t *emitter) {
  const char *fn = "mtx_blocks_sample_emitter_ray_dev";
  int rc = blk_begin(c, fn, n, true, {u_pos, u_dir, o, d, maxt, weight, p, nrm, emitter});
  if (rc || n == 0) return rc;
  if ((rc = need_device(c, fn, {u_pos, u_dir, active, o, d, maxt, weight, p, nrm, emitter}))) return rc;
  mtxd::launch_blk_sample_emitter_ray(c->scene.dev, (uint32_t)n, u_pos, u_dir, active,
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
  mtxd::launch_blk_sensor_direction(c->scene.dev, (uint32_t)n, p, nrm, active, test_visibility != 0,
                                    mtxd::SensorDirPlanes{pos, d, dist, weight, valid}, c->stream);
  return blk_end(c, fn, nullptr);
}

int mtx_blocks_photon_gather_dev(mtx_ctx *c, const mtx_hashgrid_view *grid, const mtx_photon_planes *ph,
                                 const mtx_visible_planes *vp, uint64_t m, const float *radius,
                                 uint32_t radius_stride, uint32_t max_depth, float *out_sum, uint32_t *out_count) {
  const char *fn = "mtx_blocks_photon_gather_dev";
  int rc = blk_begin(c, fn, m, true, {grid, ph, vp, radius, out_sum, out_count});
  if (rc || m == 0) return rc;
  if (!ph->d || !ph->beta || !ph->depth || !vp->p || !vp->material || !vp->uv || !vp->wi || !vp->sh_n || !vp->n ||
      !vp->depth || radius_stride > 1) {
    mtx_set_error("%s: null plane or radius_stride > 1", fn);
    return MTX_E_ARG;
  }
  mtxd::HgView g;
  if ((rc = hashgrid_view_check(c, fn, grid, m, &g)) ||
      (rc = need_device(c, fn, {ph->d, ph->beta, ph->depth, vp->p, vp->material, vp->uv, vp->wi, vp->sh_n, vp->n,
                                vp->depth, radius, out_sum, out_count})) ||
      (rc = dalloc(c->scratch.s6, 64)))
    return rc;
  HIP_TRY(hipMemsetAsync(c->scratch.s6.p, 0, 8, c->stream));
  mtxd::launch_photon_gather(c->scene.dev, c->scene.n_materials, g, *ph, *vp, (uint32_t)m, radius, radius_stride,
                             max_depth, out_sum, out_count, (uint32_t *)c->scratch.s6.p, c->stream);
  HIP_TRY(hipGetLastError());
  uint32_t bad[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(bad, c->scratch.s6.p, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (bad[0]) return hashgrid_cap_error(fn, bad[0]);
  if (bad[1]) {
    mtx_set_error("%s: %u lanes with a material index past the scene's materials (handled as invalid)", fn, bad[1]);
    return MTX_E_ARG;
  }
  return MTX_OK;
}

// The host twin of the emitter-ray and sensor-direction kernels: the same per-lane functions over a
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
  mtxd::launch_blk_bdpt_connect(c->scene.dev, c->scene.n_materials, (uint32_t)n, *cam, *lit, s, t, max_depth, flags,
                                active, L, weight, (uint32_t *)c->scratch.s6.p, c->stream);
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
  if ((rc = need_device(c, fn, {planes, pos, L, active})) || (rc = dalloc(c->scratch.s0, 64))) return rc;
  uint32_t *counts = (uint32_t *)c->scratch.s0.p;
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
    if ((rc = dalloc(c->scratch.s1, 4 * n)) || (rc = dalloc(c->scratch.s2, 4ull * n_keys)) || (rc = dalloc(c->scratch.s3, 4ull * n_keys)) ||
        (rc = dalloc(c->scratch.s4, 4 * n)) || (rc = dalloc(c->scratch.s5, mtxd::hashgrid_workspace_bytes(n, n_keys))))
      return rc;
    uint32_t *keys = (uint32_t *)c->scratch.s1.p, *ksize = (uint32_t *)c->scratch.s2.p, *koff = (uint32_t *)c->scratch.s3.p;
    uint32_t *order = (uint32_t *)c->scratch.s4.p;
    mtxd::launch_blk_film_keys(g, (uint32_t)n, pos, active, keys, counts, c->stream);
    HIP_TRY(hipGetLastError());
    if ((rc = mtxd::group_by_u32(keys, n, n_keys, ksize, koff, order, c->scratch.s5.p, c->stream))) return rc;
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
