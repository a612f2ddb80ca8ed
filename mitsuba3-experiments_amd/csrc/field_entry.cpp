// field_entry.cpp — the radiance field (field.hip), its training
// (field_train.hip) and neural radiosity (nerad.hip).
#include <algorithm>
#include <cmath>
#include <vector>

#include "runtime.h"
#include "prims.h"

using namespace mtxh;

extern "C" {

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
  if ((rc = upload(c->field.table, f->table, table_halfs, c->stream))) return rc;
  const uint32_t n_frag = mtxd::field_frag_count(f->n_hidden);
  std::vector<uint16_t> frag((size_t)n_frag * 64 * 8);
  mtxd::field_prepack(f->weights, f->n_in, f->n_hidden, frag.data());
  if ((rc = upload(c->field.frag, frag.data(), frag.size(), c->stream))) return rc;
  const uint32_t n_w = 64u * f->n_in + f->n_hidden * 4096u + 3u * 64u;
  if ((rc = upload(c->field.w16, f->weights, n_w, c->stream))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->field.n_in = f->n_in;
  c->field.n_w = n_w;
  c->field.n_table = table_halfs;
  c->field_replaced();
  mtx::FieldEncoding &e = c->field.enc;
  e.table = (const uint16_t *)c->field.table.p;
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
  c->field.hidden = f->n_hidden;
  c->field.live = true;
  return MTX_OK;
}

static int field_stage_queries(mtx_ctx *c, uint64_t n, const float *p, const float *wi) {
  int rc;
  if ((rc = dalloc(c->field.fq_p, 16 * n))) return rc;
  if ((rc = dalloc(c->field.fq_d, 16 * n))) return rc;
  std::vector<float> tp(4 * n), td(4 * n);
  for (uint64_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      tp[4 * i + k] = p[3 * i + k];
      td[4 * i + k] = wi[3 * i + k];
    }
  HIP_TRY(hipMemcpy(c->field.fq_p.p, tp.data(), 16 * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->field.fq_d.p, td.data(), 16 * n, hipMemcpyHostToDevice));
  return MTX_OK;
}

static int field_check(mtx_ctx *c, uint64_t n) {
  if (!c || !c->field.live) {
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
  return mtxd::field_encode(c->field.enc, (const float4 *)c->field.fq_p.p, (const float4 *)c->field.fq_d.p, nullptr, (uint32_t)n,
                            (uint16_t *)c->wave[0].f_feat.p, c->stream);
}
static int field_mlp_staged(mtx_ctx *c, uint64_t n) {
  return mtxd::field_mlp((const uint16_t *)c->wave[0].f_feat.p, nullptr, (uint32_t)n, c->field.frag.p,
                         c->field.hidden, (float *)c->wave[0].f_out.p, c->n_cu, c->stream);
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

}  // extern "C"

// ============================================================================
// Radiance-field training and neural radiosity samples (nerad.py:121-375)
// ============================================================================
static int train_check(mtx_ctx *c) {
  if (!c || !c->field.live) {
    mtx_set_error("no radiance field uploaded (mtx_field_upload)");
    return MTX_E_ARG;
  }
  if (!c->train.on) {
    mtx_set_error("field training not initialised (mtx_field_train_init)");
    return MTX_E_ARG;
  }
  return MTX_OK;
}

// k_field_train keeps every layer's activation tile in LDS: a field whose
// tiles exceed what one workgroup may hold (n_hidden >= 14 on gfx950's
// 160 KiB) cannot be trained. Refused here, on the host, before any launch.
static int train_fits(mtx_ctx *c) {
  const size_t lds = mtxd::field_train_lds(c->field.hidden);
  if (lds > c->max_lds) {
    mtx_set_error("field training: n_hidden %u needs %zu B of LDS per workgroup, the device allows %zu B "
                  "(inference of this field still works)",
                  c->field.hidden, lds, c->max_lds);
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
  const uint32_t LF = c->field.enc.n_levels * c->field.enc.n_features;
  const uint32_t blocks = (n + 63) / 64;
  const uint64_t n_params = c->field.n_table + c->field.n_w;
  if ((rc = train_fits(c))) return rc;
  if ((rc = dalloc(c->train.feat, 128ull * n))) return rc;
  if ((rc = dalloc(c->train.out, 12ull * n))) return rc;
  if ((rc = dalloc(c->train.loss, 4ull * blocks))) return rc;
  if ((rc = dalloc(c->train.wpart, 4ull * blocks * c->field.n_w))) return rc;
  if ((rc = dalloc(c->train.dfeat, 4ull * n * LF))) return rc;
  if ((rc = dalloc(c->train.g, 4 * n_params))) return rc;
  if ((rc = mtxd::field_encode(c->field.enc, qp, qd, nullptr, n, (uint16_t *)c->train.feat.p, c->stream))) return rc;
  HIP_TRY(hipMemsetAsync(c->train.g.p, 0, 4 * c->field.n_table, c->stream));
  float *g = (float *)c->train.g.p;
  rc = mtxd::field_train_launch((const uint16_t *)c->train.feat.p, n, (const uint16_t *)c->field.w16.p,
                                c->field.n_in, c->field.hidden, target, (float)(2.0 * scale / (3.0 * n)),
                                (float *)c->train.out.p, (float *)c->train.loss.p, (float *)c->train.wpart.p,
                                g + c->field.n_table, (float *)c->train.dfeat.p, LF, c->stream);
  if (rc) return rc;
  mtxd::field_encode_bwd_launch(c->field.enc, qp, n, (const float *)c->train.dfeat.p, g, c->stream);
  HIP_TRY(hipGetLastError());
  if (loss) {
    std::vector<float> part(blocks);
    HIP_TRY(hipMemcpyAsync(part.data(), c->train.loss.p, 4ull * blocks, hipMemcpyDeviceToHost, c->stream));
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
  const uint64_t n_params = c->field.n_table + c->field.n_w;
  int rc;
  if ((rc = dalloc(c->train.flag, 16))) return rc;
  HIP_TRY(hipMemsetAsync(c->train.flag.p, 0, 4, c->stream));
  mtxd::grad_check_launch((const float *)c->train.g.p, n_params, (uint32_t *)c->train.flag.p, c->stream);
  uint32_t found = 0;
  HIP_TRY(hipMemcpyAsync(&found, c->train.flag.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const mtx_field_opt &o = c->train.opt;
  if (!found) {
    ++c->train.adam_t;
    const double t = c->train.adam_t;
    const float lr_t = (float)(o.lr * std::sqrt(1.0 - std::pow((double)o.beta_2, t)) /
                               (1.0 - std::pow((double)o.beta_1, t)));
    mtxd::adam_launch((float *)c->train.p.p, (float *)c->train.m.p, (float *)c->train.v.p, (const float *)c->train.g.p, n_params,
                      lr_t, o.beta_1, o.beta_2, o.epsilon, 1.f / c->train.scale, (const uint32_t *)c->train.flag.p,
                      (uint16_t *)c->field.table.p, c->field.n_table, (uint16_t *)c->field.w16.p, c->stream);
    mtxd::field_prepack_launch((const uint16_t *)c->field.w16.p, c->field.n_in, c->field.hidden,
                               (uint16_t *)c->field.frag.p, c->stream);
    HIP_TRY(hipGetLastError());
    if (++c->train.good_steps >= o.growth_interval) {
      c->train.scale *= o.growth_factor;
      c->train.good_steps = 0;
    }
  } else {
    c->train.scale *= o.backoff_factor;
    c->train.good_steps = 0;
  }
  if (st) {
    st->found_inf = found;
    st->scale = c->train.scale;
    st->step = c->train.adam_t;
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
  if (!c->scene.live || !c->nerad.live) {
    mtx_set_error("nerad: upload a scene and its surface tables (mtx_nerad_upload) first");
    return MTX_E_NOSCENE;
  }
  if (need_field && !c->field.live) {
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
  if ((rc = dalloc(c->nerad.lhs, 48ull * a->batch))) return rc;
  if ((rc = dalloc(c->nerad.qp, 16ull * a->batch))) return rc;
  if ((rc = dalloc(c->nerad.qd, 16ull * a->batch))) return rc;
  mtxd::launch_nerad_lhs(c->scene.dev, c->nerad.tables, a->lhs_seed, a->batch, (float4 *)c->nerad.lhs.p, (float4 *)c->nerad.qp.p,
                         (float4 *)c->nerad.qd.p, c->stream);
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
  if ((rc = dalloc(c->nerad.Lrhs, 12ull * a->batch))) return rc;
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
  mtxd::launch_nerad_raygen(b, p, (const float4 *)c->nerad.lhs.p, a->M, c->stream);
  Timer tm{c, st != nullptr};
  uint64_t nt = 0, ns = 0;
  run_bounces(c, w, b, p, tm, &nt, &ns);
  if ((rc = mtxd::field_encode(c->field.enc, b.cq_p, b.cq_d, b.cq_count, n, (uint16_t *)w.f_feat.p, c->stream))) return rc;
  if ((rc = mtxd::field_mlp((const uint16_t *)w.f_feat.p, b.cq_count, n, c->field.frag.p, c->field.hidden,
                            (float *)w.f_out.p, c->n_cu, c->stream)))
    return rc;
  mtxd::launch_nerad_apply(b, (const float *)w.f_out.p, n, 0, c->stream);
  mtxd::launch_nerad_mean(b, a->batch, a->M, (float *)c->nerad.Lrhs.p, lanes_dev, c->stream);
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
  if (!c || !opt || !c->field.live) {
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
  const uint64_t n_params = c->field.n_table + c->field.n_w;
  if ((rc = dalloc(c->train.p, 4 * n_params))) return rc;
  if ((rc = dalloc(c->train.m, 4 * n_params))) return rc;
  if ((rc = dalloc(c->train.v, 4 * n_params))) return rc;
  mtxd::half_to_float_launch((const uint16_t *)c->field.table.p, c->field.n_table, (float *)c->train.p.p, c->stream);
  mtxd::half_to_float_launch((const uint16_t *)c->field.w16.p, c->field.n_w, (float *)c->train.p.p + c->field.n_table,
                             c->stream);
  HIP_TRY(hipMemsetAsync(c->train.m.p, 0, 4 * n_params, c->stream));
  HIP_TRY(hipMemsetAsync(c->train.v.p, 0, 4 * n_params, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->train.opt = *opt;
  c->train.adam_t = 0;
  c->train.good_steps = 0;
  c->train.scale = opt->init_scale;
  c->train.on = true;
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
  if ((rc = upload(c->train.target, target, 3 * n, c->stream))) return rc;
  if ((rc = field_backward(c, (const float4 *)c->field.fq_p.p, (const float4 *)c->field.fq_d.p, (const float *)c->train.target.p,
                           (uint32_t)n, scale, loss)))
    return rc;
  const float *g = (const float *)c->train.g.p;
  if (out) HIP_TRY(hipMemcpyAsync(out, c->train.out.p, 12 * n, hipMemcpyDeviceToHost, c->stream));
  if (grad_table) HIP_TRY(hipMemcpyAsync(grad_table, g, 4 * c->field.n_table, hipMemcpyDeviceToHost, c->stream));
  if (grad_weights)
    HIP_TRY(hipMemcpyAsync(grad_weights, g + c->field.n_table, 4ull * c->field.n_w, hipMemcpyDeviceToHost, c->stream));
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
  if ((rc = upload(c->train.target, target, 3 * n, c->stream))) return rc;
  double loss = 0.0;
  if ((rc = field_backward(c, (const float4 *)c->field.fq_p.p, (const float4 *)c->field.fq_d.p, (const float *)c->train.target.p,
                           (uint32_t)n, c->train.scale, &loss)))
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
  const uint64_t nt = c->field.n_table, nw = c->field.n_w;
  if (table) HIP_TRY(hipMemcpy(table, c->train.p.p, 4 * nt, hipMemcpyDeviceToHost));
  if (weights) HIP_TRY(hipMemcpy(weights, (const float *)c->train.p.p + nt, 4 * nw, hipMemcpyDeviceToHost));
  if (m) HIP_TRY(hipMemcpy(m, c->train.m.p, 4 * (nt + nw), hipMemcpyDeviceToHost));
  if (v) HIP_TRY(hipMemcpy(v, c->train.v.p, 4 * (nt + nw), hipMemcpyDeviceToHost));
  return MTX_OK;
}

int mtx_nerad_upload(mtx_ctx *c, const mtx_nerad_tables *t) {
  if (!c || !t || !c->scene.live) {
    mtx_set_error("mtx_nerad_upload: null argument or no scene");
    return MTX_E_ARG;
  }
  const uint32_t S = t->n_shapes, E = t->n_entries;
  if (S != c->scene.n_shapes || !t->shape_pmf || !t->shape_cdf || !t->tri_off || !t->tri_pmf || !t->tri_cdf ||
      !t->tri_prim || !t->tri_sum || !t->tri_norm || !t->tri_valid || t->tri_off[S] != E ||
      t->shape_valid[0] > t->shape_valid[1] || t->shape_valid[1] >= S) {
    mtx_set_error("mtx_nerad_upload: tables do not match the scene (%u shapes)", c->scene.n_shapes);
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
    if (t->tri_prim[i] >= c->scene.dev.n_tris) {
      mtx_set_error("mtx_nerad_upload: tri_prim[%u] out of range", i);
      return MTX_E_ARG;
    }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if ((rc = upload(c->nerad.shape_pmf, t->shape_pmf, S, c->stream))) return rc;
  if ((rc = upload(c->nerad.shape_cdf, t->shape_cdf, S, c->stream))) return rc;
  if ((rc = upload(c->nerad.tri_off, t->tri_off, S + 1, c->stream))) return rc;
  if ((rc = upload(c->nerad.tri_pmf, t->tri_pmf, E, c->stream))) return rc;
  if ((rc = upload(c->nerad.tri_cdf, t->tri_cdf, E, c->stream))) return rc;
  if ((rc = upload(c->nerad.tri_prim, t->tri_prim, E, c->stream))) return rc;
  std::vector<mtx::DiscreteDist> d(S);
  for (uint32_t k = 0; k < S; ++k) {
    const uint32_t off = t->tri_off[k];
    d[k].pmf = (const float *)c->nerad.tri_pmf.p + off;
    d[k].cdf = (const float *)c->nerad.tri_cdf.p + off;
    d[k].n = t->tri_off[k + 1] - off;
    d[k].valid_lo = t->tri_valid[2 * k];
    d[k].valid_hi = t->tri_valid[2 * k + 1];
    d[k].sum = t->tri_sum[k];
    d[k].normalization = t->tri_norm[k];
  }
  if ((rc = upload(c->nerad.dists, d.data(), S, c->stream))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  mtx::NeradTables &n = c->nerad.tables;
  n.shape.pmf = (const float *)c->nerad.shape_pmf.p;
  n.shape.cdf = (const float *)c->nerad.shape_cdf.p;
  n.shape.n = S;
  n.shape.valid_lo = t->shape_valid[0];
  n.shape.valid_hi = t->shape_valid[1];
  n.shape.sum = t->shape_sum;
  n.shape.normalization = t->shape_norm;
  n.tri_dist = (const mtx::DiscreteDist *)c->nerad.dists.p;
  n.tri_off = (const uint32_t *)c->nerad.tri_off.p;
  n.tri_prim = (const uint32_t *)c->nerad.tri_prim.p;
  c->nerad.live = true;
  return MTX_OK;
}

int mtx_nerad_lhs(mtx_ctx *c, const mtx_nerad_args *a, float *out) {
  int rc = nerad_check(c, a, false);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = nerad_lhs_dev(c, a))) return rc;
  if (out) {
    std::vector<float> raw(12ull * a->batch);
    HIP_TRY(hipMemcpyAsync(raw.data(), c->nerad.lhs.p, 48ull * a->batch, hipMemcpyDeviceToHost, c->stream));
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
    if ((rc = dalloc(c->nerad.lanes, 12ull * a->batch * a->M))) return rc;
    lanes_dev = (float *)c->nerad.lanes.p;
  }
  if ((rc = nerad_rhs_dev(c, a, lanes_dev, nullptr))) return rc;
  if (L_rhs) HIP_TRY(hipMemcpyAsync(L_rhs, c->nerad.Lrhs.p, 12ull * a->batch, hipMemcpyDeviceToHost, c->stream));
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
  if ((rc = field_backward(c, (const float4 *)c->nerad.qp.p, (const float4 *)c->nerad.qd.p, (const float *)c->nerad.Lrhs.p,
                           a->batch, c->train.scale, &loss)))
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
