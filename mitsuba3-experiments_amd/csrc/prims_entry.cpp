// prims_entry.cpp — the reconstruction-filter queries, the five primitives
// (prims.hip), host and device-pointer entries, and the hash grid's
// fixed-radius query (photon.hip), device pointers only.
#include <algorithm>

#include "runtime.h"
#include "mtx_core/film.h"
#include "photon.h"
#include "prims.h"

using namespace mtxh;

// The fixed-radius query (photon.hip): the grid view's checks, shared with
// the photon gather (blocks_entry.cpp), then count or fill.
int mtxh::hashgrid_view_check(mtx_ctx *c, const char *fn, const mtx_hashgrid_view *g, uint64_t m, mtxd::HgView *out) {
  if (!g || !g->p || !g->cell_size || !g->cell_offset || !g->sample_idx) {
    mtx_set_error("%s: null grid argument", fn);
    return MTX_E_ARG;
  }
  if (g->n == 0 || g->n >= (1ull << 31) || m >= (1ull << 31)) {
    mtx_set_error("%s: the grid's n (%llu) and m (%llu) must be < 2^31, n > 0", fn, (unsigned long long)g->n,
                  (unsigned long long)m);
    return MTX_E_ARG;
  }
  if (g->n_cells == 0 || g->resolution == 0 || g->resolution > (1u << 24)) {
    mtx_set_error("%s: n_cells %u / resolution %u (n_cells > 0, 0 < resolution <= 2^24)", fn, g->n_cells,
                  g->resolution);
    return MTX_E_ARG;
  }
  if (!(g->bbmin <= g->bbmax)) {
    mtx_set_error("%s: bounds [%g, %g]", fn, g->bbmin, g->bbmax);
    return MTX_E_ARG;
  }
  if (int rc = need_device(c, fn, {g->p, g->cell_size, g->cell_offset, g->sample_idx})) return rc;
  *out = mtxd::HgView{g->p, (uint32_t)g->n, g->bbmin, g->bbmax, g->resolution, g->n_cells, g->cell_size,
                      g->cell_offset, g->sample_idx};
  return MTX_OK;
}
int mtxh::hashgrid_cap_error(const char *fn, uint32_t bad) {
  mtx_set_error("%s: %u queries whose cell box holds more than %u cells (not walked); build the grid with "
                "resolution ~ extent / (2 r)", fn, bad, MTX_HG_MAX_QUERY_CELLS);
  return MTX_E_ARG;
}

extern "C" {

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
  if ((rc = dalloc(c->scratch.s6, 64))) return rc;
  HIP_TRY(hipMemsetAsync(c->scratch.s6.p, 0, 4, c->stream));
  if ((rc = mtxd::keys_in_range(v, n, bound, (uint32_t *)c->scratch.s6.p, c->stream))) return rc;
  HIP_TRY(hipMemcpyAsync(bad, c->scratch.s6.p, 4, hipMemcpyDeviceToHost, c->stream));
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
  if ((rc = dalloc(c->scratch.s2, mtxd::scan_workspace_bytes(n)))) return rc;
  if (!dev) {
    if ((rc = stage(c, c->scratch.s0, 4 * n, in)) || (rc = stage(c, c->scratch.s1, 4 * n))) return rc;
    in = (const uint32_t *)c->scratch.s0.p;
  }
  uint32_t *d_out = dev ? out : (uint32_t *)c->scratch.s1.p;
  if ((rc = prim_run(c, [&] { return mtxd::scan_u32(in, d_out, n, inclusive, c->scratch.s2.p, c->stream); }))) return rc;
  return dev ? MTX_OK : unstage(c, {{out, c->scratch.s1, 4 * n}});
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
  if ((rc = dalloc(c->scratch.s1, 4 * n))) return rc;  // ping-pong partner of the output
  if (!dev) {
    if ((rc = stage(c, c->scratch.s0, 4 * n, in)) || (rc = stage(c, c->scratch.s2, 4 * n))) return rc;
    in = (const float *)c->scratch.s0.p;
  }
  float *d_out = dev ? out : (float *)c->scratch.s2.p;
  if ((rc = prim_run(c, [&] { return mtxd::scan_f32_hs_to(in, d_out, (float *)c->scratch.s1.p, n, c->stream); })))
    return rc;
  return dev ? MTX_OK : unstage(c, {{out, c->scratch.s2, 4 * n}});
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
  if ((rc = dalloc(c->scratch.s5, mtxd::hashgrid_workspace_bytes(n, n_cells)))) return rc;
  uint32_t *d_cell = cell, *d_size = cell_size, *d_offset = cell_offset, *d_idx = sample_idx;
  if (!dev) {
    if ((rc = stage(c, c->scratch.s0, 12 * n, p)) || (rc = stage(c, c->scratch.s1, 4 * n)) ||
        (rc = stage(c, c->scratch.s2, 4ull * n_cells)) || (rc = stage(c, c->scratch.s3, 4ull * n_cells)) ||
        (rc = stage(c, c->scratch.s4, 4 * n)))
      return rc;
    p = (const float *)c->scratch.s0.p;
    d_cell = (uint32_t *)c->scratch.s1.p;
    d_size = (uint32_t *)c->scratch.s2.p;
    d_offset = (uint32_t *)c->scratch.s3.p;
    d_idx = (uint32_t *)c->scratch.s4.p;
  }
  if ((rc = prim_run(c, [&] {
         return mtxd::hashgrid_build(p, n, resolution, n_cells, d_cell, d_size, d_offset, d_idx, c->scratch.s5.p, c->stream);
       })))
    return rc;
  return dev ? MTX_OK
             : unstage(c, {{cell, c->scratch.s1, 4 * n},
                           {cell_size, c->scratch.s2, 4ull * n_cells},
                           {cell_offset, c->scratch.s3, 4ull * n_cells},
                           {sample_idx, c->scratch.s4, 4 * n}});
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
  if ((rc = dalloc(c->scratch.s5, mtxd::hashgrid_workspace_bytes(n, n_keys)))) return rc;
  uint32_t *d_size = key_size, *d_offset = key_offset, *d_order = order;
  if (dev) {
    uint32_t bad = 0;
    if ((rc = dev_in_range(c, keys, n, n_keys, &bad))) return rc;
    if (bad) {
      mtx_set_error("%s: a key is >= n_keys (%u)", fn, n_keys);
      return MTX_E_ARG;
    }
  } else {
    if ((rc = stage(c, c->scratch.s1, 4 * n, keys)) || (rc = stage(c, c->scratch.s2, 4ull * n_keys)) ||
        (rc = stage(c, c->scratch.s3, 4ull * n_keys)) || (rc = stage(c, c->scratch.s4, 4 * n)))
      return rc;
    keys = (const uint32_t *)c->scratch.s1.p;
    d_size = (uint32_t *)c->scratch.s2.p;
    d_offset = (uint32_t *)c->scratch.s3.p;
    d_order = (uint32_t *)c->scratch.s4.p;
  }
  if ((rc = prim_run(c, [&] {
         return mtxd::group_by_u32(keys, n, n_keys, d_size, d_offset, d_order, c->scratch.s5.p, c->stream);
       })))
    return rc;
  return dev ? MTX_OK
             : unstage(c, {{key_size, c->scratch.s2, 4ull * n_keys}, {key_offset, c->scratch.s3, 4ull * n_keys}, {order, c->scratch.s4, 4 * n}});
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
  if ((rc = dalloc(c->scratch.s3, mtxd::scatter_workspace_bytes(n_target, n_value)))) return rc;
  float *d_target = target;
  if (dev) {
    uint32_t bad = 0;
    if ((rc = dev_in_range(c, index, n_value, (uint32_t)n_target, &bad))) return rc;
    if (bad) {
      mtx_set_error("%s: an index is >= n_target (%llu)", fn, (unsigned long long)n_target);
      return MTX_E_ARG;
    }
  } else {
    if ((rc = stage(c, c->scratch.s0, 4 * n_target, target)) || (rc = stage(c, c->scratch.s1, 4 * n_value, value)) ||
        (rc = stage(c, c->scratch.s2, 4 * n_value, index)))
      return rc;
    d_target = (float *)c->scratch.s0.p;
    value = (const float *)c->scratch.s1.p;
    index = (const uint32_t *)c->scratch.s2.p;
  }
  if ((rc = prim_run(c, [&] {
         return mtxd::scatter_reduce_f32(op, d_target, n_target, value, index, n_value, c->scratch.s3.p, c->stream);
       })))
    return rc;
  return dev ? MTX_OK : unstage(c, {{target, c->scratch.s0, 4 * n_target}});
}

static int hashgrid_query_impl(mtx_ctx *c, const char *fn, bool fill, const mtx_hashgrid_view *grid, const float *q,
                               uint64_t m, const float *radius, uint32_t radius_stride, uint32_t *count,
                               const uint32_t *offset, uint64_t total, uint32_t *query_idx, uint32_t *sample_idx_out) {
  if (!c) {
    mtx_set_error("%s: null context", fn);
    return MTX_E_ARG;
  }
  if (m == 0) return MTX_OK;
  if (!q || !radius || radius_stride > 1 || (fill ? !offset || (total && (!query_idx || !sample_idx_out)) : !count)) {
    mtx_set_error("%s: null argument or radius_stride > 1", fn);
    return MTX_E_ARG;
  }
  if (total >= (1ull << 31)) {
    mtx_set_error("%s: total >= 2^31", fn);
    return MTX_E_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  mtxd::HgView g;
  if ((rc = hashgrid_view_check(c, fn, grid, m, &g)) ||
      (rc = need_device(c, fn, {q, radius, count, offset, query_idx, sample_idx_out})))
    return rc;
  if ((rc = dalloc(c->scratch.s6, 64))) return rc;
  HIP_TRY(hipMemsetAsync(c->scratch.s6.p, 0, 4, c->stream));
  uint32_t *d_bad = (uint32_t *)c->scratch.s6.p;
  if ((rc = prim_run(c, [&] {
         if (fill)
           mtxd::launch_hg_fill(g, (uint32_t)m, q, radius, radius_stride, offset, (uint32_t)total, query_idx,
                                sample_idx_out, d_bad, c->stream);
         else
           mtxd::launch_hg_count(g, (uint32_t)m, q, radius, radius_stride, count, d_bad, c->stream);
         return MTX_OK;
       })))
    return rc;
  uint32_t bad = 0;
  HIP_TRY(hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost));
  return bad ? hashgrid_cap_error(fn, bad) : MTX_OK;
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

int mtx_hashgrid_query_count_dev(mtx_ctx *c, const mtx_hashgrid_view *grid, const float *q, uint64_t m,
                                 const float *radius, uint32_t radius_stride, uint32_t *count) {
  return hashgrid_query_impl(c, "mtx_hashgrid_query_count_dev", false, grid, q, m, radius, radius_stride, count,
                             nullptr, 0, nullptr, nullptr);
}
int mtx_hashgrid_query_fill_dev(mtx_ctx *c, const mtx_hashgrid_view *grid, const float *q, uint64_t m,
                                const float *radius, uint32_t radius_stride, const uint32_t *offset, uint64_t total,
                                uint32_t *query_idx, uint32_t *sample_idx_out) {
  return hashgrid_query_impl(c, "mtx_hashgrid_query_fill_dev", true, grid, q, m, radius, radius_stride, nullptr,
                             offset, total, query_idx, sample_idx_out);
}

}  // extern "C"
