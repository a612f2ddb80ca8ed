// scene_check.cpp — the host phase of mtx_scene_upload: every index the
// kernels take from a scene description is checked here, before anything
// reaches a device. No HIP; tests/test_scene_check.py pins each refusal.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "scene_check.h"

namespace mtxh {

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

// Mesh area emitters (mtx.h mtx_emitter: a zero normal): the kernels index
// `tables` and the triangles from the record's words, so every word is
// checked here, on the host, before anything reaches the device. Called once
// tri_shape and the shapes' emitter references are known to be in range.
int check_mesh_emitters(const mtx_scene_desc *d) {
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

int scene_check(const mtx_scene_desc *d, SceneFacts &out) {
  out = SceneFacts{};
  if (!d) {
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
  std::vector<int32_t> &occ_nodes_v = out.occ_nodes_built;
  std::vector<float> &occ_geom_v = out.occ_geom_built;
  std::vector<uint32_t> &occ_perm_v = out.occ_perm;
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
  uint32_t &bvh_depth = out.bvh_depth, &occ_depth = out.occ_depth;
  // level of every reachable node (vertex updates refit level by level)
  std::vector<uint32_t> &level4 = out.level4, &level8 = out.level8;
  level4.assign(d->n_nodes, 0xffffffffu);
  level8.assign(n_occ, 0xffffffffu);
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
  out.occ_nodes = occ_nodes;
  out.occ_geom = occ_geom;
  out.n_occ = n_occ;
  return MTX_OK;
}

}  // namespace mtxh

// Diagnostic export (not in mtx.h): scene_check without a context, and the
// depths it found (closest-hit tree, occlusion tree).
extern "C" int mtx_diag_scene_check(const mtx_scene_desc *d, uint32_t depths_out[2]) {
  mtxh::SceneFacts f;
  const int rc = mtxh::scene_check(d, f);
  if (rc == MTX_OK && depths_out) {
    depths_out[0] = f.bvh_depth;
    depths_out[1] = f.occ_depth;
  }
  return rc;
}
