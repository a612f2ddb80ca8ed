// scene.cpp — the scene on the device: the device phase of mtx_scene_upload
// (scene_check.cpp is the host phase), the camera, vertex updates (refit.hip)
// and the read-back hook.
#include <string.h>

#include <algorithm>
#include <vector>

#include "runtime.h"
#include "mtx_core/interaction.h"
#include "mtx_core/shade_class.h"
#include "scene_check.h"

using namespace mtxh;

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

extern "C" {

int mtx_scene_upload(mtx_ctx *c, const mtx_scene_desc *d) {
  if (!c) {
    mtx_set_error("mtx_scene_upload: null argument");
    return MTX_E_ARG;
  }
  // Host phase: a refusal leaves the bound scene as it was.
  SceneFacts facts;
  int rc = scene_check(d, facts);
  if (rc) return rc;
  const int32_t *occ_nodes = facts.occ_nodes;
  const float *occ_geom = facts.occ_geom;
  const std::vector<uint32_t> &occ_perm_v = facts.occ_perm, &level4 = facts.level4, &level8 = facts.level8;
  const uint32_t n_occ = facts.n_occ, bvh_depth = facts.bvh_depth, occ_depth = facts.occ_depth;
  // Device phase. The buffers are rewritten one after another: a failure in
  // the middle must not leave a mix of two scenes live.
  HIP_TRY(hipSetDevice(c->device));
  c->scene_dropped();
  hipStream_t st = c->stream;
  if ((rc = upload(c->scene.nodes, d->nodes, (size_t)MTX_BVH_NODE_WORDS * d->n_nodes, st))) return rc;
  if ((rc = upload(c->scene.occ_nodes, occ_nodes, (size_t)MTX_OCC_NODE_WORDS * n_occ, st))) return rc;
  for (int tree = 0; tree < 2; ++tree) {
    // device triangles packed to 36 B (the ABI's 48-B records carry 3 pad
    // words): 3.6 instead of 2.7 triangles per 128-B line, same load count
    const float *src = tree ? occ_geom : d->tri_geom;
    std::vector<float> g9(9ull * d->n_tris);
    for (size_t i = 0; i < d->n_tris; ++i)
      for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) g9[9 * i + 3 * k + j] = src[12 * i + 4 * k + j];
    if ((rc = upload(tree ? c->scene.occ_tri : c->scene.tri, g9.data(), g9.size(), st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // g9 is freed at scope exit
  }
  if ((rc = upload(c->refit.occ_perm, occ_perm_v.data(), (size_t)d->n_tris, st))) return rc;
  if ((rc = upload_levels(level4, bvh_depth, c->refit.lvl4_first, c->refit.lvl4_list, st))) return rc;
  if ((rc = upload_levels(level8, occ_depth, c->refit.lvl8_first, c->refit.lvl8_list, st))) return rc;
  c->scene.n_nodes = d->n_nodes;
  c->scene.n_occ = n_occ;
  c->scene.n_verts = d->n_verts;
  if ((rc = upload(c->scene.tri_vidx, d->tri_vidx, 3ull * d->n_tris, st))) return rc;
  if ((rc = upload(c->scene.tri_shape, d->tri_shape, (size_t)d->n_tris, st))) return rc;
  if ((rc = upload(c->scene.vpos, d->vpos, 3ull * d->n_verts, st))) return rc;
  if ((rc = upload(c->scene.vnormal, d->vnormal, d->vnormal ? 3ull * d->n_verts : 0, st))) return rc;
  if ((rc = upload(c->scene.vuv, d->vuv, d->vuv ? 2ull * d->n_verts : 0, st))) return rc;
  if ((rc = upload(c->scene.shapes, d->shapes, d->n_shapes, st))) return rc;
  c->scene.n_shapes = d->n_shapes;
  if ((rc = upload(c->scene.materials, d->materials, d->n_materials, st))) return rc;
  if ((rc = upload(c->scene.emitters, d->emitters, d->n_emitters, st))) return rc;
  if ((rc = upload(c->scene.textures, d->textures, d->n_textures, st))) return rc;
  if ((rc = upload(c->scene.texels, d->texels, d->n_texels, st))) return rc;
  if ((rc = upload(c->scene.tables, d->tables, d->n_tables, st))) return rc;
  c->scene.n_tables = d->n_tables;
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
    mtxd::EmTables &t = c->refit.em_tables;
    t = {};
    t.n_slots = (uint32_t)slots.size();
    t.n_blocks = (uint32_t)blks.size();
    if ((rc = upload(c->refit.em_slots, slots.data(), slots.size(), st))) return rc;
    if ((rc = upload(c->refit.em_blocks, blks.data(), blks.size(), st))) return rc;
    if ((rc = dalloc(c->refit.em_state, 4ull * mtxd::EM_WORDS * slots.size()))) return rc;
    if ((rc = dalloc(c->refit.em_pmf, 4ull * flat))) return rc;
    if ((rc = dalloc(c->refit.em_cdf, 4ull * flat))) return rc;
    if ((rc = dalloc(c->refit.em_bsum, 8ull * blks.size()))) return rc;
    if ((rc = dalloc(c->refit.em_bstat, 16ull * blks.size()))) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // slots and blks are freed at scope exit
    t.slots = (const mtxd::EmSlot *)c->refit.em_slots.p;
    t.blocks = (const mtxd::EmBlock *)c->refit.em_blocks.p;
    t.state = (uint32_t *)c->refit.em_state.p;
    t.pmf = (float *)c->refit.em_pmf.p;
    t.cdf = (float *)c->refit.em_cdf.p;
    t.bsum = (double *)c->refit.em_bsum.p;
    t.bstat = (uint32_t *)c->refit.em_bstat.p;
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
      // bits 8..12: the material's type, textured and masked bits; k_shade
      // reads its entries' shading class from them (mtx_core/shade_class.h)
      const mtx_material &m = d->materials[sh.material];
      const uint32_t cls = mtx::shade_rec_class_bits(m.type, m.tex >= 0, (m.flags & MTX_MF_MASK) != 0);
      const uint32_t mat = sh.material, fl = use_n | use_uv | (cls << 8);
      const int32_t em = sh.emitter;
      memcpy(&r[3], &mat, 4);
      memcpy(&r[7], &em, 4);
      memcpy(&r[11], &fl, 4);
    }
    if ((rc = upload(c->scene.shade_rec, rec.data(), rec.size(), st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // rec is freed at scope exit
  }
  HIP_TRY(hipStreamSynchronize(st));
  mtxd::DevScene &s = c->scene.dev;
  s.nodes = (const int4 *)c->scene.nodes.p;
  s.tri = (const float *)c->scene.tri.p;
  s.occ_nodes = (const int4 *)c->scene.occ_nodes.p;
  s.occ_tri = (const float *)c->scene.occ_tri.p;
  s.tri_vidx = (const uint32_t *)c->scene.tri_vidx.p;
  s.tri_shape = (const uint32_t *)c->scene.tri_shape.p;
  s.vpos = (const float *)c->scene.vpos.p;
  s.vnormal = (const float *)c->scene.vnormal.p;
  s.vuv = (const float *)c->scene.vuv.p;
  s.shapes = (const mtx_shape *)c->scene.shapes.p;
  s.shade_rec = (const float4 *)c->scene.shade_rec.p;
  s.materials = (const mtx_material *)c->scene.materials.p;
  s.emitters = (const mtx_emitter *)c->scene.emitters.p;
  s.textures = (const mtx_texture *)c->scene.textures.p;
  s.texels = (const float *)c->scene.texels.p;
  s.tables = (const float *)c->scene.tables.p;
  s.n_tris = d->n_tris;
  s.n_emitters = d->n_emitters;
  c->scene.n_materials = d->n_materials;
  s.camera = d->camera;
  s.has_env = d->has_env ? 1u : 0u;
  for (int k = 0; k < 3; ++k) s.env_radiance[k] = d->env_radiance[k];
  mtx::env_bsphere(d->vpos, d->n_verts, s.env_center, &s.env_radius);
  // LDS per trace block (8 blocks of 256 threads per CU fill the 160 KB):
  // closest hit 16 x 4-B stack entries per lane + 64 nodes of 64 B,
  // occlusion 8 x 8-B entries + 48 nodes of 80 B
  s.stack_entries = 3 * bvh_depth + 1;
  s.lds_entries = std::min<uint32_t>(s.stack_entries, c->knobs.lds_stack);
  s.lds_top = std::min<uint32_t>(d->n_nodes, c->knobs.lds_top);
  s.occ_stack_entries = occ_depth + 1;
  s.occ_lds_entries = std::min<uint32_t>(s.occ_stack_entries, c->knobs.occ_lds_stack);
  s.occ_lds_top = std::min<uint32_t>(n_occ, c->knobs.occ_lds_top);
  mtxd::split_trace_lds(s, c->knobs.trace_ring);  // k_trace_closest: its rings' bytes come out of its stack entries
  s.trace_batch = c->knobs.trace_batch;
  s.urefill = c->knobs.urefill;
  s.cam_urefill = c->knobs.cam_urefill;
  s.occ_urefill = c->knobs.occ_urefill;
  s.xcd_claim = c->knobs.xcd_claim;
  c->trace_grid = c->n_cu * mtxd::trace_blocks_per_cu(s);
  c->closest_grid = c->n_cu * mtxd::closest_blocks_per_cu(s);
  c->mega_grid = c->n_cu * mtxd::mega_blocks_per_cu(s);
  s.ovf_threads = (uint32_t)std::max(c->trace_grid, c->closest_grid) * mtxd::kTraceBlock;
  if ((rc = dalloc(c->wave[0].stack_ovf, mtxd::stack_ovf_bytes(s)))) return rc;  // wave 1's: ensure_wave
  s.stack_ovf = c->wave[0].stack_ovf.p;
  c->scene.live = true;
  return MTX_OK;
}

int mtx_set_camera(mtx_ctx *c, const mtx_camera *cam) {
  if (!c || !cam) {
    mtx_set_error("mtx_set_camera: null argument");
    return MTX_E_ARG;
  }
  if (!c->scene.live) {
    mtx_set_error("no scene uploaded");
    return MTX_E_NOSCENE;
  }
  if (cam->width != c->scene.dev.camera.width || cam->height != c->scene.dev.camera.height) {
    mtx_set_error("mtx_set_camera: film size changed (%ux%u -> %ux%u)", c->scene.dev.camera.width,
                  c->scene.dev.camera.height, cam->width, cam->height);
    return MTX_E_ARG;
  }
  c->scene.dev.camera = *cam;
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
  if (!c->scene.live) {
    mtx_set_error("no scene uploaded");
    return MTX_E_NOSCENE;
  }
  if (n_verts != c->scene.n_verts) {
    mtx_set_error("mtx_scene_update_vertices: %u vertices given, the scene has %u (topology changes need a new upload)",
                  n_verts, c->scene.n_verts);
    return MTX_E_ARG;
  }
  if (vnormal && !c->scene.vnormal.p) {
    mtx_set_error("mtx_scene_update_vertices: the scene was uploaded without vertex normals");
    return MTX_E_ARG;
  }
  int rc;
  if (dev && (rc = need_device(c, "mtx_scene_update_vertices", {vpos, vnormal}))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const mtxd::DevScene &s = c->scene.dev;
  const uint32_t n_tris = s.n_tris;
  const size_t vbytes = 12ull * n_verts;
  if ((rc = dalloc(c->refit.state, mtxd::RF_WORDS * sizeof(uint32_t)))) return rc;
  if ((rc = dalloc(c->refit.tbox, 24ull * n_tris))) return rc;
  if ((rc = dalloc(c->refit.nbox, 24ull * std::max(c->scene.n_nodes, c->scene.n_occ)))) return rc;
  const float *vp = vpos, *vn = vnormal;
  if (!dev) {  // stage the host arrays: the scene's own copies stay until the checks pass
    if ((rc = dalloc(c->refit.vpos, vbytes))) return rc;
    HIP_TRY(hipMemcpyAsync(c->refit.vpos.p, vpos, vbytes, hipMemcpyHostToDevice, st));
    vp = (const float *)c->refit.vpos.p;
    if (vnormal) {
      if ((rc = dalloc(c->refit.vnormal, vbytes))) return rc;
      HIP_TRY(hipMemcpyAsync(c->refit.vnormal.p, vnormal, vbytes, hipMemcpyHostToDevice, st));
      vn = (const float *)c->refit.vnormal.p;
    }
  }
  uint32_t *state = (uint32_t *)c->refit.state.p;
  mtxd::refit_state_init(state, st);
  mtxd::refit_prepass(vp, n_verts, s.tri_vidx, s.tri_shape, s.shapes, s.emitters, (const float *)c->scene.shade_rec.p,
                      n_tris, state, st);
  mtxd::refit_emitter_tables(c->refit.em_tables, vp, s.tri_vidx, s.tables, state, st);
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
  if (vp != (const float *)c->scene.vpos.p)
    HIP_TRY(hipMemcpyAsync(c->scene.vpos.p, vp, vbytes, hipMemcpyDeviceToDevice, st));
  if (vn && vn != (const float *)c->scene.vnormal.p)
    HIP_TRY(hipMemcpyAsync(c->scene.vnormal.p, vn, vbytes, hipMemcpyDeviceToDevice, st));
  float *tbox = (float *)c->refit.tbox.p, *nbox = (float *)c->refit.nbox.p;
  mtxd::refit_triangles(vp, vn, s.tri_vidx, n_tris, (float *)c->scene.tri.p, (float *)c->scene.shade_rec.p, tbox, st);
  mtxd::refit_emitter_commit(c->refit.em_tables, (float *)c->scene.tables.p, (mtx_emitter *)c->scene.emitters.p, st);
  const float extent = mtx::u2f(h[mtxd::RF_EXTENT]), occ_extent = mtx::u2f(h[mtxd::RF_OCC_EXTENT]);
  for (size_t l = c->refit.lvl4_first.size() - 1; l-- > 0;)
    mtxd::refit_level4((int32_t *)c->scene.nodes.p, c->refit.lvl4_first[l], c->refit.lvl4_first[l + 1] - c->refit.lvl4_first[l],
                       (const uint32_t *)c->refit.lvl4_list.p, tbox, nbox, extent, state, st);
  mtxd::refit_occ_gather((const float *)c->scene.tri.p, (const uint32_t *)c->refit.occ_perm.p, n_tris, (float *)c->scene.occ_tri.p, tbox,
                         st);
  for (size_t l = c->refit.lvl8_first.size() - 1; l-- > 0;)
    mtxd::refit_level8((uint32_t *)c->scene.occ_nodes.p, c->refit.lvl8_first[l], c->refit.lvl8_first[l + 1] - c->refit.lvl8_first[l],
                       (const uint32_t *)c->refit.lvl8_list.p, tbox, nbox, occ_extent, state, st);
  uint32_t flags = 0;
  hipError_t e = hipMemcpyAsync(&flags, state + mtxd::RF_FLAGS, sizeof(flags), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess || (flags & mtxd::RF_BAD_QUANT)) {
    c->scene_dropped();  // never leave a half-refit tree live
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
  mtx::env_bsphere_box(lo, hi, c->scene.dev.env_center, &c->scene.dev.env_radius);
  c->geometry_moved();  // the ReSTIR GI reservoirs are kept (runtime.h RestirState)
  return MTX_OK;
}

// Diagnostic export (not in mtx.h; needs no device): the shading class of
// every triangle of a scene description, read back from the flag word the
// record builder of mtx_scene_upload writes (out: n_tris bytes).
int mtx_diag_shade_classes(const mtx_scene_desc *d, uint8_t *out) {
  if (!d || !out || !d->tri_shape || !d->shapes || !d->materials) {
    mtx_set_error("mtx_diag_shade_classes: null argument");
    return MTX_E_ARG;
  }
  for (uint32_t t = 0; t < d->n_tris; ++t) {
    const uint32_t sh = d->tri_shape[t];
    if (sh >= d->n_shapes || d->shapes[sh].material >= d->n_materials) {
      mtx_set_error("mtx_diag_shade_classes: triangle %u: shape or material out of range", t);
      return MTX_E_ARG;
    }
    const mtx_material &m = d->materials[d->shapes[sh].material];
    const uint32_t fl = mtx::shade_rec_class_bits(m.type, m.tex >= 0, (m.flags & MTX_MF_MASK) != 0) << 8;
    out[t] = (uint8_t)mtx::shade_class_of_rec(fl);
  }
  return MTX_OK;
}

// Test / debugging hook: the device copy of one scene array.
int mtx_scene_read(mtx_ctx *c, int which, void *out, uint64_t n_bytes) {
  if (!c || !out) {
    mtx_set_error("mtx_scene_read: null argument");
    return MTX_E_ARG;
  }
  if (!c->scene.live) {
    mtx_set_error("no scene uploaded");
    return MTX_E_NOSCENE;
  }
  const uint64_t nt = c->scene.dev.n_tris, nv = c->scene.n_verts;
  const void *src = nullptr;
  uint64_t need = 0;
  switch (which) {
    case 0: src = c->scene.nodes.p; need = 4ull * MTX_BVH_NODE_WORDS * c->scene.n_nodes; break;
    case 1: src = c->scene.occ_nodes.p; need = 4ull * MTX_OCC_NODE_WORDS * c->scene.n_occ; break;
    case 2: src = c->scene.tri.p; need = 36 * nt; break;
    case 3: src = c->scene.occ_tri.p; need = 36 * nt; break;
    case 4: src = c->scene.shade_rec.p; need = 128 * nt; break;
    case 5: src = c->scene.vpos.p; need = 12 * nv; break;
    case 6: src = c->scene.vnormal.p; need = c->scene.vnormal.p ? 12 * nv : 0; break;
    case 7: need = 16; break;
    case 8: src = c->scene.tables.p; need = 4ull * c->scene.n_tables; break;
    case 9: src = c->scene.emitters.p; need = sizeof(mtx_emitter) * (uint64_t)c->scene.dev.n_emitters; break;
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
    float sph[4] = {c->scene.dev.env_center[0], c->scene.dev.env_center[1], c->scene.dev.env_center[2], c->scene.dev.env_radius};
    memcpy(out, sph, sizeof(sph));
    return MTX_OK;
  }
  if (need == 0) return MTX_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
  return MTX_OK;
}

}  // extern "C"
