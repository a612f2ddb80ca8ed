// scene_check_main.cpp — scene_check (csrc/scene_check.cpp) as a plain host
// program, for AddressSanitizer / UBSan: the check reads indices out of the
// caller's arrays and must not read out of bounds itself before it has
// checked them. Links scene_check.cpp, bvh_build.cpp and error.cpp only;
// built and run by tests/test_scene_check.py. Every array is a std::vector of
// exactly its length, so a read one past the end is a report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <vector>

#include "mtx.h"
#include "scene_check.h"

namespace {

struct Scene {
  std::vector<float> vpos, tri_geom, occ_geom, texels;
  std::vector<uint32_t> tri_vidx, tri_shape, occ_perm;
  std::vector<int32_t> nodes, occ_nodes;
  std::vector<mtx_shape> shapes;
  std::vector<mtx_material> materials;
  std::vector<mtx_emitter> emitters;
  std::vector<mtx_texture> textures;
  uint32_t n_tris = 0, n_nodes = 0, n_occ = 0;
  bool give_occ = true, give_geom = true, give_perm = true;

  mtx_scene_desc desc() const {
    mtx_scene_desc d;
    memset(&d, 0, sizeof d);
    d.n_tris = n_tris;
    d.n_nodes = n_nodes;
    d.n_verts = (uint32_t)(vpos.size() / 3);
    d.n_shapes = (uint32_t)shapes.size();
    d.n_materials = (uint32_t)materials.size();
    d.n_emitters = (uint32_t)emitters.size();
    d.n_textures = (uint32_t)textures.size();
    d.nodes = nodes.data();
    d.tri_geom = tri_geom.data();
    d.tri_vidx = tri_vidx.data();
    d.tri_shape = tri_shape.data();
    d.vpos = vpos.data();
    d.shapes = shapes.data();
    d.materials = materials.data();
    d.emitters = emitters.data();
    d.textures = textures.empty() ? nullptr : textures.data();
    d.texels = texels.data();
    d.n_texels = texels.size();
    d.occ_nodes = give_occ ? occ_nodes.data() : nullptr;
    d.occ_tri_geom = give_geom ? occ_geom.data() : nullptr;
    d.n_occ_nodes = give_occ ? n_occ : 0;
    d.occ_perm = give_perm ? occ_perm.data() : nullptr;
    return d;
  }
};

// A G x G grid of quads in the plane z = 0: 2 G^2 triangles, enough for inner
// children in both trees. One shape, one textured material, one rectangle
// emitter.
Scene make_scene() {
  const uint32_t G = 8, V = G + 1;
  Scene s;
  for (uint32_t j = 0; j < V; ++j)
    for (uint32_t i = 0; i < V; ++i) {
      s.vpos.push_back((float)i);
      s.vpos.push_back((float)j);
      s.vpos.push_back(0.f);
    }
  std::vector<uint32_t> vidx;
  for (uint32_t j = 0; j < G; ++j)
    for (uint32_t i = 0; i < G; ++i) {
      const uint32_t a = j * V + i, b = a + 1, c = a + V, e = c + 1;
      for (uint32_t v : {a, b, e, a, e, c}) vidx.push_back(v);
    }
  s.n_tris = 2 * G * G;
  s.nodes.resize(((size_t)s.n_tris + 1) * MTX_BVH_NODE_WORDS);
  s.tri_geom.resize(12 * (size_t)s.n_tris);
  std::vector<uint32_t> perm(s.n_tris);
  if (mtx_bvh_build(s.vpos.data(), V * V, vidx.data(), s.n_tris, s.nodes.data(), &s.n_nodes, s.tri_geom.data(),
                    perm.data(), nullptr)) {
    fprintf(stderr, "mtx_bvh_build: %s\n", mtx_last_error());
    exit(2);
  }
  s.nodes.resize((size_t)s.n_nodes * MTX_BVH_NODE_WORDS);
  for (uint32_t t = 0; t < s.n_tris; ++t)
    for (int k = 0; k < 3; ++k) s.tri_vidx.push_back(vidx[3 * (size_t)perm[t] + k]);
  s.occ_nodes.resize(((size_t)s.n_tris + 1) * MTX_OCC_NODE_WORDS);
  s.occ_geom.resize(12 * (size_t)s.n_tris);
  s.occ_perm.resize(s.n_tris);
  if (mtx_bvh_build_occlusion(s.tri_geom.data(), s.n_tris, s.occ_nodes.data(), &s.n_occ, s.occ_geom.data(),
                              s.occ_perm.data(), nullptr)) {
    fprintf(stderr, "mtx_bvh_build_occlusion: %s\n", mtx_last_error());
    exit(2);
  }
  s.occ_nodes.resize((size_t)s.n_occ * MTX_OCC_NODE_WORDS);
  s.tri_shape.assign(s.n_tris, 0u);
  s.shapes.push_back(mtx_shape{0u, 0, 1u, 0u});
  mtx_material m;
  memset(&m, 0, sizeof m);
  m.type = MTX_MAT_DIFFUSE;
  m.tex = 0;
  m.table = -1;
  s.materials.push_back(m);
  s.textures.push_back(mtx_texture{2u, 2u, 0u});
  s.texels.assign(12, 0.5f);
  mtx_emitter e;
  memset(&e, 0, sizeof e);
  e.col0[0] = e.col1[1] = e.normal[2] = 1.f;
  e.inv_area = 0.25f;
  e.radiance[0] = e.radiance[1] = e.radiance[2] = 1.f;
  s.emitters.push_back(e);
  return s;
}

int failures = 0;

void expect(const char *name, const Scene &s, const char *match) {
  const mtx_scene_desc d = s.desc();
  mtxh::SceneFacts f;
  const int rc = mtxh::scene_check(&d, f);
  const bool ok = match ? rc == MTX_E_ARG && strstr(mtx_last_error(), match) : rc == MTX_OK;
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAIL %s: rc %d, \"%s\" (wanted %s)\n", name, rc, mtx_last_error(), match ? match : "MTX_OK");
  }
}

void refused(const char *name, const Scene &good, const char *match, const std::function<void(Scene &)> &corrupt) {
  Scene s = good;
  corrupt(s);
  expect(name, s, match);
}

uint32_t *node8(Scene &s, uint32_t nd) { return (uint32_t *)s.occ_nodes.data() + (size_t)MTX_OCC_NODE_WORDS * nd; }
uint32_t meta8(const uint32_t *w, uint32_t sl) { return (w[6 + (sl >> 2)] >> (8 * (sl & 3))) & 0xffu; }
void set_meta8(uint32_t *w, uint32_t sl, uint32_t m) {
  uint32_t &x = w[6 + (sl >> 2)];
  x = (x & ~(0xffu << (8 * (sl & 3)))) | (m << (8 * (sl & 3)));
}

}  // namespace

int main() {
  const Scene good = make_scene();
  // where the corruptions go: an inner and a leaf reference of the 4-wide
  // tree, an inner and a leaf slot of the 8-wide tree
  int in4 = -1, leaf4 = -1;
  for (uint32_t nd = 0; nd < good.n_nodes; ++nd)
    for (uint32_t k = 0; k < ((uint32_t)good.nodes[16 * (size_t)nd + 3] >> 24); ++k) {
      const size_t at = 16 * (size_t)nd + 4 + k;
      if (good.nodes[at] >= 0 && in4 < 0) in4 = (int)at;
      if (good.nodes[at] < 0 && leaf4 < 0) leaf4 = (int)at;
    }
  int in8_nd = -1, in8_sl = -1, leaf8_nd = -1, leaf8_sl = -1;
  {
    Scene s = good;
    for (uint32_t nd = 0; nd < s.n_occ; ++nd)
      for (uint32_t sl = 0; sl < MTX_OCC_WIDTH; ++sl) {
        const uint32_t *w = node8(s, nd);
        const bool inner = ((w[3] >> 24) >> sl) & 1u;
        if (inner && in8_nd < 0) in8_nd = (int)nd, in8_sl = (int)sl;
        if (!inner && meta8(w, sl) && leaf8_nd < 0) leaf8_nd = (int)nd, leaf8_sl = (int)sl;
      }
  }
  if (in4 < 0 || leaf4 < 0 || in8_nd < 0 || leaf8_nd < 0) {
    fprintf(stderr, "the scene lacks an inner child or a leaf in one of its trees\n");
    return 2;
  }

  expect("intact", good, nullptr);
  refused("intact, correspondence derived", good, nullptr, [](Scene &s) { s.give_perm = false; });
  refused("intact, tree built inside", good, nullptr, [](Scene &s) { s.give_occ = s.give_geom = s.give_perm = false; });

  refused("4: cycle", good, "BVH is not a tree", [&](Scene &s) { s.nodes[in4] = 0; });
  refused("4: no children", good, "has 0 children", [](Scene &s) { s.nodes[3] &= 0x00ffffff; });
  refused("4: five children", good, "has 5 children",
          [](Scene &s) { s.nodes[3] = (s.nodes[3] & 0x00ffffff) | (5 << 24); });
  refused("4: child n_nodes", good, "out of range", [&](Scene &s) { s.nodes[in4] = (int32_t)s.n_nodes; });
  refused("4: leaf past n_tris", good, "exceeds",
          [&](Scene &s) { s.nodes[leaf4] = ~(int32_t)(((s.n_tris - 1) << 3) | 1u); });

  refused("8: cycle", good, "occlusion BVH is not a tree", [&](Scene &s) { node8(s, in8_nd)[4] = 0; });
  refused("8: inner meta", good, "bad inner child",
          [&](Scene &s) { set_meta8(node8(s, in8_nd), in8_sl, (0x20u | (24u + in8_sl)) ^ 1u); });
  refused("8: child n_occ", good, "bad inner child", [&](Scene &s) { node8(s, in8_nd)[4] = s.n_occ; });
  refused("8: leaf count code", good, "bad leaf", [&](Scene &s) {
    uint32_t *w = node8(s, leaf8_nd);
    set_meta8(w, leaf8_sl, (2u << 5) | (meta8(w, leaf8_sl) & 31u));
  });
  refused("8: leaf off + cnt > 24", good, "bad leaf", [&](Scene &s) {
    uint32_t *w = node8(s, leaf8_nd);
    set_meta8(w, leaf8_sl, (meta8(w, leaf8_sl) & 0xe0u) | 24u);
  });
  refused("8: tri_base past n_tris", good, "bad leaf", [&](Scene &s) { node8(s, leaf8_nd)[5] = s.n_tris; });

  refused("occ_nodes without occ_tri_geom", good, "go together", [](Scene &s) { s.give_geom = false; });
  refused("foreign record, perm given", good, "occ_perm[4]", [](Scene &s) { s.occ_geom[12 * 4 + 5] += 0.25f; });
  refused("foreign record, perm derived", good, "not a permutation of tri_geom", [](Scene &s) {
    s.occ_geom[12 * 4 + 5] += 0.25f;
    s.give_perm = false;
  });
  refused("perm twice", good, "occ_perm[1]", [](Scene &s) { s.occ_perm[1] = s.occ_perm[0]; });
  refused("perm out of range", good, "occ_perm[2]", [](Scene &s) { s.occ_perm[2] = s.n_tris; });
  refused("vertex n_verts", good, "vertex index out of range",
          [](Scene &s) { s.tri_vidx[5] = (uint32_t)(s.vpos.size() / 3); });
  refused("shape n_shapes", good, "shape index out of range", [](Scene &s) { s.tri_shape[3] = 1; });
  refused("material n_materials", good, "missing material/emitter", [](Scene &s) { s.shapes[0].material = 1; });
  refused("emitter n_emitters", good, "missing material/emitter", [](Scene &s) { s.shapes[0].emitter = 1; });
  refused("texture n_textures", good, "texture out of range", [](Scene &s) { s.materials[0].tex = 1; });
  refused("texture extent", good, "exceeds texel buffer", [](Scene &s) { s.textures[0].offset = 1; });
  refused("roughplastic without table", good, "no transmittance table",
          [](Scene &s) { s.materials[0].type = MTX_MAT_ROUGHPLASTIC; });

  if (failures) return 1;
  printf("scene_check_main: OK\n");
  return 0;
}
