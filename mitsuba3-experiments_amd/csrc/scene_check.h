// scene_check.h — the host phase of mtx_scene_upload (scene_check.cpp).
// Internal, no HIP: tests/host links it into a plain host program.
#pragma once
#include <stdint.h>

#include <vector>

#include "mtx.h"

void mtx_set_error(const char *fmt, ...);  // error.cpp

namespace mtxh {

// What the device phase needs from the check.
struct SceneFacts {
  uint32_t bvh_depth = 0, occ_depth = 0, n_occ = 0;
  // level of every node of the two trees (0xffffffff: unreachable), and
  // occlusion triangle -> scene triangle
  std::vector<uint32_t> level4, level8, occ_perm;
  std::vector<int32_t> occ_nodes_built;  // the occlusion tree built here; empty when the caller gave one
  std::vector<float> occ_geom_built;
  const int32_t *occ_nodes = nullptr;  // the caller's or the built tree
  const float *occ_geom = nullptr;
};

// Everything mtx_scene_upload decides on the host: MTX_OK means no kernel can
// index out of bounds through this description. Touches no device.
int scene_check(const mtx_scene_desc *d, SceneFacts &out);

// The mesh emitter records alone (also mtx_blocks_light_host). Needs
// tri_shape and the shapes' emitter references in range.
int check_mesh_emitters(const mtx_scene_desc *d);

}  // namespace mtxh
