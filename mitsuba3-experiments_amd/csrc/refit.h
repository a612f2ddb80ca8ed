// refit.h — device passes behind mtx_scene_update_vertices (refit.hip): new
// vertex positions under an unchanged topology, both BVHs refit in place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mtx.h"

namespace mtxd {

// Pre-pass results (device words, refit_state_init before the pre-pass).
enum {
  RF_FLAGS = 0,     // RF_BAD_* bits
  RF_EXTENT = 1,    // closest-hit tree: max |coordinate| bits over referenced vertices
  RF_OCC_EXTENT = 2,  // occlusion tree: the same over v0, v0 + e1, v0 + e2
  RF_LO = 3,        // 3 ordered keys: min over all vertices (refit_key_decode)
  RF_HI = 6,        // 3 ordered keys: max over all vertices
  RF_WORDS = 16
};
enum {
  RF_BAD_COORD = 1,    // non-finite or beyond the magnitude bound
  RF_BAD_EMITTER = 2,  // a triangle of an emitter shape would move
  RF_BAD_QUANT = 4     // a level pass could not quantise a bound
};

float refit_key_decode(uint32_t key);

void refit_state_init(uint32_t *state, hipStream_t st);
// Writes nothing but `state`.
void refit_prepass(const float *vpos, uint32_t n_verts, const uint32_t *tri_vidx, const uint32_t *tri_shape,
                   const mtx_shape *shapes, const float *shade_rec, uint32_t n_tris, uint32_t *state, hipStream_t st);
// Leaf-order triangles: 36-B records, position (and, with vnormal, normal)
// rows of the shading records, vertex-exact boxes into tbox.
void refit_triangles(const float *vpos, const float *vnormal, const uint32_t *tri_vidx, uint32_t n_tris, float *tri,
                     float *shade_rec, float *tbox, hipStream_t st);
// occ_tri[i] = tri[occ_perm[i]] bit for bit; the records' boxes into tbox.
void refit_occ_gather(const float *tri, const uint32_t *occ_perm, uint32_t n_tris, float *occ_tri, float *tbox,
                      hipStream_t st);
// One level of a tree: nodes list[first .. first + count) (list NULL: nodes
// first .. first + count - 1). Children's boxes are read from nbox, the
// nodes' own written to it; a failure ORs RF_BAD_QUANT into state.
void refit_level4(int32_t *nodes, uint32_t first, uint32_t count, const uint32_t *list, const float *tbox, float *nbox,
                  float extent, uint32_t *state, hipStream_t st);
void refit_level8(uint32_t *occ_nodes, uint32_t first, uint32_t count, const uint32_t *list, const float *tbox,
                  float *nbox, float extent, uint32_t *state, hipStream_t st);

}  // namespace mtxd
