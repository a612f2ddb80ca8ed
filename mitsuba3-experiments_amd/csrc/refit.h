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
  RF_EM = 9,        // RF_BAD_AREA: the smallest emitter index it was found on (else 0xffffffff)
  RF_WORDS = 16
};
enum {
  RF_BAD_COORD = 1,    // non-finite or beyond the magnitude bound
  RF_BAD_EMITTER = 2,  // a triangle of a rectangle-emitter shape would move
  RF_BAD_QUANT = 4,    // a level pass could not quantise a bound
  RF_BAD_AREA = 8      // a mesh emitter's triangles have no finite positive total area
};

// Mesh emitter tables (pmf | cdf | prim in the scene's `tables`, mtx.h): one
// EmSlot per mesh emitter and one EmBlock per kEmBlock entries of one emitter,
// both built by the host at upload; a block never spans two emitters.
constexpr uint32_t kEmBlock = 256;
struct EmSlot {
  uint32_t emitter;  // index of the mtx_emitter record
  uint32_t offset;   // mesh_offset: first float of pmf | cdf | prim
  uint32_t count;    // mesh_count
  uint32_t flat;     // first entry in the scratch pmf / cdf
  uint32_t block;    // first EmBlock
  uint32_t pad[3];
};
struct EmBlock {
  uint32_t slot, first;  // entries [first, min(first + kEmBlock, count)) of the slot's emitter
};
// Per-slot words written by the passes (device); the first four also per block.
enum {
  EM_MAX = 0,   // bits of the largest area (NaN and inf order above every finite area)
  EM_MIN = 1,   // bits of the smallest non-zero area, 0xffffffff if none
  EM_LO = 2,    // first entry with pmf > 0, 0xffffffff if none
  EM_HI = 3,    // last entry with pmf > 0
  EM_SUM = 4,   // float cdf[count - 1]
  EM_NORM = 5,  // float 1 / sum
  EM_PATH = 6,  // 1: block-parallel scan, 2: ordered fallback, 0: neither (refused)
  EM_WORDS = 8
};
struct EmTables {
  const EmSlot *slots;
  const EmBlock *blocks;
  uint32_t n_slots, n_blocks;
  uint32_t *state;   // EM_WORDS per slot
  float *pmf, *cdf;  // scratch, flat over all slots
  double *bsum;      // per block: the sum of its areas
  uint32_t *bstat;   // per block: EM_MAX, EM_MIN, EM_LO, EM_HI over its entries
};

float refit_key_decode(uint32_t key);

void refit_state_init(uint32_t *state, hipStream_t st);
// Writes nothing but `state`.
void refit_prepass(const float *vpos, uint32_t n_verts, const uint32_t *tri_vidx, const uint32_t *tri_shape,
                   const mtx_shape *shapes, const mtx_emitter *emitters, const float *shade_rec, uint32_t n_tris,
                   uint32_t *state, hipStream_t st);
// Mesh emitter tables at the new positions, part of the pre-pass: areas, the
// double-accumulated prefix, valid range, sum and normalization into the
// scratch of `t`; a refusal ORs RF_BAD_AREA into state. Writes nothing of the
// scene. `tables`: the scene's (the prim block is read).
void refit_emitter_tables(const EmTables &t, const float *vpos, const uint32_t *tri_vidx, const float *tables,
                          uint32_t *state, hipStream_t st);
// After every check has passed: scratch pmf | cdf into `tables`, the five
// record words (valid_lo, valid_hi, sum, norm, inv_area) into `emitters`.
void refit_emitter_commit(const EmTables &t, float *tables, mtx_emitter *emitters, hipStream_t st);
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
