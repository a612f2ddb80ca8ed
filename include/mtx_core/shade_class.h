// shade_class.h — the shading class of a hit: which BSDF code a lane of the
// wavefront shade step runs. k_shade sorts its queue windows by this class
// so that a block step holds one class (shade.hip shade_loop<INT, CAM, CLS>).
// The split lives here only: the class count, the type -> class mapping and
// the way the class is read from a triangle's shading record.
#pragma once
#include "../mtx.h"
#include "common.h"

namespace mtx {

// class 0: diffuse, and every lane that runs no BSDF code (a miss, an
// invalid hit); class 1: roughplastic; class 2: every other type.
constexpr uint32_t kShadeClasses = 3;

MTX_HD uint32_t shade_class_of_type(uint32_t type) {
  return type == MTX_MAT_DIFFUSE ? 0u : type == MTX_MAT_ROUGHPLASTIC ? 1u : 2u;
}

// Bits 8..12 of a shading record's flag word (word 11, mtx_scene_upload):
// 1 + (type << 2 | textured << 1 | masked); 0 is no record (a miss).
MTX_HD uint32_t shade_rec_class_bits(uint32_t type, bool textured, bool masked) {
  return 1u + ((type & 7u) << 2 | (textured ? 2u : 0u) | (masked ? 1u : 0u));
}
MTX_HD uint32_t shade_class_of_rec(uint32_t flag_word) {
  const uint32_t c = (flag_word >> 8) & 0x1fu;
  return c ? shade_class_of_type((c - 1u) >> 2) : 0u;
}

}  // namespace mtx
