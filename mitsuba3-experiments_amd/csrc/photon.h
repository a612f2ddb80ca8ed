// photon.h — launch wrappers of photon.hip: the three visitors of the
// hash-grid neighbour walk (hashgrid_query_dev.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hashgrid_query_dev.h"
#include "wavefront.h"

namespace mtxd {

// m queries q (3, m); radius[i * radius_stride]. `bad` (device word, zeroed by
// the caller): queries whose cell box is over MTX_HG_MAX_QUERY_CELLS.
void launch_hg_count(const HgView &g, uint32_t m, const float *q, const float *radius, uint32_t radius_stride,
                     uint32_t *count, uint32_t *bad, hipStream_t st);
void launch_hg_fill(const HgView &g, uint32_t m, const float *q, const float *radius, uint32_t radius_stride,
                    const uint32_t *offset, uint32_t total, uint32_t *query_idx, uint32_t *sample_idx_out,
                    uint32_t *bad, hipStream_t st);
// bad[0]: queries over the cell cap; bad[1]: lanes with a material past n_materials.
void launch_photon_gather(const DevScene &s, uint32_t n_materials, const HgView &g, const mtx_photon_planes &ph,
                          const mtx_visible_planes &vp, uint32_t m, const float *radius, uint32_t radius_stride,
                          uint32_t max_depth, float *out_sum, uint32_t *out_count, uint32_t *bad, hipStream_t st);

}  // namespace mtxd

namespace mtxh {
// prims_entry.cpp: the checks of a caller's grid view (need_device on its
// pointers included) and the error of queries over the cell cap, shared by
// the query entries and the photon gather's.
int hashgrid_view_check(mtx_ctx *c, const char *fn, const mtx_hashgrid_view *g, uint64_t m, mtxd::HgView *out);
int hashgrid_cap_error(const char *fn, uint32_t bad);
}  // namespace mtxh
