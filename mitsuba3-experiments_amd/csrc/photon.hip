// photon.hip — fixed-radius queries on the hash grid and the photon gather:
// three visitors of the one neighbour walk (hashgrid_query_dev.h). One lane
// handles one query in a grid-stride loop, like the other blocks; the walk's
// order (cz, cy, cx, then ascending sample index) is each lane's summation
// order, so the gather equals its composition from the blocks bit for bit.
//
// Queries arrive in pixel order, so the lanes of a wave walk overlapping cell
// boxes: their cell_size / cell_offset words and most of their candidates'
// points come from the same few lines. The trip count differs per lane (the
// number of candidates in the lane's cells); a wave runs as long as its
// busiest lane.
#include "photon.h"

#include <algorithm>

#include "device_common.h"

namespace mtxd {

namespace {

constexpr int kPhotonBlock = 256;

__device__ __forceinline__ V3 ld3(const float *a, uint32_t n, uint32_t i) {
  return V3{a[i], a[(size_t)n + i], a[2 * (size_t)n + i]};
}

__global__ __launch_bounds__(kPhotonBlock) void k_hg_count(HgView g, uint32_t m, const float *q, const float *radius,
                                                           uint32_t radius_stride, uint32_t *count, uint32_t *bad) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    const V3 qq = ld3(q, m, i);
    const float r = radius[(size_t)i * radius_stride];
    uint32_t c = 0;
    HgBox box;
    const int st = hg_box(g, qq.x, qq.y, qq.z, r, &box);
    if (st == 2) atomicAdd(bad, 1u);
    if (st == 0) hg_walk(g, box, qq.x, qq.y, qq.z, r, [&](uint32_t, float, float, float) { ++c; });
    count[i] = c;
  }
}

__global__ __launch_bounds__(kPhotonBlock) void k_hg_fill(HgView g, uint32_t m, const float *q, const float *radius,
                                                          uint32_t radius_stride, const uint32_t *offset,
                                                          uint32_t total, uint32_t *query_idx,
                                                          uint32_t *sample_idx_out, uint32_t *bad) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    const V3 qq = ld3(q, m, i);
    const float r = radius[(size_t)i * radius_stride];
    HgBox box;
    const int st = hg_box(g, qq.x, qq.y, qq.z, r, &box);
    if (st == 2) atomicAdd(bad, 1u);
    if (st != 0) continue;
    uint32_t k = offset[i];
    hg_walk(g, box, qq.x, qq.y, qq.z, r, [&](uint32_t j, float, float, float) {
      if (k < total) {  // offset is the caller's: nothing is written past the pair arrays
        query_idx[k] = i;
        sample_idx_out[k] = j;
      }
      ++k;
    });
  }
}

// The hot path: the density estimate at a visible point over the photons
// within r (include/mtx.h mtx_blocks_photon_gather_dev has the per-neighbour
// operation sequence).
__global__ __launch_bounds__(kPhotonBlock) void k_photon_gather(DevScene s, uint32_t n_materials, HgView g,
                                                                mtx_photon_planes ph, mtx_visible_planes vp,
                                                                uint32_t m, const float *radius,
                                                                uint32_t radius_stride, uint32_t max_depth,
                                                                float *out_sum, uint32_t *out_count, uint32_t *bad) {
  const SceneView view = make_view(s);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    const V3 qq = ld3(vp.p, m, i);
    const float r = radius[(size_t)i * radius_stride];
    int32_t mi = vp.material[i];
    if (mi >= 0 && (uint32_t)mi >= n_materials) {
      atomicAdd(bad + 1, 1u);
      mi = -1;
    }
    V3 acc = v3s(0.f);
    uint32_t cnt = 0;
    HgBox box;
    const int st = hg_box(g, qq.x, qq.y, qq.z, r, &box);
    if (st == 2) atomicAdd(bad, 1u);
    if (st == 0 && mi >= 0) {
      const mtx_material mat = s.materials[mi];
      const V2 uv = V2{vp.uv[i], vp.uv[(size_t)m + i]};
      const V3 wi = ld3(vp.wi, m, i), ng = ld3(vp.n, m, i);
      const Frame fr = frame_from_normal(ld3(vp.sh_n, m, i));
      const int64_t dq = vp.depth[i];
      hg_walk(g, box, qq.x, qq.y, qq.z, r, [&](uint32_t j, float, float, float) {
        if (dq + (int64_t)ph.depth[j] > (int64_t)max_depth) return;
        const V3 dp = ld3(ph.d, g.n, j);
        const V3 wo = to_local(fr, dp);
        V3 val;
        float pdf;
        bsdf_eval_pdf(view.bsdf, mat, uv, wi, wo, &val, &pdf);
        const float cg = dot(ng, dp);
        if (!(cg * wo.z > 0.f) || !(wi.z * wo.z > 0.f)) return;
        const V3 b = ld3(ph.beta, g.n, j);
        const float ac = fabsf(cg);
        acc = acc + V3{(val.x * b.x) / ac, (val.y * b.y) / ac, (val.z * b.z) / ac};
        ++cnt;
      });
    }
    out_sum[i] = acc.x;
    out_sum[(size_t)m + i] = acc.y;
    out_sum[2 * (size_t)m + i] = acc.z;
    out_count[i] = cnt;
  }
}

inline unsigned photon_grid(uint32_t n) {
  return std::max(1u, std::min<unsigned>((n + kPhotonBlock - 1) / kPhotonBlock, 256u * 32u));
}

}  // namespace

void launch_hg_count(const HgView &g, uint32_t m, const float *q, const float *radius, uint32_t radius_stride,
                     uint32_t *count, uint32_t *bad, hipStream_t st) {
  hipLaunchKernelGGL(k_hg_count, dim3(photon_grid(m)), dim3(kPhotonBlock), 0, st, g, m, q, radius, radius_stride,
                     count, bad);
}
void launch_hg_fill(const HgView &g, uint32_t m, const float *q, const float *radius, uint32_t radius_stride,
                    const uint32_t *offset, uint32_t total, uint32_t *query_idx, uint32_t *sample_idx_out,
                    uint32_t *bad, hipStream_t st) {
  hipLaunchKernelGGL(k_hg_fill, dim3(photon_grid(m)), dim3(kPhotonBlock), 0, st, g, m, q, radius, radius_stride,
                     offset, total, query_idx, sample_idx_out, bad);
}
void launch_photon_gather(const DevScene &s, uint32_t n_materials, const HgView &g, const mtx_photon_planes &ph,
                          const mtx_visible_planes &vp, uint32_t m, const float *radius, uint32_t radius_stride,
                          uint32_t max_depth, float *out_sum, uint32_t *out_count, uint32_t *bad, hipStream_t st) {
  hipLaunchKernelGGL(k_photon_gather, dim3(photon_grid(m)), dim3(kPhotonBlock), 0, st, s, n_materials, g, ph, vp, m,
                     radius, radius_stride, max_depth, out_sum, out_count, bad);
}

}  // namespace mtxd
