// stack_depth.cpp — host probe (tools/stack_depth.py): the closest-hit
// traversal of the 4-wide BVH in the device loop's per-ray order
// (oracle/oracle.cpp trace_closest, device_common.h trace_loop_closest) with
// its stack observed: push_hist[e] counts the pushes that wrote stack entry
// e, max_hist[m] the rays whose stack held at most m entries. An entry
// e >= lds_entries of the persistent kernel is one store to and one load from
// the global spill area.
#include <stdint.h>

#include "mtx.h"
#include "mtx_core/geometry.h"

using namespace mtx;

extern "C" void stack_depth_hist(const int32_t *nodes, const float *tri_geom, const float *rays, uint32_t n_rays,
                                 uint64_t *push_hist, uint64_t *max_hist, uint32_t hist_len, uint64_t *node_visits) {
  uint64_t visits = 0;
  for (uint32_t i = 0; i < n_rays; ++i) {
    const float *q = rays + 8 * (size_t)i;
    const TraceRay r = make_trace_ray(V3{q[0], q[1], q[2]}, V3{q[4], q[5], q[6]}, q[3]);
    float tbest = q[3];
    uint32_t best = 0xffffffffu;
    int32_t stack[3 * MTX_BVH_MAX_DEPTH + 2];
    int sp = 0, sp_max = 0;
    int32_t node = 0;
    while (true) {
      if (node >= 0) {
        const int32_t *w = nodes + MTX_BVH_NODE_WORDS * (size_t)node;
        const float *f = reinterpret_cast<const float *>(w);
        ++visits;
        uint32_t key[4];
        const int n = wide_node_order(r, f[0], f[1], f[2], (uint32_t)w[3], (uint32_t)w[8], (uint32_t)w[9],
                                      (uint32_t)w[10], (uint32_t)w[11], (uint32_t)w[12], (uint32_t)w[13], tbest, key);
        if (n > 0) {
          for (int rr = n - 1; rr >= 1; --rr) {
            if ((uint32_t)sp < hist_len) ++push_hist[sp];
            stack[sp++] = wide_ref(key[rr], w[4], w[5], w[6], w[7]);
          }
          if (sp > sp_max) sp_max = sp;
          node = wide_ref(key[0], w[4], w[5], w[6], w[7]);
          continue;
        }
      } else {
        uint32_t first, count;
        leaf_decode(node, &first, &count);
        for (uint32_t k = 0; k < count; ++k) {
          const uint32_t prim = first + k;
          const float *g = tri_geom + 12 * (size_t)prim;
          float t, u, v;
          if (tri_intersect(r, V3{g[0], g[1], g[2]}, V3{g[4], g[5], g[6]}, V3{g[8], g[9], g[10]}, tbest, &t, &u, &v) &&
              (t < tbest || (t == tbest && prim < best))) {
            tbest = t;
            best = prim;
          }
        }
      }
      if (sp == 0) break;
      node = stack[--sp];
    }
    if ((uint32_t)sp_max < hist_len) ++max_hist[sp_max];
  }
  *node_visits = visits;
}
