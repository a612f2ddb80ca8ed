/* mtx.h — C ABI of libmtx, the MI355X (gfx950) wavefront path-tracing
 * integrator that replaces the per-bounce `sample()` loop of
 * DoeringChristian/mitsuba3-experiments.
 *
 * Plain C: fixed-width integers, floats, pointers and sizes only. Every entry
 * point returns 0 on success and a negative MTX_E* code on failure; the
 * message is available from mtx_last_error() (thread-local). No exceptions
 * cross the ABI. Host buffers are caller-owned and only read/written during
 * the call; calls are synchronous with respect to their outputs. A context
 * is bound to one HIP device and is not thread-safe: one host thread per
 * context (ctypes releases the GIL during the call, so N Python threads or N
 * processes can drive N GPUs).
 *
 * What each entry point replaces in the reference (file:line under the
 * reference root) is stated above its declaration. The ctypes binding a
 * maintainer adds on the reference side is in INTEGRATION.md.
 */
#ifndef MTX_H_
#define MTX_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTX_ABI_VERSION 8

enum {
  MTX_OK = 0,
  MTX_E_ARG = -1,     /* bad argument / shape mismatch */
  MTX_E_HIP = -2,     /* HIP runtime error */
  MTX_E_NOSCENE = -3, /* no scene uploaded */
  MTX_E_OOM = -4,     /* device allocation failed */
  MTX_E_UNSUPPORTED = -5
};

/* ------------------------------------------------------------------ */
/* Scene layout (SoA records copied to HBM as-is by mtx_scene_upload). */
/* ------------------------------------------------------------------ */

/* Material types: the 8 BSDF plugins of data/bedroom/scene.xml:26-219. */
enum {
  MTX_MAT_DIFFUSE = 1,         /* diffuse (rgb or bitmap reflectance) */
  MTX_MAT_ROUGHPLASTIC = 2,    /* roughplastic (ggx/beckmann, nonlinear) */
  MTX_MAT_CONDUCTOR = 3,       /* conductor (smooth) */
  MTX_MAT_ROUGHCONDUCTOR = 4,  /* roughconductor (ggx/beckmann) */
  MTX_MAT_DIELECTRIC = 5,      /* dielectric (smooth) */
  MTX_MAT_ROUGHDIELECTRIC = 6  /* roughdielectric */
};
/* Material flags. A `mask` BSDF is its nested BSDF + MTX_MF_MASK + opacity;
 * a `twosided` wrapper is MTX_MF_TWOSIDED on the nested BSDF. */
enum {
  MTX_MF_TWOSIDED = 1,
  MTX_MF_MASK = 2,
  MTX_MF_BECKMANN = 4, /* microfacet distribution: 0 = ggx */
  MTX_MF_NONLINEAR = 8
};

#define MTX_ROUGH_TRANSMITTANCE_RES 64

typedef struct mtx_material {
  uint32_t type;
  uint32_t flags;
  int32_t tex;           /* bitmap texture index for (diffuse_)reflectance, -1 = use rgb */
  float opacity;         /* mask opacity */
  float rgb[3];          /* reflectance | diffuse_reflectance | specular_reflectance */
  float alpha;           /* microfacet roughness */
  float eta;             /* int_ior / ext_ior (dielectric, roughdielectric, roughplastic) */
  float eta_rgb[3];      /* conductor eta (real part) */
  float k_rgb[3];        /* conductor k (imaginary part) */
  float spec_weight;     /* roughplastic specular sampling weight */
  float internal_refl;   /* roughplastic internal reflectance */
  int32_t table;         /* roughplastic: offset (floats) of its 64-entry external transmittance table */
} mtx_material;

typedef struct mtx_texture {
  uint32_t width, height;
  uint64_t offset; /* offset (in floats) into texels[], RGB interleaved, linear */
} mtx_texture;

/* Area emitter on a shape: an analytic `rectangle` (scene.xml:706-731) or a
 * triangle mesh (`obj`, `cube`). Both forms share the 64-B record; the first
 * nine words are a union.
 *
 * Rectangle: center / col0 / col1 describe the affine unit square, `normal`
 * is unit length.
 *
 * Mesh: `normal` is (0, 0, 0) -- that is what marks the record -- and the
 * union holds the discrete distribution over the shape's triangles (Mitsuba's
 * DiscreteDistribution, mtx_core/discrete.h), whose arrays lie in the scene's
 * float `tables` from `mesh_offset` on (after the roughplastic tables):
 *   pmf[mesh_count]   fp32 triangle areas
 *   cdf[mesh_count]   inclusive prefix, accumulated in double, stored as float
 *   prim[mesh_count]  scene (closest-hit leaf-order) triangle of each entry,
 *                     uint32 bit patterns
 * mesh_valid_lo / _hi are the first / last entry with a non-zero pmf,
 * mesh_sum = cdf[mesh_count - 1], mesh_norm = 1 / mesh_sum, mesh_kind =
 * MTX_EMITTER_MESH, inv_area = 1 / (sum of the triangle areas). The shape
 * that carries a mesh emitter is shaded with face normals (flag bit 0).
 * mtx_scene_update_vertices rebuilds pmf, cdf and the five words valid_lo,
 * valid_hi, sum, norm and inv_area from moved vertices; offset, count, kind,
 * radiance and the prim block stay.
 * mtx_scene_upload refuses (MTX_E_ARG) a mesh record whose table range leaves
 * `tables`, whose entries are not exactly the triangles of the shapes that
 * name the emitter, whose cdf decreases, or whose sum is not positive. */
#define MTX_EMITTER_MESH 1u
typedef struct mtx_emitter {
  union {
    struct {
      float center[3];  /* to_world translation */
      float col0[3];    /* to_world * (1,0,0) */
      float col1[3];    /* to_world * (0,1,0) */
    };
    struct {
      uint32_t mesh_offset;   /* first float of pmf | cdf | prim in tables[] */
      uint32_t mesh_count;    /* entries (triangles) */
      uint32_t mesh_valid_lo; /* first entry with pmf > 0 */
      uint32_t mesh_valid_hi; /* last entry with pmf > 0 */
      float mesh_sum;         /* cdf[mesh_count - 1] */
      float mesh_norm;        /* 1 / mesh_sum */
      uint32_t mesh_kind;     /* MTX_EMITTER_MESH */
      uint32_t mesh_pad[2];   /* 0 */
    };
  };
  float normal[3];  /* rectangle: normalize(inverse-transpose(to_world) * (0,0,1)); mesh: 0 */
  float inv_area;   /* rectangle: 1 / |cross(2 col0, 2 col1)|; mesh: 1 / total triangle area */
  float radiance[3];
} mtx_emitter;

typedef struct mtx_shape {
  uint32_t material;
  int32_t emitter; /* -1 if not an emitter */
  uint32_t flags;  /* bit0: face_normals / no vertex normals, bit1: has uv */
  uint32_t pad;
} mtx_shape;

/* Perspective sensor (scene.xml:10-25). */
typedef struct mtx_camera {
  float origin[3];  /* to_world translation */
  float axis_x[3];  /* to_world columns */
  float axis_y[3];
  float axis_z[3];
  float tan_x, tan_y; /* tan(fov_x/2), tan(fov_x/2) / aspect */
  float near_clip, far_clip;
  uint32_t width, height;
  float inv_rows[9];  /* rows of inverse([axis_x axis_y axis_z]) (world -> camera) */
  uint32_t pad;
} mtx_camera;

/* A scene carries two BVHs over the same triangles (round 4: each is the
 * faster form for its query):
 *
 * Closest-hit BVH node (64 B, Scene.ray_intersect): up to 4 children with
 * 8-bit quantised boxes, collapsed from a binned-SAH BVH2 by dynamic
 * programming over the 4-wide tree's SAH (bvh_build.cpp); visited near child
 * first (the traversal sorts the four entry distances). Breadth-first, the
 * inner children of a node consecutive and first in slot order, then its
 * leaves, whose triangle ranges are consecutive. Words:
 *   f[0..2] = origin.xyz (fp32);  w[3] = bytes [ex, ey, ez, n_children],
 *             e* int8 in [-32, 31]: axis scale 2^e
 *   i[4..7] = child refs: >= 0 inner node index,
 *             < 0 leaf: ~c = (first_tri << 3) | (count - 1)
 *   w[8..13] = q_lo.x, q_hi.x, q_lo.y, q_hi.y, q_lo.z, q_hi.z: one byte per
 *             child (child k in bits 8k..8k+7); bound = origin + q * 2^e in
 *             fp32, conservative (contains the child's padded box)
 *   w[14], w[15] = 0
 * Its leaf order is THE triangle order of the scene (tri_geom, tri_vidx,
 * tri_shape, hit records' prim). Triangles are 12 floats (48 B):
 *   v0.xyz, 0, e1 = v1-v0 .xyz, 0, e2 = v2-v0 .xyz, 0 */
#define MTX_BVH_WIDTH 4
#define MTX_BVH_MAX_LEAF 8
#define MTX_BVH_NODE_WORDS 16
#define MTX_BVH_MAX_DEPTH 40

/* Occlusion BVH node (80 B, Scene.ray_test: any hit; a compressed 8-wide
 * node after Ylitie, Karras & Laine 2017), built over the closest-hit
 * tree's triangle records (mtx_bvh_build_occlusion) with its own leaf order
 * and its own copy of the records (occ_tri_geom): up to 8 children with
 * 8-bit quantised boxes, collapsed from a binned-SAH BVH2 by dynamic
 * programming over the 8-wide tree's SAH. The children sit in slots chosen
 * so that visiting slot s at position s ^ octant(ray) (octant bit a set when
 * the direction's component a is negative) is approximately front to back:
 * no per-visit sort. Breadth-first; a node's inner children are consecutive
 * from child_base in slot order, its leaves' triangles consecutive from
 * tri_base in slot order. Words:
 *   f[0..2]  origin.xyz (fp32)
 *   w[3]     bytes [ex, ey, ez, imask]: int8 axis exponents in [-32, 31]
 *            (axis scale 2^e); imask bit s set: slot s holds an inner node
 *   w[4]     child_base: node index of the first inner child; the inner
 *            child in slot s is child_base + popcount(imask & ((1 << s) - 1))
 *   w[5]     tri_base: first triangle (occlusion leaf order) of the leaves
 *   w[6..7]  meta, one byte per slot (slot s in byte s of the 8):
 *              0 = empty; inner: 0x20 | (24 + s);
 *              leaf of n = 1..3 triangles: ((1 << n) - 1) << 5 | offset,
 *              its triangles tri_base + offset .. + n - 1 (offset + n <= 24)
 *   w[8..19] q_lo.x, q_hi.x, q_lo.y, q_hi.y, q_lo.z, q_hi.z: 8 bytes each
 *            (two words, slot s in byte s); bound = origin + q * 2^e in
 *            fp32, conservative (contains the child's padded box); empty
 *            slots hold q_lo 255, q_hi 0 */
#define MTX_OCC_WIDTH 8
#define MTX_OCC_MAX_LEAF 3
#define MTX_OCC_NODE_WORDS 20

typedef struct mtx_scene_desc {
  uint32_t n_tris, n_nodes, n_verts, n_shapes;
  uint32_t n_materials, n_emitters, n_textures, flags;
  const int32_t *nodes;      /* closest-hit BVH: MTX_BVH_NODE_WORDS (16) words per node */
  const float *tri_geom;     /* 12 floats per triangle (leaf order) */
  const uint32_t *tri_vidx;  /* 3 vertex indices per triangle (leaf order) */
  const uint32_t *tri_shape; /* shape index per triangle (leaf order) */
  const float *vpos;         /* 3 per vertex */
  const float *vnormal;      /* 3 per vertex, may be NULL */
  const float *vuv;          /* 2 per vertex, may be NULL */
  const mtx_shape *shapes;
  const mtx_material *materials;
  const mtx_emitter *emitters;
  const mtx_texture *textures;
  const float *texels;
  uint64_t n_texels;         /* floats */
  const float *tables;       /* roughplastic transmittance tables, then mesh emitters' pmf | cdf | prim */
  uint32_t n_tables;         /* floats */
  uint32_t pad0;
  mtx_camera camera;
  /* occlusion BVH (MTX_OCC_NODE_WORDS words per node) and its triangle
   * records (12 floats each, its leaf order): both NULL = mtx_scene_upload
   * builds them (mtx_bvh_build_occlusion over tri_geom) */
  const int32_t *occ_nodes;
  const float *occ_tri_geom;
  uint32_t n_occ_nodes, pad1;
  /* scene triangle (closest-hit leaf order) of each occlusion leaf-order
   * triangle (mtx_bvh_build_occlusion's perm). Given with occ_nodes /
   * occ_tri_geom: mtx_scene_upload checks occ_tri_geom[i] ==
   * tri_geom[occ_perm[i]] for every i and that it is a permutation; NULL
   * with given trees: derived at upload by matching the records, and the
   * trees rejected (MTX_E_ARG) unless occ_tri_geom is a permutation of
   * tri_geom. */
  const uint32_t *occ_perm;
  /* constant environment emitter (Mitsuba `constant`, the scene.environment()
   * of path-mis.py:41 / pssmltpath.py:39 / restirgi.py:475; mtx_core/interaction.h):
   * has_env != 0 adds it as emitter index n_emitters, picked uniformly with the
   * area emitters; its bounding sphere is that of the vertices' box. With
   * has_env, n_emitters may be 0. (ABI 8) */
  float env_radiance[3];
  uint32_t has_env;
} mtx_scene_desc;

/* Integrators (the reference scripts whose sample() loop is replaced). */
enum {
  MTX_INT_PATH = 1,          /* path.py:194-302 ("mypath") */
  MTX_INT_PATH_MIS = 2,      /* path-mis.py:24-155 ("path_test") */
  MTX_INT_NRC = 3,           /* nrc.py:25-125 */
  MTX_INT_PSSMLT_SIMPLE = 4, /* pssmlt.py:167-228 + pssmltsimple.py:16-142 */
  MTX_INT_RESTIR_GI = 5,     /* restirgi.py:182-588 */
  MTX_INT_PSSMLT_PATH = 6,   /* pssmlt.py:167-228 + pssmltpath.py:17-190 ("pssmlt") */
  MTX_INT_NERAD_RHS = 7,     /* nerad.py:174-233 Integrator.sample_rhs (internal: mtx_nerad_*) */
  MTX_INT_NERAD = 8,         /* nerad.py:235-254 Integrator.sample: next_smooth_si + the uploaded field
                                (max_depth = 11: first hit + up to 10 delta bounces) */
  MTX_INT_SIMPLE = 9         /* simple.py:14-116 ("integrator"): BSDF sampling only, no NEE */
};

typedef struct mtx_render_args {
  uint32_t integrator;
  uint32_t max_depth;
  uint32_t rr_depth;
  uint32_t seed;
  uint32_t spp;          /* samples traced per pixel by this call */
  uint32_t spp_total;    /* samples per pixel of the whole job (lane stride) */
  uint32_t sample_offset;/* first global sample index of this call (rank shard) */
  uint32_t y0, y1;       /* film rows [y0, y1) traced by this call */
  uint32_t chunk_paths;  /* wavefront size (0 = default) */
  float nrc_c;           /* NRC spread threshold (nrc.py:123) */
  uint32_t flags;        /* bit0: collect traversal stats, bit1: per-kernel HIP event timing,
                            bit2 (NRC): query the uploaded radiance field where the spread
                            criterion ends a segment (NRC radiance cache) */
  uint32_t iterations;   /* PSSMLT Metropolis iterations (pssmlt.py:208: 200; 0 = 200) */
  uint32_t frame;        /* ReSTIR GI frame index (restirgi.py self.n); 0 resets the reservoirs */
  /* ReSTIR GI properties (restirgi.py:157-166) */
  uint32_t restir_flags; /* bit0 bias_correction, bit1 jacobian, bit2 bsdf_sampling, bit3 spatial_spatial_reuse */
  uint32_t max_M_temporal; /* 0 = None */
  uint32_t max_M_spatial;  /* 0 = None */
  float initial_search_radius;
  float minimal_search_radius;
  uint32_t rfilter;      /* MTX_RFILTER_*: the film's reconstruction filter (mtx_render only; 0 = tent,
                            so callers that zeroed the former `reserved` word are unchanged) */
} mtx_render_args;

/* Reconstruction filters of the film (mtx_core/film.h; Mitsuba's `tent`,
 * `box` and `gaussian` rfilter plugins). border = the filter's reach in
 * pixels = the border of the raw film on every side. */
#ifndef MTX_RFILTER_TENT
#define MTX_RFILTER_TENT 0u     /* radius 1,   border 1: max(0, 1 - |r|) */
#define MTX_RFILTER_BOX 1u      /* radius 0.5, border 0: the sample goes to its own pixel with weight 1 */
#define MTX_RFILTER_GAUSSIAN 2u /* radius 2,   border 2: stddev 0.5, max(0, exp(-2 r^2) - exp(-8)) */
#endif

enum {
  MTX_RESTIR_BIAS_CORRECTION = 1,
  MTX_RESTIR_JACOBIAN = 2,
  MTX_RESTIR_BSDF_SAMPLING = 4,
  MTX_RESTIR_SPATIAL_SPATIAL = 8,
  /* row-banded frames (multi-GPU): stage A = sample_initial + temporal
   * resampling of rows [y0,y1); stage B = spatial resampling + render_final +
   * film of the same rows. Between them the caller imports the neighbours'
   * halo rows (mtx_restir_rows). Neither flag: the whole frame in one call. */
  MTX_RESTIR_STAGE_A = 16,
  MTX_RESTIR_STAGE_B = 32
};

/* Device-side counters, filled when mtx_render_args.flags has bit0/bit1. */
typedef struct mtx_stats {
  uint64_t rays_closest, rays_shadow;
  uint64_t nodes_closest, tris_closest; /* node / triangle visits */
  uint64_t nodes_shadow, tris_shadow;
  uint64_t trace_launches;              /* closest-hit traversal launches */
  uint64_t shadow_launches;
  double trace_ms, shadow_ms, shade_ms, other_ms; /* HIP-event time, summed */
  uint64_t paths;
  /* closest-hit traversal wave iterations (node phase, leaf phase): SIMD
   * utilisation = visits / (64 * iterations) */
  uint64_t wave_node_iters, wave_leaf_iters;
  /* NRC radiance cache (MTX_RENDER_NRC_CACHE): queries answered, HIP-event
   * time of the feature encoder and of the fused MLP (part of other_ms's
   * complement: other_ms excludes them) */
  uint64_t cache_queries;
  double cache_encode_ms, cache_mlp_ms;
  /* wavefronts / HIP streams the render ran on: > 1 means the per-kernel
   * times above are summed over overlapping launches (wall time is other_ms
   * + the kernels only for a one-stream render) */
  uint32_t streams, reserved;
} mtx_stats;

/* --------------------------- context ------------------------------ */
int mtx_abi_version(void);
const char *mtx_last_error(void);
typedef struct mtx_ctx mtx_ctx;
/* One context per HIP device; owns every device allocation. */
int mtx_ctx_create(int hip_device, mtx_ctx **out);
void mtx_ctx_destroy(mtx_ctx *ctx);

/* --------------------------- scene -------------------------------- */
/* Host-only BVH build over an indexed triangle mesh (replaces the Embree /
 * OptiX acceleration-structure build behind mi.load_file, upstream): binned-
 * SAH BVH2, collapsed to the 4-wide closest-hit node above.
 * nodes_out: capacity (n_tris + 1) * MTX_BVH_NODE_WORDS words; tri_geom_out:
 * 12*n_tris floats; perm_out: n_tris (leaf order -> input triangle index);
 * depth_out: levels of the 4-wide tree (the traversal stack's bound). */
int mtx_bvh_build(const float *vpos, uint32_t n_verts, const uint32_t *tri_vidx, uint32_t n_tris,
                  int32_t *nodes_out, uint32_t *n_nodes_out, float *tri_geom_out, uint32_t *perm_out,
                  uint32_t *depth_out);
/* Host-only occlusion BVH (8-wide node above) over n_tris triangle records
 * (12 floats each, e.g. mtx_bvh_build's tri_geom_out). nodes_out: capacity
 * (n_tris + 1) * MTX_OCC_NODE_WORDS words; tri_geom_out: the same records
 * (bit-identical) in the occlusion tree's leaf order; perm_out (may be NULL):
 * occlusion leaf order -> input record; depth_out: levels of the tree. */
int mtx_bvh_build_occlusion(const float *tri_geom, uint32_t n_tris, int32_t *nodes_out, uint32_t *n_nodes_out,
                            float *tri_geom_out, uint32_t *perm_out, uint32_t *depth_out);
/* Host-only refit of the closest-hit tree after a vertex update (the host
 * half of assigning vertex_positions and calling params.update() on
 * mi.traverse of a scene): topology, leaf order and slot order stay; origins,
 * exponents and the 8-bit child bounds of `nodes` (n_nodes nodes, in place)
 * are recomputed bottom-up from the new vertices exactly as the builder
 * computes them, so unchanged vertices give back the builder's nodes bit for
 * bit. tri_vidx is in leaf order (the scene's); tri_geom_out: 12*n_tris
 * floats, the new records. A non-finite coordinate, or one of magnitude above
 * 2^37 (the bound under which quantisation with exponents <= 31 provably
 * succeeds, mtx_core/geometry.h), is MTX_E_ARG and nothing is written. */
int mtx_bvh_refit(const float *vpos, uint32_t n_verts, const uint32_t *tri_vidx, uint32_t n_tris,
                  int32_t *nodes, uint32_t n_nodes, float *tri_geom_out);
/* The same for the occlusion tree: tri_geom are the new records in scene
 * order, occ_perm the scene triangle of each occlusion leaf-order triangle;
 * occ_tri_geom_out: the records copied bit for bit through occ_perm. */
int mtx_bvh_refit_occlusion(const float *tri_geom, const uint32_t *occ_perm, uint32_t n_tris,
                            int32_t *occ_nodes, uint32_t n_occ_nodes, float *occ_tri_geom_out);
/* Host-only roughplastic precompute (upstream roughplastic constructor):
 * external transmittance table (64 floats) and internal reflectance. */
int mtx_roughplastic_tables(uint32_t distribution, float alpha, float eta, float *table_out,
                            float *internal_refl_out);
/* Copy a scene to HBM (replaces mi.load_file / mi.load_dict scene
 * construction, path.py:308-309, restirgi.py:599). */
int mtx_scene_upload(mtx_ctx *ctx, const mtx_scene_desc *scene);
/* New vertex positions for the uploaded scene, without a re-upload: the
 * device half of assigning vertex_positions and calling params.update() on
 * mi.traverse of a scene (test-restir-dynamic.py does the same for the sensor;
 * see mtx_set_camera). vpos: 3*n_verts floats, n_verts as uploaded; vnormal:
 * 3*n_verts floats or NULL (the normals are kept); on_device != 0: both are
 * device memory of the context's device (the caller orders their producer
 * before the call), else host memory. Topology, leaf order and slot order
 * stay: the 36-byte triangle records of both trees, the position (and
 * normal) rows of the shading records, vpos / vnormal, both trees' quantised
 * child boxes and the environment's bounding sphere are rewritten in place on
 * the context's stream, complete on return, and equal what mtx_bvh_refit /
 * mtx_bvh_refit_occlusion and a fresh upload would give, bit for bit. Device
 * pointers of the scene do not move.
 *   Mesh emitters move with their vertices. For each one, in `tables`:
 * pmf[k] becomes the fp32 area of entry k's triangle at the new positions
 * (mtx_core/discrete.h tri_area, mtx_tri_area_f32), cdf[k] the inclusive
 * prefix accumulated sequentially in double, in entry order, and stored as
 * float; the prim block stays. In the record mesh_valid_lo / _hi become the
 * first / last entry with pmf > 0, mesh_sum = cdf[n - 1], mesh_norm = inv_area
 * = 1.f / mesh_sum (one fp32 division); the other words stay. So unchanged
 * vertices give back the uploaded tables, and the result equals a fresh upload
 * of the scene a loader builds from the new vertices in this leaf order, bit
 * for bit. The device scans in parallel only where the order provably cannot
 * matter: with M = ilogb(largest area), m = max(ilogb(smallest non-zero
 * area), -126) - 23 and n entries, M + 1 + ceil(log2 n) - m <= 53 makes every
 * partial sum of every subset a double, so no addition rounds
 * (prefix_order_free); an emitter that fails this is summed by one lane in
 * entry order (slow, exact).
 *   A read-only pre-pass refuses (MTX_E_ARG, scene untouched) a wrong vertex
 * count, a non-finite coordinate or one of magnitude above 2^37, a mesh
 * emitter whose triangles have no finite positive total area at the new
 * positions (all collapsed, or an area that overflows fp32; the message names
 * the emitter), and any change to a triangle of a rectangle-emitter shape: a
 * rectangle emitter is an analytic record derived from to_world, not from its
 * vertices, and four moved vertices cannot give back the loader's bits, so
 * moving its triangles would split emitter sampling from traversal. Neural-radiosity
 * surface tables are dropped as by an upload. ReSTIR GI reservoirs are kept:
 * the reference has no reprojection under moving geometry either, so a caller
 * restarts with frame = 0 or accepts stale reuse. Should a refit pass fail
 * after the pre-pass, the scene is dropped (MTX_E_NOSCENE until the next
 * upload) and an error returned: no half-refit tree stays live. */
int mtx_scene_update_vertices(mtx_ctx *ctx, const float *vpos, const float *vnormal, uint32_t n_verts,
                              int on_device);
/* Read back one device array of the uploaded scene (test / debugging hook):
 * which = 0 nodes, 1 occ_nodes (the ABI's words), 2 the closest-hit tree's
 * triangles and 3 the occlusion tree's (9 floats each: v0, e1, e2), 4 the
 * shading records (32 floats per triangle), 5 vpos, 6 vnormal, 7 the
 * environment's bounding sphere (centre.xyz, radius), 8 the float `tables`
 * (n_tables floats), 9 the emitter records (64 bytes each). n_bytes must
 * match. */
int mtx_scene_read(mtx_ctx *ctx, int which, void *out, uint64_t n_bytes);
/* area_out[i] = the fp32 area of triangle i of tris (9 floats each: p0, p1,
 * p2), in the arithmetic of a mesh emitter's pmf (mtx_core/discrete.h
 * tri_area): what mtx_scene_update_vertices computes on the device. Host. */
int mtx_tri_area_f32(const float *tris, uint64_t n, float *area_out);

/* --------------------------- integrators -------------------------- */
/* Render film rows [y0,y1) plus the border b of args->rfilter into
 * film_rgbw, an (y1-y0+2b) x (width+2b) x 4 float buffer (host pointer, or a
 * device pointer when film_on_device != 0): un-normalised RGB*weight and
 * weight sums in a fixed summation order. Film shape per filter:
 *   MTX_RFILTER_TENT (0, the default)  b = 1  (y1-y0+2) x (width+2) x 4
 *   MTX_RFILTER_BOX                    b = 0  (y1-y0)   x  width    x 4
 *   MTX_RFILTER_GAUSSIAN               b = 2  (y1-y0+4) x (width+4) x 4
 * An unknown filter id is MTX_E_ARG and nothing is rendered. Replaces mi.render(scene, integrator, spp, seed)
 * driving SamplingIntegrator::render (transcribed path.py:103-192) with the
 * sample() of path.py:194-302 / path-mis.py:24-155 / nrc.py:104-125,
 * Pssmlt.render (pssmlt.py:167-228), and one RestirIntegrator.render frame
 * (restirgi.py:182-258; whole film only, y0 = 0, y1 = height, spp_total =
 * spp; args.frame = 0 resets the reservoirs kept in ctx, later frames reuse
 * them and the camera of the previous frame as prev_sensor). */
int mtx_render(mtx_ctx *ctx, const mtx_render_args *args, float *film_rgbw, int film_on_device,
               mtx_stats *stats);

/* Replace the sensor of the uploaded scene (mi.traverse(sensor).update,
 * test-restir-dynamic.py; restirgi.py:247 keeps the old one as prev_sensor
 * for the next ReSTIR frame). The film size must not change. */
int mtx_set_camera(mtx_ctx *ctx, const mtx_camera *camera);

/* Copy rows [row0, row0+nrows) of the ReSTIR GI state to (to_state = 0) or
 * from (to_state = 1) a device buffer, plane-major (planes x rows x W*spp
 * float4): which = 0 the current frame's samples (5 planes), 1 the temporal
 * reservoirs (6 planes), 2 the previous frame's samples (5 planes; between
 * frames only: the buffer temporal resampling reprojects into,
 * restirgi.py:374-383). The halo exchange of a row-banded frame
 * (restirgi.py:301-313 reads up to search_radius rows away; a
 * moving camera reprojects arbitrarily far, so a banded caller gathers the
 * whole previous-sample buffer with which = 2 before stage A). */
int mtx_restir_rows(mtx_ctx *ctx, int which, uint32_t row0, uint32_t nrows, void *buf, int to_state);

/* Read back ReSTIR GI frame state (test / debugging hook for restirgi.py's
 * self.sample, temporal_reservoir, spatial_reservoir, search_radius):
 * which = 0 samples (5 float4 planes), 1 temporal reservoirs (6 planes),
 * 2 spatial reservoirs (6 planes), 3 search radius (1 float per lane);
 * layout in include/mtx_core/restir.h. n_floats must match exactly. */
int mtx_restir_state(mtx_ctx *ctx, int which, float *out, uint64_t n_floats);

/* Evaluate the integrator's sample() for n given rays (replaces
 * SamplingIntegrator.sample(scene, sampler, ray), path-mis.py:24-31).
 * rays: 6n floats (o.xyz, d.xyz); lanes: n sampler lane ids; each lane's
 * PCG32 stream is seeded with (seed, lane) and advanced by rng_skip draws
 * before the first bounce (the render loop consumes 2 for the film jitter).
 * Outputs: L (3n floats), valid (n bytes). Host pointers. */
int mtx_sample_rays(mtx_ctx *ctx, const mtx_render_args *args, uint64_t n, const float *rays,
                    const uint32_t *lanes, uint32_t rng_skip, float *L, uint8_t *valid);

/* Device-pointer forms (SURVEY §8b mtx_device_ptrs): the reference calls
 * sample(), ray_intersect and its primitives on wavefront-wide Dr.Jit arrays
 * that live on the GPU (path.py:194-202, prefix_sum.py:9-36,
 * hashgrid.py:16-84, reductions.py:12-54). The *_dev functions take buffers
 * in the context's device memory (hipMalloc'd; e.g. a torch CUDA tensor's
 * data_ptr), with the layouts of their host twins, and copy nothing through
 * the host: no staging copy, results written in place. Work runs on the
 * context's stream and is complete on return (the caller orders its own
 * producer of the inputs before the call). A host pointer is refused
 * (MTX_E_ARG); device indices are range-checked on the device. */
int mtx_sample_rays_dev(mtx_ctx *ctx, const mtx_render_args *args, uint64_t n, const float *rays,
                        const uint32_t *lanes, uint32_t rng_skip, float *L, uint8_t *valid);

/* Raw closest-hit / any-hit traversal (Scene.ray_intersect / ray_test,
 * path-mis.py:69-71, restirgi.py:320). rays: 8n floats (o.xyz, tmax, d.xyz,
 * 0); any_hit: 0 closest hit (4-wide tree), 1 any hit (8-wide occlusion
 * tree); hits: 4n words
 * (t, prim, u, v) for closest hit, or n words (1 = occluded) for any hit.
 * visits (optional, 2n u32): node and triangle visits.
 * The direction need not be normalised (t is in units of |d|), but its
 * largest component magnitude must lie in [2^-40, 2^60]: the slab tests
 * replace components below 1e-20 by +-1e-20 (mtx_core/geometry.h
 * make_trace_ray), which tilts a shorter direction by more than the child
 * boxes' padding absorbs, and the tree then culls triangles the ray meets
 * (seen from 2^-50 down on a scene of extent 4; brute force over the
 * triangles is unaffected). Smaller components beside a largest one in range
 * are fine, zero and -0 included. d = (0, 0, 0) is allowed and misses.
 * Non-finite rays are outside the contract (the CPU restatement terminates
 * and misses on them). Pinned at both ends of the range by
 * tests/test_lattice.py and tests/test_lattice_gpu.py (class c). */
int mtx_trace(mtx_ctx *ctx, uint64_t n, const float *rays, int any_hit, uint32_t *hits,
              uint32_t *visits);
/* mtx_trace on device buffers (Scene.ray_intersect on a device wavefront). */
int mtx_trace_dev(mtx_ctx *ctx, uint64_t n, const float *rays, int any_hit, uint32_t *hits,
                  uint32_t *visits);

/* --------------------------- building blocks ---------------------- */
/* The calls the reference's integrators are composed of (path-mis.py:69-121,
 * simple.py:57-114), one wavefront-wide kernel each, for estimators written
 * in Python on device tensors (mtx.blocks; INTEGRATION.md "Writing an
 * integrator on the blocks"). Every buffer is device memory of the context's
 * device in the facade's Dr.Jit layout: a quantity of C components over n
 * items is one contiguous (C, n) array, component c of item i at [c * n + i];
 * masks are n bytes (0 = off). A host pointer is refused (MTX_E_ARG). Work
 * runs on the context's stream and is complete on return; the caller orders
 * its own producers before the call. There are no host twins (one exception:
 * mtx_blocks_light_host below, the CPU reference of the two light-path
 * entries, which the oracle does not cover). n = 0 returns at once; n < 2^31.
 *   Indices that arrive in caller tensors (material, emitter, prim) are
 * compared against the scene's counts on the device before any load that
 * depends on them: one out of range is treated as invalid (null BSDF, no
 * emitter, a miss), the outputs are complete, and the call returns MTX_E_ARG
 * with the number of such lanes in the message.
 *   `active` may be NULL (all lanes). A masked-off lane writes the zero /
 * invalid values and is never traced. */

/* Surface interaction planes (SurfaceInteraction3f as the reference's loops
 * use it). The shading frame is not stored: every consumer rebuilds it from
 * sh_n (mtx_core/warp.h frame_from_normal, a function of the normal alone). */
typedef struct mtx_si_planes {
  float *p, *n, *sh_n;   /* (3, n) position, geometric and shading normal */
  float *uv;             /* (2, n) */
  float *wi;             /* (3, n) incident direction, local frame */
  float *t;              /* (n) ray distance, inf for an invalid interaction */
  uint32_t *prim;        /* (n) leaf-order triangle, 0xffffffff = none */
  int32_t *material;     /* (n) -1 for an invalid interaction */
  int32_t *emitter;      /* (n) -1 = none; a miss under an environment: n_emitters */
  float *bary;           /* (2, n) barycentrics of the hit record (u, v); may be NULL */
} mtx_si_planes;

/* DirectionSample3f planes of emitter sampling. */
typedef struct mtx_ds_planes {
  float *p, *n, *d;      /* (3, n) */
  float *dist, *pdf;     /* (n) */
  int32_t *emitter;      /* (n) */
} mtx_ds_planes;

/* Outputs of bsdf.eval_pdf_sample. */
typedef struct mtx_bsdf_planes {
  float *value;          /* (3, n) eval at wo */
  float *pdf;            /* (n) pdf at wo */
  float *s_wo;           /* (3, n) sampled direction, local */
  float *s_pdf, *s_eta;  /* (n) */
  uint32_t *s_type;      /* (n) sampled component's BSDFFlags */
  float *weight;         /* (3, n) sample weight */
} mtx_bsdf_planes;

/* sampler.seed (IndependentSampler over the given lane ids, restirgi.py:203):
 * state[i] = the PCG32 of (seed, lanes[i]) advanced by skip draws, two 64-bit
 * words per lane (state, sequence id). Needs no scene. */
int mtx_blocks_sampler_seed_dev(mtx_ctx *ctx, uint64_t n, uint32_t seed, const uint32_t *lanes, uint32_t skip,
                                uint64_t *state);
/* sampler.next_1d (dims = 1: out is (n)) / next_2d (dims = 2: out is (2, n))
 * (path-mis.py:97,104-105,147). Advances the state of every lane in place. */
int mtx_blocks_sampler_next_dev(mtx_ctx *ctx, uint64_t n, uint64_t *state, int dims, float *out);
/* scene.ray_intersect (path-mis.py:69-71): closest-hit traversal of the rays
 * o, d (3, n) with maxt (n; NULL = the largest float) and the surface
 * interaction of each hit, in one launch. The direction contract of
 * mtx_trace applies: d need not be normalised, its largest component
 * magnitude must lie in [2^-40, 2^60], (0, 0, 0) misses, non-finite rays are
 * outside the contract. A miss is the invalid interaction with emitter =
 * n_emitters under an environment, else -1; a masked-off lane is invalid
 * with emitter = -1 and wi = -d. */
int mtx_blocks_ray_intersect_dev(mtx_ctx *ctx, uint64_t n, const float *o, const float *d, const float *maxt,
                                 const uint8_t *active, const mtx_si_planes *si);
/* scene.ray_test (restirgi.py:320): any-hit traversal, out[i] = 1 if
 * occluded within maxt (required). mtx_trace's direction contract applies.
 * Masked-off lanes give 0. */
int mtx_blocks_ray_test_dev(mtx_ctx *ctx, uint64_t n, const float *o, const float *d, const float *maxt,
                            const uint8_t *active, uint8_t *out);
/* The interaction half of scene.ray_intersect (path-mis.py:69-71) for hit
 * records the caller holds (mtx_trace_dev's t, prim, u, v; ray direction d): what
 * Mesh::compute_surface_interaction gives. prim = 0xffffffff is a miss. */
int mtx_blocks_interact_dev(mtx_ctx *ctx, uint64_t n, const float *d, const float *t, const uint32_t *prim,
                            const float *u, const float *v, const uint8_t *active, const mtx_si_planes *si);
/* si.spawn_ray(d) (to = 0, path-mis.py:121) / si.spawn_ray_to(target)
 * (to = 1) from p, n (3, n) and x = the direction or the target: o, d (3, n)
 * and maxt (n). Needs no scene. */
int mtx_blocks_spawn_dev(mtx_ctx *ctx, uint64_t n, const float *p, const float *nrm, const float *x, int to,
                         float *o, float *d, float *maxt);
/* scene.sample_emitter_direction(si, u, test_visibility) (path-mis.py:94-98)
 * from the reference point p, its geometric normal nrm (3, n; read only with
 * test_visibility) and u (2, n): ds and the weight (3, n). test_visibility
 * != 0 traces spawn_ray_to(p, nrm, ds.p) through the any-hit tree in the
 * same launch and zeroes the weight of an occluded sample. A scene without
 * emitters gives zeros. */
int mtx_blocks_sample_emitter_dev(mtx_ctx *ctx, uint64_t n, const float *p, const float *nrm, const float *u,
                                  const uint8_t *active, int test_visibility, const mtx_ds_planes *ds,
                                  float *weight);
/* scene.pdf_emitter_direction (path-mis.py:78) and emitter.eval
 * (path-mis.py:83) for the emitter index of each lane (-1 = none): pdf (n)
 * from the direction d (3, n) towards the emitter, its distance dist (n) and
 * the emitter-side normal nrm (3, n); le (3, n) from the local incident
 * direction wi (3, n). Either output group may be NULL with its inputs. */
int mtx_blocks_emitter_dev(mtx_ctx *ctx, uint64_t n, const int32_t *emitter, const float *d, const float *dist,
                           const float *nrm, const float *wi, const uint8_t *active, float *pdf, float *le);
/* bsdf.eval_pdf_sample (path-mis.py:104-109) of the material index of each
 * lane (< 0: the null BSDF, all zeros) at uv (2, n), wi and wo (3, n, local),
 * u1 (n), u2 (2, n); flags (n, may be NULL): bsdf.flags() of the lane's
 * material (path.py:245), 0 for the null BSDF. out = NULL with flags given
 * evaluates the flags alone (uv .. u2 are then not read). */
int mtx_blocks_bsdf_dev(mtx_ctx *ctx, uint64_t n, const int32_t *material, const float *uv, const float *wi,
                        const float *wo, const float *u1, const float *u2, const uint8_t *active,
                        const mtx_bsdf_planes *out, uint32_t *flags);
/* Exact elementwise arithmetic in the oracle's rounding (mtx_core/common.h,
 * warp.h, interaction.h): dr.fma and the operations whose rounding a tensor
 * library does not pin. n items; a, b, c as the op needs (else NULL):
 *   FMA  out = fmaf(a, b, c)          DIV  out = a / b
 *   RCP  out = 1 / a                  SQRT out = sqrtf(a)        (1 component)
 *   DOT3 out (n) = dot(a, b)          NORM3 out (n) = norm(a)
 *   NORMALIZE3 out (3, n)             (a, b of 3 components)
 *   TO_LOCAL / TO_WORLD out (3, n) = b in / out of the frame of the normal a
 *   MIS_A / MIS_B out (n) = the power heuristic of path.py:10-18 /
 *   path-mis.py:9-15 for the pdfs a, b. */
enum {
  MTX_MATH_FMA = 0, MTX_MATH_DIV = 1, MTX_MATH_RCP = 2, MTX_MATH_SQRT = 3, MTX_MATH_DOT3 = 4,
  MTX_MATH_NORM3 = 5, MTX_MATH_NORMALIZE3 = 6, MTX_MATH_TO_LOCAL = 7, MTX_MATH_TO_WORLD = 8,
  MTX_MATH_MIS_A = 9, MTX_MATH_MIS_B = 10
};
int mtx_blocks_math_dev(mtx_ctx *ctx, int op, uint64_t n, const float *a, const float *b, const float *c,
                        float *out);
/* sensor.sample_ray (path.py:45-62) of the context's bound camera for the
 * film positions pos (2, n) in pixels (pixel + jitter): o, d (3, n) =
 * camera_ray(cam, pos / size) with the fp32 division of the fixed
 * integrators' camera rays, and maxt (n; may be NULL) the ray's extent to the
 * far clip, which those integrators trace with. Positions outside the film
 * give the rays the formula gives. Masked-off lanes get zeros. */
int mtx_blocks_sensor_ray_dev(mtx_ctx *ctx, uint64_t n, const float *pos, const uint8_t *active, float *o, float *d,
                              float *maxt);
/* scene.sample_emitter_ray(time, sample1, u_pos, u_dir) (bdpt02.py:86-88):
 * the first ray of a light path, from u_pos, u_dir (2, n). u_pos.x picks the
 * emitter (the environment, if any, is index n_emitters) and is reused;
 * the position is the emitter's sample_position, the direction a cosine
 * hemisphere about its normal. o, d (3, n), maxt (n): spawn_ray(p, nrm, d) of
 * an area emitter, or the unoffset point of the scene's bounding sphere for
 * the environment. weight (3, n) = radiance * pi / pdf_pos * count (area),
 * radiance * 4 pi^2 r^2 * count (environment). p, nrm (3, n): the unoffset
 * position and the normal; emitter (n): the picked index. A scene without
 * emitters gives zeros and emitter = -1, as a masked-off lane does. */
int mtx_blocks_sample_emitter_ray_dev(mtx_ctx *ctx, uint64_t n, const float *u_pos, const float *u_dir,
                                      const uint8_t *active, float *o, float *d, float *maxt, float *weight, float *p,
                                      float *nrm, int32_t *emitter);
/* sensor.sample_direction(it, ..) of the context's bound camera: connects the
 * points p (3, n) to the pinhole. pos (2, n): the film position in pixels;
 * d (3, n), dist (n): the unit direction from p to the camera origin and the
 * distance; weight (n) = importance / dist^2 with importance = 1 / (4 tan_x
 * tan_y cos^3 theta), normalised over the image rectangle; valid (n bytes):
 * 0 outside the clip range or the frustum, where all outputs are zero.
 * test_visibility != 0 traces spawn_ray_to(p, nrm, origin) (nrm (3, n): the
 * geometric normal at p, read only then) through the any-hit tree in the same
 * launch and zeroes the weight of an occluded sample; valid is unchanged. */
int mtx_blocks_sensor_direction_dev(mtx_ctx *ctx, uint64_t n, const float *p, const float *nrm,
                                    const uint8_t *active, int test_visibility, float *pos, float *d, float *dist,
                                    float *weight, uint8_t *valid);
/* Host-only, needs no context (like mtx_bvh_build): the per-lane functions of
 * the two entries above, run on the CPU over a host scene description. The
 * one exception to "there are no host twins": the library's host code is
 * compiled with the kernels' floating-point flags, so these are the kernels'
 * bit-exact twins, and the reference the tests hold them to. in / out are
 * host (C, n) planes; integers are stored as bit patterns.
 *   MTX_LIGHT_EMITTER_RAY       in (4, n) = u_pos, u_dir; out (17, n) = o, d,
 *     maxt, weight, p, nrm, emitter (int32). Needs the emitters, the vertex
 *     and index arrays, shapes and tables of the description; no BVH.
 *   MTX_LIGHT_SENSOR_DIRECTION  in (3, n) = p; out (8, n) = pos, d, dist,
 *     weight, valid (uint32 0 / 1), without the visibility test. Reads
 *     desc->camera alone.
 *   MTX_LIGHT_PROJECT           in (3, n) = p; out (3, n) = the film position
 *     of the projection sample_direction shares with ReSTIR's reprojection
 *     (mtx_core/restir.h project_prev) and its validity (uint32 0 / 1). */
enum { MTX_LIGHT_EMITTER_RAY = 0, MTX_LIGHT_SENSOR_DIRECTION = 1, MTX_LIGHT_PROJECT = 2 };
int mtx_blocks_light_host(const mtx_scene_desc *desc, int op, uint64_t n, const float *in, float *out);
/* A vertex store: one subpath per lane, D = `depth` vertex slots, every plane
 * coalesced over lanes (vertex k, component c of lane i at [(k * C + c) * n + i]).
 * mtx_core/bdpt.h states what a camera and a light subpath keep in it. */
typedef struct mtx_path_planes {
  uint32_t depth;                      /* D = max vertices per subpath */
  const int32_t *len;                  /* (n)        vertices recorded for this lane, 0..D */
  const float *p, *n, *sh_n, *wi;      /* (D, 3, n)  position, geometric / shading normal, wi (local) */
  const float *uv;                     /* (D, 2, n) */
  const int32_t *material, *emitter;   /* (D, n)     -1 = none */
  const float *beta;                   /* (D, 3, n)  throughput with which the subpath arrives at the vertex */
  const float *pdf_fwd, *pdf_rev;      /* (D, n)     area-measure densities */
  const uint8_t *delta;                /* (D, n)     the lobe sampled AT this vertex was a delta / null lobe */
} mtx_path_planes;
/* Connect a camera subpath z_0 .. and a light subpath y_0 .. per lane
 * (mtx_core/bdpt.h has the conventions): strategy (s, t) joins y_{s-1} and
 * z_{t-1}, t >= 2; s = 0 is the camera subpath's own emitter hit. s = t = -1
 * sums every strategy with s + t - 1 <= max_depth into L (3, n); s, t >= 0
 * evaluates that one, and `weight` (n, may be NULL; refused with s = t = -1)
 * receives its weight. flags: MTX_BDPT_MIS weighs the strategies by the power
 * heuristic (exponent 2) over all strategies of the same path with t' >= 2,
 * else every weight is 1; MTX_BDPT_VISIBILITY traces the connection's shadow
 * ray spawn_ray_to(z.p, z.n, y.p) through the any-hit tree in the same lane,
 * only where the unoccluded contribution is non-zero. A strategy a lane's
 * subpaths are too short for, or one that touches a vertex without a smooth
 * lobe, gives 0 (and weight 0). Both stores have the same depth D, max_depth
 * >= 1, s <= D, 2 <= t <= D. A material or emitter index outside the scene's
 * tables is handled as none and reported (MTX_E_ARG) like the other blocks'.
 * Environment emitters are not connected (s = 0 at a miss gives 0). */
enum { MTX_BDPT_MIS = 1, MTX_BDPT_VISIBILITY = 2 };
int mtx_blocks_bdpt_connect_dev(mtx_ctx *ctx, uint64_t n, const mtx_path_planes *camera,
                                const mtx_path_planes *light, int s, int t, uint32_t max_depth,
                                uint32_t flags, const uint8_t *active,
                                float *L /* (3, n) */, float *weight /* (n), may be NULL */);
/* Host-only and context-free twin of the entry above (like
 * mtx_blocks_light_host): the same per-lane functions over host planes and a
 * host scene description, of which it reads the materials, emitters, textures
 * and tables. MTX_BDPT_VISIBILITY is refused: the library has no host
 * traversal. Indices outside the tables are handled as none, silently. */
int mtx_blocks_bdpt_host(const mtx_scene_desc *desc, uint64_t n, const mtx_path_planes *camera,
                         const mtx_path_planes *light, int s, int t, uint32_t max_depth,
                         uint32_t flags, float *L, float *weight);
/* ImageBlock.put (path.py:101): stage 1 of the film (DESIGN.md "Film") for
 * samples the caller holds. The film is the caller's: `planes` are the
 * contribution planes of the band of rows [y0, y1) of a film `width` wide,
 * 8 slots x K = (2b + 1)^2 taps x band pixels float4 ([slot][K][band_px]),
 * b = the filter's reach (mtx_rfilter_info); zeroed by the caller before the
 * first put. Needs no scene.
 *   A sample (pos (2, n), L (3, n)) belongs to the source pixel (floor(pos.x),
 * floor(pos.y)). It is dropped if its lane is off, its position is not
 * finite, or its source pixel lies outside [0, width) x [y0, y1); *dropped
 * (host, may be NULL) receives the number dropped for the last two reasons,
 * which is no error. Per source pixel the kept samples of the call are
 * ranked r = 0, 1, .. by ascending lane; sample r goes to slot
 * film_slot(sample_offset + r, T), T = spp_total, or the pixel's count in
 * this call when spp_total = 0. The pixel's accumulators are loaded from the
 * planes, updated in rank order by the operation sequence of the fixed
 * integrators' film kernels, and stored back: a put split into passes of
 * whole pixels, or into sample ranges with spp_total / sample_offset set,
 * leaves the same planes as the single put.
 *   pixel_major_spp = s > 0 declares the layout of a render loop: lane i
 * belongs to pixel px0 + i / s (pixels as y * width + x; n a multiple of s;
 * the pixels inside the band). The claim is checked on the device before any
 * plane is written: an active lane with a finite position must have its
 * position in that pixel, the upper edge included ((float)x + u rounds up to
 * x + 1 for u next to 1, and such a sample stays with the pixel that drew
 * it, as in the fixed integrators). Otherwise MTX_E_ARG with the number of
 * such lanes, and the planes are unchanged. Non-finite positions are dropped
 * and counted as above. Where both layouts describe the same samples
 * (floor(pos) is the claimed pixel for every kept lane) the planes are
 * identical. */
int mtx_blocks_film_put_dev(mtx_ctx *ctx, float *planes, uint32_t width, uint32_t y0, uint32_t y1, uint32_t rfilter,
                            uint64_t n, const float *pos, const float *L, const uint8_t *active, uint32_t spp_total,
                            uint32_t sample_offset, uint32_t pixel_major_spp, uint32_t px0, uint64_t *dropped);
/* Stage 2: the raw film (y1 - y0 + 2b) x (width + 2b) x RGBW (device) of the
 * planes: per slot the K neighbours of a film pixel in (dy, dx) order, then
 * the slots' fixed tree -- the layout and order of mtx_render's film. */
int mtx_blocks_film_gather_dev(mtx_ctx *ctx, const float *planes, uint32_t width, uint32_t y0, uint32_t y1,
                               uint32_t rfilter, float *film);
/* A built hash grid as a fixed-radius query reads it: the points p (3, n) it
 * was built over, their scalar bounds (minimum and maximum over all three
 * axes, as the build takes them), resolution and n_cells of the build, and
 * its cell_size, cell_offset (n_cells each) and sample_idx (n). All device
 * pointers. */
typedef struct mtx_hashgrid_view {
  const float *p;
  uint64_t n;
  float bbmin, bbmax;
  uint32_t resolution, n_cells;
  const uint32_t *cell_size, *cell_offset, *sample_idx;
} mtx_hashgrid_view;
/* A query whose cell box holds more cells than this does no walk and fails. */
#define MTX_HG_MAX_QUERY_CELLS 4096u
/* Photon gather: the fixed-radius query below (mtx_hashgrid_query_count_dev,
 * same walk, same order, same cap) over a grid whose samples are photons,
 * fused with the density estimate at m visible points. Photon j: the world
 * direction d (3, n) towards where it came from, its weight beta (3, n) and
 * the segments of its light path, depth (n). Visible point i: its position
 * p (3, m) is the query; material (m, < 0 = the null BSDF), uv (2, m), wi
 * (3, m, local), the shading and geometric normals sh_n, n (3, m) and the
 * segments of its camera path, depth (m). */
typedef struct mtx_photon_planes {
  const float *d, *beta;
  const int32_t *depth;
} mtx_photon_planes;
typedef struct mtx_visible_planes {
  const float *p;
  const int32_t *material;
  const float *uv, *wi, *sh_n, *n;
  const int32_t *depth;
} mtx_visible_planes;
/* Per neighbour of lane i, in walk order: skipped if depth_i + depth_j >
 * max_depth; wo = to_local(frame(sh_n), d_j); val = bsdf_eval_pdf(material,
 * uv, wi, wo), the function mtx_blocks_bsdf_dev evaluates (radiance mode,
 * f |wo.n_s|); cg = dot(n, d_j); skipped unless cg wo.z > 0 (the particle
 * tracer's light-leak mask for the photon's direction) and wi.z wo.z > 0 (the
 * photon arrived on the side the point is seen from); contrib = (val *
 * beta_j) / |cg| per component, one product and one correctly rounded
 * division; sum = sum + contrib from +0. out_sum (3, m), out_count (m): the
 * neighbours that contributed. Needs a scene. A material index past the
 * scene's materials is handled as the null BSDF and reported (MTX_E_ARG)
 * like mtx_blocks_bsdf_dev's; queries over the cell cap are reported like
 * the query's. */
int mtx_blocks_photon_gather_dev(mtx_ctx *ctx, const mtx_hashgrid_view *grid, const mtx_photon_planes *photons,
                                 const mtx_visible_planes *points, uint64_t m, const float *radius,
                                 uint32_t radius_stride, uint32_t max_depth, float *out_sum, uint32_t *out_count);

/* --------------------------- film filters ------------------------- */
/* Host-only: border (pixels on every side of the raw film) and radius of a
 * reconstruction filter; either output may be NULL. Unknown id: MTX_E_ARG. */
int mtx_rfilter_info(uint32_t rfilter, uint32_t *border_out, float *radius_out);
/* Host-only: the filter's one-axis weight (the function the film kernels
 * evaluate, mtx_core/film.h rfilter_eval) at n offsets r from a pixel centre;
 * a sample's weight is the product over x and y. Box: 1 for |r| <= 0.5, else 0. */
int mtx_rfilter_eval(uint32_t rfilter, const float *r, float *w_out, uint64_t n);

/* --------------------------- primitives --------------------------- */
/* prefix_sum.py:9-36: inclusive (or exclusive) scan of u32, device-wide
 * decoupled look-back. Host pointers. */
int mtx_prefix_sum_u32(mtx_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n, int inclusive);
/* prefix_sum.py:9-36 with f32 data in Hillis-Steele summation order
 * (floor(log2 n)+1 passes x[j] += x[j-2^i]), bit-identical to the reference. */
int mtx_prefix_sum_f32_hs(mtx_ctx *ctx, const float *in, float *out, uint64_t n);
/* The two scans on device buffers (prefix_sum.py:9-36 on Dr.Jit arrays); the
 * input is not modified. */
int mtx_prefix_sum_u32_dev(mtx_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n, int inclusive);
int mtx_prefix_sum_f32_hs_dev(mtx_ctx *ctx, const float *in, float *out, uint64_t n);
/* hashgrid.py:16-90: cell = hash(trunc((p-bbmin)/(bbmax-bbmin)*res)) % n_cells,
 * cell_size, exclusive cell_offset, and sample_idx (per-cell order ascending
 * by sample index). p: 3n floats (x[n], y[n], z[n] planes). */
int mtx_hashgrid_build(mtx_ctx *ctx, const float *p, uint64_t n, uint32_t resolution, uint32_t n_cells,
                       uint32_t *cell, uint32_t *cell_size, uint32_t *cell_offset, uint32_t *sample_idx);
/* HashGrid(sample, ...) on device buffers (hashgrid.py:16-84 on Dr.Jit arrays). */
int mtx_hashgrid_build_dev(mtx_ctx *ctx, const float *p, uint64_t n, uint32_t resolution, uint32_t n_cells,
                           uint32_t *cell, uint32_t *cell_size, uint32_t *cell_offset, uint32_t *sample_idx);
/* reductions.py:12-54 scatter_reduce_with for func in {ADD=0, MIN=1, MAX=2,
 * MUL=3}: target[index[i]] = func(target[index[i]], value[i]), each target's
 * values applied in ascending i order (deterministic; the reference's order
 * is race-defined). The reference takes any Python callable (:12, :53): the
 * Python layer folds such a callable over mtx_group_by_u32 /
 * mtx_group_by_u32_dev's groups, round by round (on the device with torch
 * tensors). target is read-modify-write. */
int mtx_scatter_reduce_f32(mtx_ctx *ctx, int op, float *target, uint64_t n_target, const float *value,
                           const uint32_t *index, uint64_t n_value);
/* scatter_reduce_with on device buffers (reductions.py:12-54 on Dr.Jit
 * arrays); target is updated in place; an index >= n_target: MTX_E_ARG. */
int mtx_scatter_reduce_f32_dev(mtx_ctx *ctx, int op, float *target, uint64_t n_target, const float *value,
                               const uint32_t *index, uint64_t n_value);
/* The stable group-by behind mtx_hashgrid_build / mtx_scatter_reduce_f32
 * for caller keys (< n_keys): key_size, exclusive key_offset and order
 * (element indices grouped by key, ascending inside a key). The Python
 * scatter_reduce_with folds an arbitrary callable over it round by round,
 * as reductions.py:21-54 does with one election per round. Host pointers. */
int mtx_group_by_u32(mtx_ctx *ctx, const uint32_t *keys, uint64_t n, uint32_t n_keys, uint32_t *key_size,
                     uint32_t *key_offset, uint32_t *order);
/* mtx_group_by_u32 on DEVICE pointers of the context's device (keys: n u32,
 * key_size / key_offset: n_keys u32, order: n u32), for callers whose data
 * stays in HBM (mtx.primitives.scatter_reduce_with with torch tensors). The
 * keys are range-checked on the device first (MTX_E_ARG if one is >= n_keys);
 * returns after the results are complete. */
int mtx_group_by_u32_dev(mtx_ctx *ctx, const uint32_t *keys, uint64_t n, uint32_t n_keys, uint32_t *key_size,
                         uint32_t *key_offset, uint32_t *order);
/* mtx_hashgrid_view and MTX_HG_MAX_QUERY_CELLS: with the photon gather above. */
/* Fixed-radius query: the samples of the grid within radius of each of the
 * m points q (3, m). One lane per query walks the grid cells its sphere can
 * touch, ascending in cz, then cy, then cx, and inside a grid cell the
 * samples in ascending index; samples of other grid cells that share the
 * hash cell are told apart by their own cell coordinates, so a sample is met
 * once. The cell coordinate of a value is the build's, with a negative or NaN
 * argument giving 0, the argument clamped to resolution, and 0 everywhere
 * when bbmax - bbmin is not positive. Sample j is a neighbour iff, in fp32
 * without contraction, (dx dx + dy dy) + dz dz <= r r with dx = p.x - q.x,
 * ...; NaN in q or r, or r < 0, gives none. radius: one device float for all
 * queries (radius_stride 0) or m of them (radius_stride 1). count (m)
 * receives each query's number of neighbours. A query whose cell box holds
 * more than MTX_HG_MAX_QUERY_CELLS cells is not walked: MTX_E_ARG with the
 * number of such queries (build the grid with resolution ~ extent / (2 r));
 * the context stays usable. Entries of cell_size, cell_offset and sample_idx
 * that would lead past n are not followed. Complete on return. */
int mtx_hashgrid_query_count_dev(mtx_ctx *ctx, const mtx_hashgrid_view *grid, const float *q, uint64_t m,
                                 const float *radius, uint32_t radius_stride, uint32_t *count);
/* The pairs of the query above in walk order: query i writes its neighbours
 * to query_idx / sample_idx_out [offset[i], offset[i] + count[i]), offset the
 * exclusive scan of count, total its sum (< 2^31); a pair that would land at
 * or past total is not written. */
int mtx_hashgrid_query_fill_dev(mtx_ctx *ctx, const mtx_hashgrid_view *grid, const float *q, uint64_t m,
                                const float *radius, uint32_t radius_stride, const uint32_t *offset, uint64_t total,
                                uint32_t *query_idx, uint32_t *sample_idx_out);

/* --------------------------- radiance field ----------------------- */
/* nerad.py:54-106 Field (hash-grid + SH encoding, fp16 MLP with LeakyReLU,
 * no bias), the radiance cache queried by NRC. */
typedef struct mtx_field_desc {
  uint32_t n_levels, n_features, log2_table, base_res; /* grid encoding */
  float per_level_scale;
  float bbox_min[3], bbox_max[3];                     /* scene.bbox() */
  uint32_t n_in;      /* features per query: 3 + n_levels*n_features + 3 + 16, <= 64 */
  uint32_t n_hidden;  /* hidden 64x64 layers (nerad.py:61: 4) */
  const uint16_t *table;   /* fp16 bits [n_levels][2^log2_table][n_features] */
  const uint16_t *weights; /* fp16 bits, row-major W0[64][n_in], W1..Wn[64][64], Wout[3][64] */
} mtx_field_desc;
/* Copy a field to HBM (weights prepacked as MFMA fragments). */
int mtx_field_upload(mtx_ctx *ctx, const mtx_field_desc *field);
/* Features (n x 64 fp16 bits) of n queries (p, wi: 3n floats). Host pointers. */
int mtx_field_features(mtx_ctx *ctx, uint64_t n, const float *p, const float *wi, uint16_t *feat);
/* MLP on n feature rows (n x 64 fp16 bits) -> out (3n floats). Host pointers. */
int mtx_field_mlp(mtx_ctx *ctx, uint64_t n, const uint16_t *feat, float *out);
/* Field(si) for n queries: encode + MLP -> out (3n floats). Host pointers. */
int mtx_field_eval(mtx_ctx *ctx, uint64_t n, const float *p, const float *wi, float *out);

/* ------------------ radiance-field training (nerad.py) ------------------ */
/* nerad.py:336-400: the field above trained by neural radiosity. The fp16
 * table / weights uploaded with mtx_field_upload are the network; training
 * keeps fp32 master copies + Adam moments in the context and re-casts the
 * fp16 field after every step (:389-390). */
typedef struct mtx_field_opt {
  float lr, beta_1, beta_2, epsilon;     /* drjit.opt.Adam(lr=1e-3) defaults (:336-342) */
  float init_scale, growth_factor, backoff_factor;
  uint32_t growth_interval;              /* drjit.opt.GradScaler (:347) */
} mtx_field_opt;
typedef struct mtx_train_stats {
  double loss;        /* mean((L_lhs - L_rhs)^2) of the step, unscaled (:370) */
  float scale;        /* GradScaler scale after the step */
  uint32_t found_inf; /* 1: non-finite gradient, step skipped */
  uint32_t step;      /* Adam steps taken */
  uint32_t rhs_queries;
  double ms_lhs, ms_rhs, ms_train, ms_total; /* HIP-event times of the phases */
  double ms_trace;    /* closest-hit traversal launches of the RHS */
  uint64_t rays_closest, nodes_closest, tris_closest; /* RHS visit counters (args.flags bit 0) */
} mtx_train_stats;
/* Start training the uploaded field (fp32 master copies, zero moments). */
int mtx_field_train_init(mtx_ctx *ctx, const mtx_field_opt *opt);
/* Loss and gradients of scale * loss w.r.t. the table (fp32, n_levels*2^log2_table*n_features)
 * and the weights (fp32, mtx_field_desc order) for n points (p, wi: 3n) and targets (3n);
 * out: the network output (3n). Host pointers; any output may be NULL. No update. */
int mtx_field_grad(mtx_ctx *ctx, uint64_t n, const float *p, const float *wi, const float *target, float scale,
                   float *out, double *loss, float *grad_table, float *grad_weights);
/* One optimiser step on host-supplied points / targets (forward, backward, GradScaler + Adam). */
int mtx_field_train_step(mtx_ctx *ctx, uint64_t n, const float *p, const float *wi, const float *target,
                         mtx_train_stats *stats);
/* fp32 master parameters (table, weights) and Adam moments; any pointer may be NULL. */
int mtx_field_params(mtx_ctx *ctx, float *table, float *weights, float *m, float *v);

/* Surface-area tables of the uploaded scene (IntersectionSampler, nerad.py:281-289): the
 * shape distribution and per shape the distribution over its triangles (entries
 * [tri_off[s], tri_off[s+1]) of tri_pmf / tri_cdf / tri_prim; leaf-order triangles).
 * cdf = double-accumulated inclusive prefix stored as float; *_valid = first / last
 * index with non-zero pmf. */
typedef struct mtx_nerad_tables {
  uint32_t n_shapes, n_entries;
  const float *shape_pmf, *shape_cdf;
  float shape_sum, shape_norm;
  uint32_t shape_valid[2];
  const uint32_t *tri_off;    /* n_shapes + 1 */
  const float *tri_pmf, *tri_cdf;
  const uint32_t *tri_prim;
  const float *tri_sum, *tri_norm; /* n_shapes */
  const uint32_t *tri_valid;       /* 2 per shape */
} mtx_nerad_tables;
int mtx_nerad_upload(mtx_ctx *ctx, const mtx_nerad_tables *t);
typedef struct mtx_nerad_args {
  uint32_t lhs_seed;  /* sampler_lhs.seed(seed(), batch_size) (:387) */
  uint32_t rhs_seed;  /* sampler.seed(seed(), batch_size * M) in sample_rhs (:189) */
  uint32_t batch;     /* batch_size (:258: 2^14) */
  uint32_t M;         /* RHS samples per point (:259: 32) */
  uint32_t flags;     /* bit 0: count traversal visits (slower STATS kernels) */
} mtx_nerad_args;
/* IntersectionSampler.sample for `batch` points (:291-310): 9 floats per point
 * (prim as uint32 bits, b1, b2, p.xyz, wi_world.xyz). */
int mtx_nerad_lhs(mtx_ctx *ctx, const mtx_nerad_args *a, float *out);
/* Integrator.sample_rhs (:174-233) at the mtx_nerad_lhs(a) points with the current field:
 * L_rhs (3 per point); lanes (NULL or 3 * batch * M): every sample's L before the mean. */
int mtx_nerad_rhs(mtx_ctx *ctx, const mtx_nerad_args *a, float *L_rhs, float *lanes);
/* training_step (:363-375) on the device: LHS points, L_lhs = Field(si), L_rhs, loss,
 * backward, GradScaler + Adam, fp16 refresh of the field. */
int mtx_nerad_step(mtx_ctx *ctx, const mtx_nerad_args *a, mtx_train_stats *stats);

/* HIP-event time (ms) of the device work of the last primitive call on ctx
 * (the scan / hash / scatter kernels, without the host<->device copies);
 * used by bench.py to report the primitives against their rooflines. */
double mtx_last_device_ms(mtx_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MTX_H_ */
