"""Axis-aligned lattice scenes and an exact reference for the BVH traversal and
the triangle test, shared by test_lattice.py (CPU oracle) and
test_lattice_gpu.py (the kernels).

Scene: sheets of N x N axis-aligned quads (step 0.5, N = 8, so a sheet spans
[-2, 2]^2), each quad split along alternating diagonals with the right angle
at the triangle's first vertex (the hypotenuse u + v = 1 is the diagonal), in
the planes -2, -1, -1 again, 0, 1, 2 of each of the three axes: 18 sheets,
2,304 triangles. The repeated -1 plane is a coincident duplicate sheet, so
closest hits there are equal-t ties between different triangles. Every vertex
is a multiple of 1/4. Variants: ``plain`` (one shape per orientation; the x
stack emits, the z stack is the movable non-emitter), ``emit`` (one shape and
one mesh area emitter per sheet, radiance channels distinct powers of two),
``rot`` (``plain`` without the duplicate sheets under a fixed rigid rotation:
the off-lattice class), and each of the first two translated by OFFSET (still
exact in fp32).

Reference: Moeller-Trumbore in float64 numpy over the scene's leaf-order
records (p0, e1, e2). det == 0 is a miss; a hit needs u >= 0, u <= 1, v >= 0,
u + v <= 1 and 0 < t <= maxt; the closest hit is the smallest t, ties to the
smallest leaf-order index; any hit iff some triangle hits. It is exact because
of its premises, asserted on every call (`lattice_reference`):

  * every vertex and ray origin is a multiple of 1/4,
  * every direction component is 0 or +- a power of two,
  * |det| is a power of two for every (ray, triangle) pair with det != 0,
  * the returned t, u, v survive a round trip through float32.

Then every product, sum and quotient of fp32 tri_intersect is exact, fused or
not, and the kernels must return the reference's four words bit for bit. The
scalar triple products are evaluated as (rays x 3) @ (3 x triangles) matrix
products (u det = e2.(o x d) - d.(e2 x p0), v det = -e1.(o x d) - d.(p0 x e1),
t det = (o - p0).n, det = -d.n with n = e1 x e2): algebraically the
Moeller-Trumbore terms, exact in float64 on the lattice in any order;
`direct_reference` evaluates the textbook form pair by pair (the off-lattice
class uses it, and a CPU test holds the two against each other). No code is
shared with mtx_core."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from test_mitsuba_dict import T

N, STEP = 8, 0.5
PLANES = (-2.0, -1.0, -1.0, 0.0, 1.0, 2.0)
OFFSET = (1024.0, -2048.0, 4096.0)
MOVE = (0.25, -0.5, 0.75)  # the lattice vector of the refit tests
MISS = 0xFFFFFFFF
FAR = np.float32(3.0e38)
SKEW = [(2, 1, 0), (1, -2, 0), (0, 1, 4), (-4, 0, 1), (1, 2, 4)]
NEG_ZERO = [(-0.0, 1, 0), (1, -0.0, -0.0), (-0.0, -0.0, -1), (-0.0, 1, 1), (1, -0.0, 2), (-1, -1, -0.0)]
N_ORIGINS = 1400
ROT_AXIS, ROT_DEG = (1.0, 2.0, 3.0), 37.0
VARIANTS = ("plain", "emit", "rot")


# ------------------------------------------------------------------ scene --
def sheet(axis, c):
    """(vertices (81, 3), faces (128, 3) 0-based) of the sheet in plane
    x[axis] = c; the in-plane axes are (axis + 1) % 3 and (axis + 2) % 3."""
    a, b = (axis + 1) % 3, (axis + 2) % 3
    g = -N * STEP / 2 + STEP * np.arange(N + 1)
    v = np.zeros(((N + 1) ** 2, 3))
    v[:, axis] = c
    v[:, a] = np.repeat(g, N + 1)
    v[:, b] = np.tile(g, N + 1)
    f = []
    for i in range(N):
        for j in range(N):
            p, q, r, s = i * (N + 1) + j, (i + 1) * (N + 1) + j, (i + 1) * (N + 1) + j + 1, i * (N + 1) + j + 1
            if (i + j) % 2 == 0:  # diagonal p-r, right angles at q and s
                f += [(q, r, p), (s, p, r)]
            else:  # diagonal q-s, right angles at p and r
                f += [(p, q, s), (r, s, q)]
    return v, np.array(f)


def sheet_radiance(k):
    """Radiance of sheet k (0 .. 17) in the ``emit`` variant."""
    return [2.0 ** (k - 8), 2.0 ** -k, 2.0 ** (k % 7)]


def rotation():
    return T().rotate(ROT_AXIS, ROT_DEG).matrix[:3, :3]


def _write_obj(path, verts, faces):
    with open(path, "w") as fh:
        for p in verts:
            fh.write("v %r %r %r\n" % tuple(float(x) for x in p))
        for t in faces:
            fh.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def write_meshes(dirname):
    """sheet_<k>.obj (per sheet), stack_<axis>.obj (per orientation),
    rot_<axis>.obj (rotated, rounded to fp32) and the t_ files translated by
    OFFSET."""
    R = rotation()
    for axis in range(3):
        vs, fs, nv = [], [], 0
        for j, c in enumerate(PLANES):
            v, f = sheet(axis, c)
            for pre, off in (("", 0.0), ("t_", np.array(OFFSET))):
                _write_obj(os.path.join(dirname, "%ssheet_%d.obj" % (pre, axis * len(PLANES) + j)), v + off, f)
            vs.append(v)
            fs.append(f + nv)
            nv += len(v)
        v, f = np.concatenate(vs), np.concatenate(fs)
        _write_obj(os.path.join(dirname, "stack_%d.obj" % axis), v, f)
        _write_obj(os.path.join(dirname, "t_stack_%d.obj" % axis), v + np.array(OFFSET), f)
        # the rotated copy leaves the duplicate sheet out: an exact tie is never "clear" (class f)
        keep_v, keep_f = np.arange(len(v)) // (N + 1) ** 2 != 2, np.arange(len(f)) // (2 * N * N) != 2
        fr = f[keep_f] - np.where(f[keep_f] >= 3 * (N + 1) ** 2, (N + 1) ** 2, 0)
        _write_obj(os.path.join(dirname, "rot_%d.obj" % axis), (v[keep_v] @ R.T).astype(np.float32), fr)


def scene_dict(variant="plain", translated=False):
    assert variant in VARIANTS and not (translated and variant == "rot")
    pre = "t_" if translated else ""
    c = np.array(OFFSET) if translated else np.zeros(3)
    d = {
        "type": "scene",
        "sensor": {"type": "perspective", "fov": 60.0, "near_clip": 0.01, "far_clip": 100.0,
                   "to_world": T.look_at(list(c + [0.3, 0.4, 6.0]), list(c), [0, 1, 0]),
                   "film": {"type": "hdrfilm", "width": 16, "height": 16, "rfilter": {"type": "tent"}}},
        "grey": {"type": "diffuse", "reflectance": {"type": "rgb", "value": 0.5}},
    }
    if variant == "emit":
        for k in range(3 * len(PLANES)):
            d["sheet_%d" % k] = {"type": "obj", "filename": "%ssheet_%d.obj" % (pre, k),
                                 "bsdf": {"type": "ref", "id": "grey"},
                                 "emitter": {"type": "area", "radiance": {"type": "rgb", "value": sheet_radiance(k)}}}
        return d
    name = "rot" if variant == "rot" else pre + "stack"
    for axis in range(3):
        d["stack_%d" % axis] = {"type": "obj", "filename": "%s_%d.obj" % (name, axis),
                                "bsdf": {"type": "ref", "id": "grey"}}
    d["stack_0"]["emitter"] = {"type": "area", "radiance": {"type": "rgb", "value": [1.0, 2.0, 4.0]}}
    return d


MOVABLE_SHAPE = 2  # ``plain``: the z stack (shapes keep the dictionary's order)
_SCENES = {}


def build(dirname, variant="plain", translated=False):
    """The mtx Scene of a variant (cached per directory)."""
    from mtx.mitsuba_dict import scene_from_dict

    key = (str(dirname), variant, translated)
    if key not in _SCENES:
        if not os.path.exists(os.path.join(dirname, "rot_2.obj")):
            write_meshes(dirname)
        _SCENES[key] = scene_from_dict(scene_dict(variant, translated), base_dir=str(dirname))
    return _SCENES[key]


def moved_vertices(scene):
    """``plain``'s vertices with the z stack moved by MOVE (on the lattice)."""
    from refit_cases import shape_vertices

    v = scene.vpos.reshape(-1, 3).astype(np.float32).copy()
    v[shape_vertices(scene, MOVABLE_SHAPE)] += np.array(MOVE, np.float32)
    return v


# ------------------------------------------------------------------- rays --
def make_rays(o, d, maxt=FAR):
    r = np.zeros((len(o), 8), np.float32)
    r[:, 0:3], r[:, 4:7], r[:, 3] = o, d, maxt
    return r


_RAYS_A = None


def directions_a():
    d26 = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
    return np.array(d26 + SKEW + NEG_ZERO, np.float32)


def rays_a(offset=(0.0, 0.0, 0.0)):
    """Class (a): N_ORIGINS lattice origins of [-2, 2]^3 (step 1/4) x the 26
    directions of {-1, 0, 1}^3, five skew dyadic ones and six with -0.0
    components; unbounded. Ray-major in the direction (origin i has rows
    37 i .. 37 i + 36)."""
    global _RAYS_A
    if _RAYS_A is None:
        rng = np.random.default_rng(20)
        idx = rng.choice(17 ** 3, N_ORIGINS, replace=False)
        o = np.stack(np.unravel_index(idx, (17, 17, 17)), 1) * 0.25 - 2.0
        d = directions_a()
        _RAYS_A = make_rays(np.repeat(o, len(d), 0), np.tile(d, (len(o), 1)))
        _RAYS_A.setflags(write=False)
    r = _RAYS_A.copy()
    r[:, 0:3] += np.array(offset, np.float32)
    return r


def rays_b(rays, ref):
    """Class (b): the hits of `rays` with maxt = float32(t) (they must hit)
    and with maxt = nextafter(float32(t), 0) (that hit is gone)."""
    sel = ref.prim != MISS
    at, below = rays[sel].copy(), rays[sel].copy()
    t = ref.t[sel].astype(np.float32)
    at[:, 3] = t
    below[:, 3] = np.nextafter(t, np.float32(0))
    return at, below


def scaled(rays, k):
    """Class (c): directions times 2^k."""
    r = rays.copy()
    r[:, 4:7] = np.ldexp(r[:, 4:7], k)
    return r


def rays_zero(n=512):
    """Class (e): d = (0, 0, 0) from lattice origins, on and off the sheets,
    bounded and unbounded."""
    r = rays_a()[::37][:n].copy()
    r[:, 4:7] = 0.0
    r[::3, 3] = 1.0
    return r


# -------------------------------------------------------------- reference --
class Ref:
    """Per ray: t, u, v (float64; inf, 0, 0 on a miss), prim (uint32, MISS),
    any (bool), and the classification the hollow-class assertions use:
    ties (triangles hit at the closest t), on_surface (some triangle with
    det != 0 contains the origin: t = 0), in_plane (some triangle has det = 0
    and the origin in its plane)."""

    def words(self):
        """The (n, 4) words (t, prim, u, v) mtx_trace returns (`canonical`)."""
        w = np.zeros((len(self.t), 4), np.uint32)
        w[:, 0] = self.t.astype(np.float32).view(np.uint32)
        w[:, 1] = self.prim
        w[:, 2] = self.u.astype(np.float32).view(np.uint32)
        w[:, 3] = self.v.astype(np.float32).view(np.uint32)
        return w


def canonical(hits):
    """Hit words with a zero u or v as +0: the sign of a zero barycentric is
    that of the last exact sum that formed it, an artefact of the order of the
    terms and no property of the hit. Everything else is compared bit for bit."""
    w = np.array(hits, np.uint32).reshape(-1, 4)
    w[:, 2:4] = np.where(w[:, 2:4] == 0x80000000, 0, w[:, 2:4])
    return w


def _geom64(geom):
    g = np.asarray(geom, np.float32).reshape(-1, 12).astype(np.float64)
    return g[:, 0:3], g[:, 4:7], g[:, 8:11]


def _pow2_or_zero(x):
    m, _ = np.frexp(np.abs(x))
    return bool(np.all((x == 0) | (m == 0.5)))


def _select(ref_parts, det, un, vn, tn, maxt, pn, any_only=False):
    """One chunk: numerators and det (rays x triangles) -> closest hit."""
    ok = det != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v, t = un / det, vn / det, tn / det
        return _select_uvt(ref_parts, ok, det, u, v, t, tn, maxt, pn, any_only)


def _select_uvt(ref_parts, ok, det, u, v, t, tn, maxt, pn, any_only):
    hit = ok & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0) & (t <= maxt[:, None])
    if any_only:
        ref_parts["any"].append(hit.any(1))
        return
    th = np.where(hit, t, np.inf)
    tmin = th.min(1)
    first = (hit & (th == tmin[:, None]))
    prim = first.argmax(1)  # the first True: the smallest leaf-order index
    anyh = hit.any(1)
    rows = np.arange(len(det))
    ref_parts["t"].append(np.where(anyh, tmin, np.inf))
    ref_parts["u"].append(np.where(anyh, u[rows, prim], 0.0) + 0.0)  # + 0.0: a zero is +0 (canonical)
    ref_parts["v"].append(np.where(anyh, v[rows, prim], 0.0) + 0.0)
    ref_parts["prim"].append(np.where(anyh, prim, MISS).astype(np.uint32))
    ref_parts["any"].append(anyh)
    ref_parts["ties"].append(first.sum(1))
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)
    ref_parts["on_surface"].append((inside & (tn == 0)).any(1))
    ref_parts["in_plane"].append(((det == 0) & (pn == 0)).any(1))


def _finish(parts):
    r = Ref()
    for k, v in parts.items():
        setattr(r, k, np.concatenate(v))
    return r


_FIELDS = ("t", "u", "v", "prim", "any", "ties", "on_surface", "in_plane")


def lattice_reference(geom, rays, lattice=0.25, chunk=2048, any_only=False):
    """The exact reference over 12-float records `geom` (scene.tri_geom for
    closest hit, scene.occ_tri_geom for any hit) and (n, 8) rays. Asserts its
    premises (module docstring). `any_only`: only the any-hit answer."""
    p0, e1, e2 = _geom64(geom)
    rays = np.asarray(rays, np.float32)
    o, d, maxt = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64), rays[:, 3].astype(np.float64)
    for name, a in (("p0", p0), ("e1", e1), ("e2", e2), ("origins", o)):
        assert np.array_equal(a / lattice, np.round(a / lattice)), name + " off the lattice"
    assert np.all(np.sum(e1 * e2, 1) == 0), "right angle at p0: the hypotenuse is the quad's diagonal"
    assert _pow2_or_zero(d), "direction components are 0 or +- powers of two"
    n = np.cross(e1, e2)
    c_u, c_v, c_t = np.cross(e2, p0), np.cross(p0, e1), np.sum(p0 * n, 1)
    fields = ("any",) if any_only else _FIELDS

    def one(s):
        oc, dc = o[s:s + chunk], d[s:s + chunk]
        od = np.cross(oc, dc)
        det = -(dc @ n.T)
        assert _pow2_or_zero(det), "|det| is a power of two wherever it is not 0"
        pn = oc @ n.T - c_t  # (o - p0).n = t det
        part = {k: [] for k in fields}
        _select(part, det, od @ e2.T - dc @ c_u.T, -(od @ e1.T) - dc @ c_v.T, pn, maxt[s:s + chunk], pn, any_only)
        return part

    with ThreadPoolExecutor(max_workers=8) as pool:  # numpy releases the GIL; chunks are independent
        chunks = list(pool.map(one, range(0, len(rays), chunk)))
    r = _finish({k: [c[k][0] for c in chunks] for k in fields})
    for a in (() if any_only else (r.t, r.u, r.v)):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), "t, u, v are fp32 numbers"
    return r


def direct_reference(geom, rays, bounds=False):
    """Textbook Moeller-Trumbore pair by pair in float64 (rays x triangles in
    memory: a few thousand rays). With `bounds` also returns, per pair, the
    values and their fp32 error bounds (offlattice_classes)."""
    p0, e1, e2 = _geom64(geom)
    rays = np.asarray(rays, np.float32)
    o = rays[:, None, 0:3].astype(np.float64)
    d = rays[:, None, 4:7].astype(np.float64)
    maxt = rays[:, 3].astype(np.float64)
    pvec = np.cross(d, e2[None])
    det = np.sum(e1[None] * pvec, 2)
    tvec = o - p0[None]
    un = np.sum(tvec * pvec, 2)
    qvec = np.cross(tvec, e1[None])
    vn = np.sum(d * qvec, 2)
    tn = np.sum(e2[None] * qvec, 2)
    parts = {k: [] for k in _FIELDS}
    _select(parts, det, un, vn, tn, maxt, tn)
    r = _finish(parts)
    if not bounds:
        return r

    def acr(a, b):  # the cross product's terms in magnitude
        a, b = np.abs(a), np.abs(b)
        return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)

    at = np.abs(o) + np.abs(p0[None])  # the terms of tvec = o - p0
    apv, aqv = acr(d, e2[None]), acr(at, e1[None])
    s_det = np.sum(np.abs(e1[None]) * apv, 2)
    s_u, s_v, s_t = np.sum(at * apv, 2), np.sum(np.abs(d) * aqv, 2), np.sum(np.abs(e2[None]) * aqv, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v, t = un / det, vn / det, tn / det
        k = TAU_C * 2.0 ** -24 / np.abs(det)
        tau = [k * (s + np.abs(x) * s_det) for s, x in ((s_u, u), (s_v, v), (s_t, t))]
    return r, (u, v, t), tau


# Off-lattice error bound (class f). fp32 tri_intersect computes x = num /
# det for x in (u, v, t) as num * (1 / det). Expand num into its terms
# a_i b_j c_k (one factor each from tvec = o - p0, an edge, and d or the other
# edge). On the longest chain (t and v, through qvec = cross(tvec, e1)) a term
# passes at most six roundings: the subtraction forming tvec (taken on the
# terms |o| + |p0|, so cancellation there is covered), the product inside the
# cross, the cross's subtraction, the product inside the dot, and the dot's two
# additions; fused multiply-adds only remove roundings. det's terms pass five
# (no tvec), then 1 / det and the final product round once each. So, with
# S_x = sum |terms of num_x| and S_det = sum |terms of det| >= |det|,
#   |fp32(x) - x| <= 2^-24 (6 S_x + |x| (5 S_det + 2 |det|)) / |det| + O(2^-48)
#                 <= TAU_C 2^-24 (S_x + |x| S_det) / |det|,  TAU_C = 8
# (8 >= 7 leaves the second-order terms a margin of one part in seven). The
# sum u + v rounds once more: its bound is tau_u + tau_v + 2^-24. The bound is
# derived, not measured on any kernel.
TAU_C = 8.0
AIM_KINDS = (("interior", 1200), ("edge", 600), ("vertex", 600))


def rays_f(geom, seed=3):
    """Class (f): rays from random points of [-1.9, 1.9]^3 aimed (in float64,
    then rounded to fp32) at triangle interiors, edge midpoints and vertices of
    the ``rot`` scene. Returns (rays, kind index per ray)."""
    p0, e1, e2 = _geom64(geom)
    rng = np.random.default_rng(seed)
    rays, kinds = [], []
    for ki, (kind, n) in enumerate(AIM_KINDS):
        tri = rng.integers(0, len(p0), n)
        if kind == "interior":
            a = rng.uniform(0.1, 0.8, n)
            b = rng.uniform(0.1, 0.9 - a)
        elif kind == "edge":
            e = rng.integers(0, 3, n)
            a, b = np.array([0.5, 0.0, 0.5])[e], np.array([0.0, 0.5, 0.5])[e]
        else:
            c = rng.integers(0, 3, n)
            a, b = np.array([0.0, 1.0, 0.0])[c], np.array([0.0, 0.0, 1.0])[c]
        target = p0[tri] + a[:, None] * e1[tri] + b[:, None] * e2[tri]
        o = rng.uniform(-1.9, 1.9, (n, 3))
        d = target - o
        rays.append(make_rays(o, d / np.linalg.norm(d, axis=1, keepdims=True)))
        kinds.append(np.full(n, ki))
    return np.concatenate(rays), np.concatenate(kinds)


def offlattice_classes(geom, rays):
    """(ref, clear mask, bound_t, bound_u, bound_v). A ray is clear when fp32
    tri_intersect, whatever its rounding, must report the reference's triangle:
    either every triangle misses by more than its bound, or some triangle k
    hits robustly (u, v and 1 - u - v above their bounds, t above its bound)
    and every other triangle either misses robustly or lies certainly behind
    (t_j - tau_j > t_k + tau_k). The rays are unbounded, so maxt plays no
    part. Everything else is borderline."""
    ref, (u, v, t), (tu, tv, tt) = direct_reference(geom, rays, bounds=True)
    tuv = tu + tv + 2.0 ** -24
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(tuv) & np.isfinite(tt)
        rob_hit = fin & (u > tuv) & (v > tuv) & (1 - u - v > tuv) & (t > tt)
        rob_miss = fin & ((u < -tuv) | (v < -tuv) | (u + v > 1 + tuv) | (t < -tt))
    rows = np.arange(len(rays))
    k = np.where(ref.any, ref.prim, 0).astype(np.int64)
    near = (t[rows, k] + tt[rows, k])[:, None]
    with np.errstate(invalid="ignore"):
        behind = fin & (t - tt > near)
    other = rob_miss | behind
    other[rows, k] = True
    clear_hit = ref.any & rob_hit[rows, k] & other.all(1)
    clear = np.where(ref.any, clear_hit, rob_miss.all(1))
    return ref, clear, tt[rows, k], tu[rows, k], tv[rows, k]


def check_off_lattice(hits, ref, clear, bt, bu, bv):
    """Clear rays of class (f): the reference's triangle exactly, t, u, v
    within their bounds; a clear miss is a miss."""
    w = np.asarray(hits, np.uint32).reshape(-1, 4)
    f = w.view(np.float32).astype(np.float64)
    assert np.array_equal(w[clear, 1], ref.prim[clear])
    h = clear & ref.any
    for col, want, bound, name in ((0, ref.t, bt, "t"), (2, ref.u, bu, "u"), (3, ref.v, bv, "v")):
        err = np.abs(f[h, col] - want[h])
        assert np.all(err <= bound[h]), (name, float((err / bound[h]).max()))
    assert np.all(np.isinf(f[clear & ~ref.any, 0]))


# ------------------------------------------------- hollow-class assertions --
def class_a_counts(ref):
    """What class (a) must contain, from the reference alone."""
    hit = ref.prim != MISS
    corner = hit & (((ref.u == 0) & (ref.v == 0)) | ((ref.u == 1) & (ref.v == 0)) | ((ref.u == 0) & (ref.v == 1)))
    return {"on_surface": int(ref.on_surface.sum()),
            "diagonal": int((hit & (ref.u + ref.v == 1) & (ref.u > 0) & (ref.v > 0)).sum()),
            "vertex4": int((corner & (ref.ties >= 4)).sum()),
            "in_plane": int(ref.in_plane.sum()),
            "hit_share": float(hit.mean())}


def twins(geom):
    """Per leaf-order triangle: True when another triangle has the same
    (p0, e1, e2) -- the coincident duplicate sheets."""
    g = np.asarray(geom, np.float32).reshape(-1, 12)[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]
    _, inv, cnt = np.unique(g, axis=0, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)] > 1


def assert_class_a_not_hollow(geom, ref):
    c = class_a_counts(ref)
    hit = ref.prim != MISS
    c["coincident_tie"] = int((hit & twins(geom)[np.where(hit, ref.prim, 0)]).sum())
    for k in ("on_surface", "diagonal", "vertex4", "coincident_tie", "in_plane"):
        assert c[k] >= 200, c
    assert 0.5 < c["hit_share"] < 0.95, c
    return c


# ------------------------------------------------------- expected radiance --
def expected_radiance(scene, geom, rays, ref):
    """L and valid of the ``integrator`` estimator at max_depth 1 on the
    ``emit`` scene: the radiance of the hit triangle's sheet where the ray
    meets its emitting side, n.d < 0 with n = e1 x e2 (emitter_eval returns the
    radiance when the local wi = -d has z > 0 in the frame of the face normal
    normalize(cross(p1 - p0, p2 - p0))), and 0 elsewhere. The sign is exact:
    n is +-1/4 along one axis and d a power of two there."""
    _, e1, e2 = _geom64(geom)
    hit = ref.prim != MISS
    k = np.where(hit, ref.prim, 0).astype(np.int64)
    nd = np.sum(np.cross(e1[k], e2[k]) * rays[:, 4:7].astype(np.float64), 1)
    sheet_of = np.asarray(scene.tri_shape)[k]  # one shape per sheet, in the dictionary's order
    rad = np.array([sheet_radiance(s) for s in range(3 * len(PLANES))], np.float32)
    L = np.where((hit & (nd < 0))[:, None], rad[sheet_of], np.float32(0)).astype(np.float32)
    return L, hit


# ------------------------------------------------------ shared test bodies --
_REFS = {}


def cached(key, fn):
    """Compute a reference once per process; the result is never modified."""
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def refs(key, scene, rays):
    """(closest-hit reference over tri_geom, any-hit reference over
    occ_tri_geom) of `rays`, cached under `key`."""
    return cached(key, lambda: (lattice_reference(scene.tri_geom, rays), lattice_reference(scene.occ_tri_geom, rays, any_only=True)))


def check_trace(trace, scene, rays, words, occluded, label=""):
    """trace(scene, rays, mode) -> hit words: mode 0 equals `words` bit for bit
    (`canonical`), mode 1 equals `occluded`."""
    got = canonical(trace(scene, rays, 0))
    bad = np.flatnonzero((got != words).any(1))
    assert len(bad) == 0, (label, "closest", len(bad), rays[bad[:3]], got[bad[:3]], words[bad[:3]])
    occ = np.asarray(trace(scene, rays, 1)).reshape(-1)
    bad = np.flatnonzero(occ.astype(bool) != occluded)
    assert set(np.unique(occ)) <= {0, 1} and len(bad) == 0, (label, "any", len(bad), rays[bad[:3]])


def scaled_words(ref, k):
    """Hit words of `ref`'s rays with the directions times 2^k: prim, u and v
    unchanged, t times 2^-k (exact)."""
    w = ref.words()
    w[:, 0] = np.ldexp(ref.t, -k).astype(np.float32).view(np.uint32)
    return w


PRODUCTION_N = (1, 63, 64, 65, 257, None)  # None: every ray of class (a)


def production_order(n_rays):
    """A fixed shuffle of class (a): the first n rows mix origins and
    directions at every n."""
    return np.random.default_rng(9).permutation(n_rays)


def sample_closest(scene, rays):
    """L, valid of the ``integrator`` estimator at max_depth 1 (one closest-hit
    trace per lane through the production loop, then emitter_eval)."""
    from mtx import IndependentSampler, load_dict

    integ = load_dict({"type": "integrator", "max_depth": 1})
    lanes = np.arange(len(rays), dtype=np.uint32)
    L, valid, _ = integ.sample(scene, IndependentSampler(1, lanes, skip=2), (rays[:, 0:3], rays[:, 4:7]))
    return L, valid


def variant_payload(dirname):
    """What a traversal-variant child compares against: classes (a) and (b)
    on ``plain`` and the closest-hit radiance on ``emit``, computed once by the
    parent from the reference."""
    plain, emit = build(dirname, "plain"), build(dirname, "emit")
    rays = rays_a()
    ra, oa = refs("a", plain, rays)
    at, below = rays_b(rays, ra)
    (rat, oat), (rbe, obe) = refs("b-at", plain, at), refs("b-below", plain, below)
    re_, _ = refs("a-emit", emit, rays)
    L, valid = expected_radiance(emit, emit.tri_geom, rays, re_)
    return {"rays": rays, "words": ra.words(), "occ": oa.any, "at": at, "at_words": rat.words(), "at_occ": oat.any,
            "below": below, "below_words": rbe.words(), "below_occ": obe.any, "L": L, "valid": valid,
            "plain_geom": plain.tri_geom, "emit_geom": emit.tri_geom}


def run_variant_child(dirname, npz):
    """Body of a traversal-variant child process (the environment is read when
    the context is created): the GPU against the parent's payload."""
    from test_gpu_parity import _trace_gpu

    p = np.load(npz)
    plain, emit = build(dirname, "plain"), build(dirname, "emit")
    assert np.array_equal(plain.tri_geom, p["plain_geom"]) and np.array_equal(emit.tri_geom, p["emit_geom"])

    def trace(s, r, m):
        return _trace_gpu(s, r, m)[0]

    check_trace(trace, plain, p["rays"], p["words"], p["occ"], "a")
    check_trace(trace, plain, p["at"], p["at_words"], p["at_occ"], "b-at")
    check_trace(trace, plain, p["below"], p["below_words"], p["below_occ"], "b-below")
    order = production_order(len(p["rays"]))
    for n in PRODUCTION_N:
        sel = order[:n]
        L, valid = sample_closest(emit, p["rays"][sel])
        assert np.array_equal(L, p["L"][sel]) and np.array_equal(valid, p["valid"][sel]), ("closest", n)
