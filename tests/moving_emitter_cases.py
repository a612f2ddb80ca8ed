"""Moves of mesh lights and the single-emitter scenes shared by
test_moving_emitters.py (the host's Scene.with_vertices, the oracle) and
test_moving_emitters_gpu.py (mtx_scene_update_vertices). The fixture scenes
are those of mesh_emitter_cases.py and lattice_cases.py; nothing here is
modified once built."""
import os

import mesh_emitter_cases as mc
import numpy as np
from refit_cases import shape_vertices
from test_mitsuba_dict import T

SHAPES = ("box", "steps", "patch", "rect")
STEPS_PIVOT = (0.25, 1.5, -0.5)  # a lattice point (multiples of 1/8) in the plane of ``steps``


def shape_index(name, variant="full"):
    return [k for k in mc.scene_dict(variant) if k in SHAPES].index(name)


def verts_of(scene, name, variant="full"):
    return shape_vertices(scene, shape_index(name, variant))


def base_vertices(scene):
    return np.array(scene.vpos, np.float32).reshape(-1, 3)


def steps_scaled(scene, variant="full"):
    """``steps`` scaled by 2 about STEPS_PIVOT: every coordinate stays exact,
    every area is multiplied by exactly 4."""
    v = base_vertices(scene)
    idx = verts_of(scene, "steps", variant)
    c = np.array(STEPS_PIVOT, np.float32)
    v[idx] = c + np.float32(2.0) * (v[idx] - c)
    return v


def patch_sheared(scene, variant="full", v=None):
    """``patch`` sheared (x grows with y) and translated: still facing +x,
    still inside the box, nothing between it and the reference points."""
    v = base_vertices(scene) if v is None else v
    idx = verts_of(scene, "patch", variant)
    p = v[idx].astype(np.float64)
    p[:, 0] += 0.1 * (p[:, 1] + 1.0) + 0.05
    p[:, 1] += 0.1
    p[:, 2] -= 0.1
    v[idx] = p.astype(np.float32)
    return v


def lights_and_wall(scene, variant="full"):
    """Both mesh lights and a non-emitter wall vertex in one update."""
    v = patch_sheared(scene, variant, steps_scaled(scene, variant))
    box = verts_of(scene, "box", variant)
    v[box[:4]] *= np.float32(1.03125)
    return v


def steps_ends_collapsed(scene, variant="full"):
    """The first and the last entry with pmf > 0 of ``steps`` collapsed onto
    a line (the third vertex to the midpoint of the other two; exact). Returns
    (vertices, the two entries)."""
    em = mc.emitter_of(scene, "steps", variant)
    m = scene.emitters[em].mesh
    _, _, prim = mc.mesh_tables(scene, em)
    v = base_vertices(scene)
    vid = np.asarray(scene.tri_vidx).reshape(-1, 3)
    ends = (m["valid_lo"], m["valid_hi"])
    for k in ends:
        a, b, c = vid[prim[k]]
        v[c] = (v[a] + v[b]) * np.float32(0.5)
    return v, ends


def all_collapsed(scene, name, variant="full"):
    v = base_vertices(scene)
    idx = verts_of(scene, name, variant)
    v[idx] = v[idx[0]]
    return v


def overflowing(scene, name="patch", variant="full"):
    """Coordinates within the vertex bound 2^37 whose squared cross product
    overflows fp32: edges of 2^36 give |cross| = 2^72, squared 2^144."""
    v = base_vertices(scene)
    idx = verts_of(scene, name, variant)
    v[idx] = (v[idx].astype(np.float64) * 2.0 ** 36).astype(np.float32)
    assert np.abs(v).max() <= 2.0 ** 37
    return v


def rectangle_moved(scene, variant="full"):
    v = base_vertices(scene)
    v[verts_of(scene, "rect", variant)[0], 1] += np.float32(0.01)
    return v


def tables_equal(a, b):
    """tables and emitter records of two host scenes, bit for bit."""
    return (np.array_equal(np.asarray(a.tables).view(np.uint32), np.asarray(b.tables).view(np.uint32))
            and bytes(a.emitters) == bytes(b.emitters) and a.n_tables == b.n_tables)


# ------------------------------------------------- single-emitter scenes --
def _sensor():
    return {"type": "perspective", "fov": 60.0, "near_clip": 0.01, "far_clip": 100.0,
            "to_world": T.look_at([0.3, 0.4, 6.0], [0.0, 0.0, 0.0], [0, 1, 0]),
            "film": {"type": "hdrfilm", "width": 16, "height": 16, "rfilter": {"type": "tent"}}}


def _light(filename, radiance):
    return {"type": "obj", "filename": filename, "bsdf": {"type": "ref", "id": "grey"},
            "emitter": {"type": "area", "radiance": {"type": "rgb", "value": radiance}}}


def _write_obj(path, verts, faces):
    with open(path, "w") as fh:
        for p in verts:
            fh.write("v %r %r %r\n" % tuple(float(x) for x in p))
        for t in faces:
            fh.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


_SCENES = {}


def _load(key, dirname, files, lights):
    from mtx.mitsuba_dict import scene_from_dict

    key = (str(dirname),) + key
    if key not in _SCENES:
        for name, (v, f) in files.items():
            _write_obj(os.path.join(dirname, name), v, f)
        d = {"type": "scene", "sensor": _sensor(),
             "grey": {"type": "diffuse", "reflectance": {"type": "rgb", "value": 0.5}}}
        d.update(lights)
        _SCENES[key] = scene_from_dict(d, base_dir=str(dirname))
    return _SCENES[key]


def strip_mesh(n, seed=1):
    """A strip of n unequal triangles in the plane z = 0 (fixed seed)."""
    rng = np.random.default_rng(seed + n)
    m = n + 2
    x = np.cumsum(rng.uniform(0.01, 0.05, m)) - 0.03 * m / 2
    y = np.where(np.arange(m) % 2 == 0, -1.0, 1.0) * rng.uniform(0.2, 1.0, m)
    v = np.stack([x, y, np.zeros(m)], 1)
    f = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1)
    return v, f


def strip_scene(dirname, n):
    return _load(("strip", n), dirname, {"strip_%d.obj" % n: strip_mesh(n)}, {"strip": _light("strip_%d.obj" % n, [1.0, 2.0, 3.0])})


def strip_moved(scene):
    """Every vertex of the strip moved: a stretch, a shear and a fixed jitter."""
    v = base_vertices(scene).astype(np.float64)
    rng = np.random.default_rng(5)
    out = v.copy()
    out[:, 0] = 1.25 * v[:, 0] + 0.2 * v[:, 1]
    out[:, 1] = 0.8 * v[:, 1] + 0.01 * rng.uniform(-1, 1, len(v))
    out[:, 2] = 0.05 * v[:, 0]
    return out.astype(np.float32)


def order_mesh(n_slivers=512, mirror=False):
    """Triangles of area 1 (legs 2 x 1), 2^-24 (legs 2^-11 x 2^-12) and
    n_slivers of 2^-60 (legs 2^-29 x 2^-30), in this file order, right angle
    at the first vertex, in the plane z = 0; every coordinate and area is
    exact in fp32. The large ones lie at smaller x than the slivers (mirror:
    larger), for the leaf order to keep them first."""
    tris = [(-4.0, 2.0, 1.0), (-1.0, 2.0 ** -11, 2.0 ** -12)]
    tris += [(j * 2.0 ** -17, 2.0 ** -29, 2.0 ** -30) for j in range(n_slivers)]
    v, f = [], []
    for x0, a, b in tris:
        s = -1.0 if mirror else 1.0
        v += [(s * x0, 0.0, 0.0), (s * (x0 + a), 0.0, 0.0), (s * x0, b, 0.0)]
        f.append((len(v) - 3, len(v) - 2, len(v) - 1))
    return np.array(v), np.array(f)


def order_free(pmf):
    """The exactness predicate of a double prefix sum over fp32 areas
    (mtx.h mtx_scene_update_vertices), restated: M + 1 + ceil(log2 n) - m <= 53."""
    a = np.asarray(pmf, np.float64)
    nz = a[a > 0]
    M = int(np.floor(np.log2(nz.max())))
    m = max(int(np.floor(np.log2(nz.min()))), -126) - 23
    return M + 1 + int(np.ceil(np.log2(len(a)))) - m <= 53


def blocked_cdf(pmf, block):
    """An fp32 cdf from a blocked double summation: block totals first (each
    summed on its own), their prefix, then the prefix inside each block."""
    a = np.asarray(pmf, np.float64)
    out = np.zeros(len(a))
    tot = 0.0
    for s in range(0, len(a), block):
        out[s: s + block] = tot + np.cumsum(a[s: s + block])
        tot = tot + a[s: s + block].sum()
    return out.astype(np.float32)


def order_premise(pmf):
    """True when the sequential double cumsum of `pmf` and some blocked one
    differ in an fp32 cdf entry, and the exactness predicate is false."""
    seq = np.cumsum(np.asarray(pmf, np.float64)).astype(np.float32)
    differs = any(not np.array_equal(seq, blocked_cdf(pmf, b)) for b in (64, 256))
    return differs and not order_free(pmf)


def order_scene(dirname, n_slivers=512, with_patch=False):
    """The one-emitter scene of order_mesh whose entry order (the loader's
    leaf order) satisfies order_premise -- mirrored if the plain one does not;
    with_patch adds mesh_emitter_cases' patch as a second light."""
    for mirror in (False, True):
        name = "order_%d_%d.obj" % (n_slivers, mirror)
        lights = {"order": _light(name, [2.0, 1.0, 0.5])}
        if with_patch:
            if not os.path.exists(os.path.join(dirname, "patch.obj")):
                mc.write_meshes(dirname)
            lights["patch"] = _light("patch.obj", [1.0, 2.0, 3.0])
        s = _load(("order", n_slivers, mirror, with_patch), dirname, {name: order_mesh(n_slivers, mirror)}, lights)
        pmf, _, _ = mc.mesh_tables(s, 0)
        if order_premise(pmf):
            return s
    raise AssertionError("no leaf order of the order-sensitive mesh keeps the large areas first")


def order_moved(scene):
    """Every vertex moved by a lattice vector and mirrored in y: the areas
    and the entry order stay, every vertex changes."""
    v = base_vertices(scene)
    first = shape_vertices(scene, 0)
    v[first] = v[first] * np.array([1.0, -1.0, 1.0], np.float32) + np.array([0.0, 0.0, 0.5], np.float32)
    return v
