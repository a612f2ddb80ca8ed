"""The mesh-emitter fixture scene shared by test_mesh_emitters.py (CPU) and
test_mesh_emitters_gpu.py: a closed two-sided diffuse box [-2, 2]^3 with the
camera inside and three emitters,

  (a) ``steps.obj``: six right triangles in the plane y = 1.5, facing down,
      whose legs are powers of two, so their areas are 2^-2 .. 2^-7 -- distinct
      powers of two, every coordinate, area and cdf entry exact in fp32 -- plus
      one zero-area (collinear) triangle;
  (b) ``patch.obj``: a jittered 11 x 9 grid on the wall x = -1.75, 198 unequal
      triangles facing +x (not a power of two; eight bisection steps, which
      the lanes of a wave take differently);
  (c) a rectangle emitter on the wall x = +1.75 facing -x.

Variants: ``env`` adds a constant environment (mesh, rectangle and environment
indices mix in the uniform pick), ``mesh`` drops the rectangle, ``single``
replaces (a) by a one-triangle mesh light. (b) is in every variant. The same
scene can be written as a Mitsuba dictionary and as XML."""
import os

import numpy as np
from test_mitsuba_dict import T

# (leg along x, leg along z, x0) of the six triangles of (a); areas leg_x * leg_z / 2
STEPS = [(1.0, 0.5, -1.75), (0.5, 0.5, -0.625), (0.5, 0.25, 0.0), (0.25, 0.25, 0.625), (0.25, 0.125, 1.0),
         (0.125, 0.125, 1.375)]
STEPS_Y, STEPS_Z = 1.5, -0.5
PATCH_NY, PATCH_NZ = 11, 9
RADIANCE = {"steps": [6.0, 5.0, 4.0], "patch": [1.0, 2.0, 3.0], "rect": [4.0, 3.0, 5.0]}
SKY = [0.2, 0.3, 0.4]
VARIANTS = ("full", "env", "mesh", "single")


def write_meshes(dirname):
    """steps.obj, one.obj and patch.obj into `dirname`."""
    v, f = [], []
    for k, (ax, bz, x0) in enumerate(STEPS):
        if k == 3:  # the zero-area triangle, in the middle of the file
            v += [(0.0, STEPS_Y, 1.0), (0.5, STEPS_Y, 1.0), (1.0, STEPS_Y, 1.0)]
            f.append((len(v) - 2, len(v) - 1, len(v)))
        v += [(x0, STEPS_Y, STEPS_Z), (x0 + ax, STEPS_Y, STEPS_Z), (x0, STEPS_Y, STEPS_Z + bz)]
        f.append((len(v) - 2, len(v) - 1, len(v)))  # cross(e1, e2) = (0, -ax bz, 0): faces down
    _write_obj(os.path.join(dirname, "steps.obj"), v, f)
    _write_obj(os.path.join(dirname, "one.obj"), [(-0.5, STEPS_Y, -0.5), (0.5, STEPS_Y, -0.5), (-0.5, STEPS_Y, 0.5)],
               [(1, 2, 3)])
    rng = np.random.default_rng(7)
    ny, nz = PATCH_NY + 1, PATCH_NZ + 1
    dy, dz = 2.0 / PATCH_NY, 2.0 / PATCH_NZ
    v, f = [], []
    for i in range(ny):
        for j in range(nz):
            jx, jy, jz = rng.uniform(-1, 1, 3) * (0.02, 0.3 * dy, 0.3 * dz)
            v.append((-1.75 + jx, -1.0 + i * dy + jy, -1.0 + j * dz + jz))
    for i in range(PATCH_NY):
        for j in range(PATCH_NZ):
            a, b, c, d = i * nz + j, (i + 1) * nz + j, (i + 1) * nz + j + 1, i * nz + j + 1
            f += [(a + 1, b + 1, c + 1), (a + 1, c + 1, d + 1)]  # (y step) x (z step) = +x
    _write_obj(os.path.join(dirname, "patch.obj"), v, f)


def _write_obj(path, verts, faces):
    with open(path, "w") as fh:
        for p in verts:
            fh.write("v %r %r %r\n" % tuple(float(x) for x in p))
        for t in faces:
            fh.write("f %d %d %d\n" % t)


def _sensor(width, height):
    return {"type": "perspective", "fov": 70.0, "fov_axis": "x", "near_clip": 0.01, "far_clip": 100.0,
            "to_world": T.look_at([0.0, -0.2, 1.9], [0.0, 0.3, 0.0], [0, 1, 0]),
            "film": {"type": "hdrfilm", "width": width, "height": height, "rfilter": {"type": "tent"}}}


RECT_TO_WORLD = T().translate([1.75, 0.0, 0.0]).rotate([0, 1, 0], -90).scale(0.5)
BOX_TO_WORLD = T().scale(2.0)


def scene_dict(variant="full", width=32, height=18):
    assert variant in VARIANTS
    d = {
        "type": "scene",
        "sensor": _sensor(width, height),
        "wall": {"type": "twosided", "nested": {"type": "diffuse", "reflectance": {"type": "rgb", "value": 0.6}}},
        "lamp": {"type": "diffuse", "reflectance": {"type": "rgb", "value": 0.3}},
        "box": {"type": "cube", "to_world": BOX_TO_WORLD, "bsdf": {"type": "ref", "id": "wall"}},
        "steps": {"type": "obj", "filename": "one.obj" if variant == "single" else "steps.obj",
                  "bsdf": {"type": "ref", "id": "lamp"},
                  "emitter": {"type": "area", "radiance": {"type": "rgb", "value": RADIANCE["steps"]}}},
        "patch": {"type": "obj", "filename": "patch.obj", "bsdf": {"type": "ref", "id": "lamp"},
                  "emitter": {"type": "area", "radiance": {"type": "rgb", "value": RADIANCE["patch"]}}},
    }
    if variant != "mesh":
        d["rect"] = {"type": "rectangle", "to_world": RECT_TO_WORLD, "bsdf": {"type": "ref", "id": "lamp"},
                     "emitter": {"type": "area", "radiance": {"type": "rgb", "value": RADIANCE["rect"]}}}
    if variant == "env":
        d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": SKY}}
    return d


def scene_xml(variant="full", width=32, height=18):
    """The same scene as Mitsuba XML."""
    def mat(t):
        return '<transform name="to_world"><matrix value="%s"/></transform>' % " ".join(
            repr(float(x)) for x in np.asarray(t.matrix).reshape(-1))

    def rgb(name, v):
        return '<rgb name="%s" value="%s"/>' % (name, ", ".join(repr(float(x)) for x in v))

    def light(sid, typ, body, key):
        return ('<shape type="%s" id="%s">%s<ref id="lamp"/><emitter type="area">%s</emitter></shape>'
                % (typ, sid, body, rgb("radiance", RADIANCE[key])))
    s = _sensor(width, height)
    out = ['<scene version="3.0.0">',
           '<sensor type="perspective"><float name="fov" value="70"/><string name="fov_axis" value="x"/>'
           '<float name="near_clip" value="0.01"/><float name="far_clip" value="100"/>' + mat(s["to_world"])
           + '<film type="hdrfilm"><integer name="width" value="%d"/><integer name="height" value="%d"/>'
             '<rfilter type="tent"/></film></sensor>' % (width, height),
           '<bsdf type="twosided" id="wall"><bsdf type="diffuse">' + rgb("reflectance", [0.6] * 3) + '</bsdf></bsdf>',
           '<bsdf type="diffuse" id="lamp">' + rgb("reflectance", [0.3] * 3) + '</bsdf>',
           '<shape type="cube" id="box">' + mat(BOX_TO_WORLD) + '<ref id="wall"/></shape>',
           light("steps", "obj", '<string name="filename" value="%s"/>'
                 % ("one.obj" if variant == "single" else "steps.obj"), "steps"),
           light("patch", "obj", '<string name="filename" value="patch.obj"/>', "patch")]
    if variant != "mesh":
        out.append(light("rect", "rectangle", mat(RECT_TO_WORLD), "rect"))
    if variant == "env":
        out.append('<emitter type="constant">' + rgb("radiance", SKY) + '</emitter>')
    out.append("</scene>")
    return "\n".join(out)


_CACHE = {}


def build(dirname, variant="full", width=32, height=18):
    """The mtx Scene of a variant (cached per directory, variant and film)."""
    from mtx.mitsuba_dict import scene_from_dict

    key = (dirname, variant, width, height)
    if key not in _CACHE:
        if not os.path.exists(os.path.join(dirname, "patch.obj")):
            write_meshes(dirname)
        _CACHE[key] = scene_from_dict(scene_dict(variant, width, height), base_dir=dirname)
    return _CACHE[key]


def emitter_of(scene, shape_name, variant="full"):
    """Emitter index of a named shape (shapes keep the dictionary's order)."""
    order = [k for k in scene_dict(variant) if k in ("box", "steps", "patch", "rect")]
    return int(scene.shapes[order.index(shape_name)].emitter)


def mesh_tables(scene, em):
    """(pmf, cdf, prim) of mesh emitter `em` from the scene's tables."""
    m = scene.emitters[em].mesh
    t = np.asarray(scene.tables)[m["offset"]: m["offset"] + 3 * m["count"]]
    n = m["count"]
    return t[:n], t[n: 2 * n], t[2 * n:].view(np.uint32)


# ------------------------------------------------- damaged mesh records --
# One inconsistency each in the "patch" record of the "full" variant:
# corrupt(sc, em, t, n, box_tri) with t the record's 3 n table floats (pmf | cdf
# | prim), box_tri a triangle of the box. mtx_scene_upload refuses every one
# (tests/test_scene_check.py on the host, test_mesh_emitters_gpu.py through a
# context).
def _words(sc, em, **change):
    m = sc.emitters[em].mesh
    m.update(change)
    sc.emitters[em].set_mesh(m["offset"], m["count"], m["valid_lo"], m["valid_hi"], m["sum"], m["norm"])


def _bad_range(sc, em, t, n, box_tri):
    _words(sc, em, offset=sc.n_tables - 3 * n + 1)


def _bad_triangle_index(sc, em, t, n, box_tri):
    t[2 * n + 3] = np.array([sc.n_tris], np.uint32).view(np.float32)[0]


def _foreign_triangle(sc, em, t, n, box_tri):
    t[2 * n + 3] = np.array([box_tri], np.uint32).view(np.float32)[0]


def _triangle_twice(sc, em, t, n, box_tri):
    t[2 * n + 3] = t[2 * n + 4]


def _decreasing_cdf(sc, em, t, n, box_tri):
    t[n + 10] = t[n + 8]
    t[n + 9] = np.nextafter(t[n + 10], np.float32(np.inf))


def _zero_sum(sc, em, t, n, box_tri):
    t[: 2 * n] = 0
    _words(sc, em, sum=0.0)


def _missing_triangle(sc, em, t, n, box_tri):
    # the last entry dropped: the shape has a triangle the record does not list
    pmf, cdf, prim = t[:n].copy(), t[n: 2 * n].copy(), t[2 * n: 3 * n].copy()
    m = n - 1
    t[:m], t[m: 2 * m], t[2 * m: 3 * m] = pmf[:m], cdf[:m], prim[:m]
    _words(sc, em, count=m, valid_hi=m - 1, sum=float(cdf[m - 1]), norm=float(np.float32(1) / cdf[m - 1]))


MESH_RECORD_CORRUPTIONS = [(_bad_range, "table range"), (_bad_triangle_index, "names triangle"),
                           (_foreign_triangle, "another emitter or none"), (_triangle_twice, "listed twice"),
                           (_decreasing_cdf, "decreasing cdf"), (_zero_sum, "positive finite sum"),
                           (_missing_triangle, "does not list")]


def with_corrupt_patch(good, corrupt):
    """A copy of the "full" scene `good` with its own tables and emitter
    records, the patch's record damaged by `corrupt`."""
    import copy

    em = emitter_of(good, "patch")
    sc = copy.copy(good)
    sc.tables = np.array(good.tables, np.float32)
    sc.emitters = type(good.emitters).from_buffer_copy(bytes(good.emitters))
    m = sc.emitters[em].mesh
    n = m["count"]
    box_tri = int(np.flatnonzero(np.asarray(good.tri_shape) == 0)[0])
    corrupt(sc, em, sc.tables[m["offset"]: m["offset"] + 3 * n], n, box_tri)
    return sc
