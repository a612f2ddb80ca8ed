"""Float64 numpy transcriptions of the two light-path functions of mtx_core
(interaction.h sample_emitter_ray, camera_sample_direction), the scenes they
are tested on, and their fp32 error bounds. Shared by test_blocks_light.py
(the host probe, no GPU) and test_blocks_light_gpu.py (the kernels).

The transcriptions read the scene's arrays (fp32 data, widened to float64)
and restate the formulas from their description in include/mtx.h and DESIGN.md
§3; they share no code with mtx_core. Every operation is float64, so the
transcription's own rounding (2^-53) is nothing beside the bounds.

Bounds. E = 2^-24 is the unit roundoff of fp32: one correctly rounded
operation (+ - * / sqrt fma) returns its exact result times (1 + d), |d| <= E.
Each bound below counts the roundings on the chain that produces the output
and propagates them to first order through that chain's partial derivatives,
per lane, because three steps amplify: the reuse of a sample inside an
interval of width w (error / w), sqrt near 0 (error / (2 sqrt)), and the
division by a small cosine. A bound is derived here and never measured on the
code under test. A discrete output (the emitter index, the triangle, valid,
the side of spawn_ray's offset) is compared only where the float64 value that
decides it is further from its threshold than that value's bound; the other
lanes are `ambiguous` and are counted, so a test can assert they are few.
"""
import numpy as np

E = 2.0 ** -24
RAY_EPS = 1500.0 * 2.0 ** -24
LARGEST = float(np.finfo(np.float32).max)
# CEPHES sinf / cosf (the coefficient set mtx_core/dmath.h names) publish a
# peak error of 1.2e-7 = 2.02 E over |x| < 4096; 3 E leaves the 3-part argument
# reduction one rounding.
SINCOS_E = 3.0


# ----------------------------------------------------------------- scenes --
_SCENES = {}


def scene(kind, dirname=None):
    """'furnace': the six-rectangle white furnace; 'lattice': the lattice
    ``emit`` scene (18 mesh emitters; needs `dirname` for its meshes); 'sky':
    the sky furnace of tests/test_environment.py (the environment alone)."""
    if kind not in _SCENES:
        if kind == "furnace":
            from mtx.scene import Scene
            from test_gpu_convergence import furnace_spec

            _SCENES[kind] = Scene.bedroom(spec=furnace_spec(0.5, 1.5, res=32))
        elif kind == "lattice":
            import lattice_cases

            _SCENES[kind] = lattice_cases.build(dirname, "emit")
        else:
            from mtx.mitsuba_dict import scene_from_dict

            _SCENES[kind] = scene_from_dict(sky_furnace_dict(32, 32, albedo=0.8))
    return _SCENES[kind]


KINDS = ("furnace", "lattice", "sky")


# ------------------------------------------------- scene dictionaries --
# 4x4 to_world matrices (the dictionary loader takes them as they are).
def translate(v):
    m = np.eye(4)
    m[:3, 3] = v
    return m


def scale(v):
    return np.diag(list(np.broadcast_to(np.asarray(v, np.float64), 3)) + [1.0])


def rotate(axis, angle):
    """Rodrigues' rotation by `angle` degrees. The sine and cosine of a
    multiple of 90 degrees are exact: cos 90 = 6e-17 would otherwise stay in
    the matrix and in an emitter's normal, and a path_test vertex on such a
    light samples the light's own plane at a grazing cosine of 1e-17 or less,
    where the solid-angle pdf exceeds 1.8e19, its square overflows and the
    power heuristic of path-mis.py:9-15 returns inf / inf (about one path in
    a million, also on the CPU oracle; DESIGN.md "Known defects")."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = np.cos(np.radians(angle)), np.sin(np.radians(angle))
    c, s = (0.0 if abs(x) < 1e-12 else float(np.sign(x)) if abs(abs(x) - 1.0) < 1e-12 else x for x in (c, s))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + s * K + (1 - c) * K @ K
    return m


def look_at(origin, target, up):
    o, t, u = (np.asarray(x, np.float64) for x in (origin, target, up))
    d = (t - o) / np.linalg.norm(t - o)
    left = np.cross(u, d)
    left /= np.linalg.norm(left)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, np.cross(d, left), d, o
    return m


def _sensor(origin, target, fov, width, height, **kw):
    return dict({"type": "perspective", "fov": fov, "near_clip": 0.01, "far_clip": 100.0,
                 "to_world": look_at(origin, target, [0, 1, 0]),
                 "film": {"type": "hdrfilm", "width": width, "height": height, "rfilter": {"type": "box"}}}, **kw)


def _rgb(v):
    return {"type": "rgb", "value": v}


def sky_furnace_dict(width, height, albedo=1.0, sky=1.0):
    """The sky furnace of tests/test_environment.py, restated: a diffuse cube
    under a constant environment."""
    return {
        "type": "scene",
        "sensor": {"type": "perspective", "fov": 40.0, "to_world": look_at([0, 0, 4], [0, 0, 0], [0, 1, 0]),
                   "film": {"type": "hdrfilm", "width": width, "height": height}},
        "cube": {"type": "cube", "to_world": rotate([0, 1, 0], 30) @ rotate([1, 0, 0], 20) @ scale(0.6),
                 "bsdf": {"type": "diffuse", "reflectance": _rgb(albedo)}},
        "sky": {"type": "constant", "radiance": _rgb(sky)},
    }


def cornell_dict(width, height):
    """Mitsuba 3's cornell_box() dictionary, restated: five rectangles, two
    cubes, three diffuse BSDFs, one area light."""
    def ref(i):
        return {"type": "ref", "id": i}

    return {
        "type": "scene",
        "sensor": _sensor([0, 0, 3.9], [0, 0, 0], 39.3077, width, height, fov_axis="smaller", near_clip=0.001),
        "white": {"type": "diffuse", "reflectance": _rgb([0.885809, 0.698859, 0.666422])},
        "green": {"type": "diffuse", "reflectance": _rgb([0.105421, 0.37798, 0.076425])},
        "red": {"type": "diffuse", "reflectance": _rgb([0.570068, 0.0430135, 0.0443706])},
        "light": {"type": "rectangle",
                  "to_world": translate([0.0, 0.99, 0.01]) @ rotate([1, 0, 0], 90) @ scale([0.23, 0.19, 0.19]),
                  "bsdf": ref("white"), "emitter": {"type": "area", "radiance": _rgb([18.387, 13.9873, 6.75357])}},
        "floor": {"type": "rectangle", "to_world": translate([0.0, -1.0, 0.0]) @ rotate([1, 0, 0], -90),
                  "bsdf": ref("white")},
        "ceiling": {"type": "rectangle", "to_world": translate([0.0, 1.0, 0.0]) @ rotate([1, 0, 0], 90),
                    "bsdf": ref("white")},
        "back": {"type": "rectangle", "to_world": translate([0.0, 0.0, -1.0]), "bsdf": ref("white")},
        "green-wall": {"type": "rectangle", "to_world": translate([1.0, 0.0, 0.0]) @ rotate([0, 1, 0], -90),
                       "bsdf": ref("green")},
        "red-wall": {"type": "rectangle", "to_world": translate([-1.0, 0.0, 0.0]) @ rotate([0, 1, 0], 90),
                     "bsdf": ref("red")},
        "small-box": {"type": "cube", "to_world": translate([0.335, -0.7, 0.38]) @ rotate([0, 1, 0], -17) @ scale(0.3),
                      "bsdf": ref("white")},
        "large-box": {"type": "cube",
                      "to_world": translate([-0.33, -0.4, -0.28]) @ rotate([0, 1, 0], 18.25) @ scale([0.3, 0.61, 0.3]),
                      "bsdf": ref("white")},
    }


def glass_dict():
    """A closed smooth dielectric cube between a small ceiling light and a
    diffuse floor; the camera looks down at the floor and does not see the
    cube (a pinhole cannot be connected through a delta surface, so a pixel
    that looked through the glass would be black for a particle tracer). The
    floor under the cube is lit through two refractions."""
    return {
        "type": "scene",
        "sensor": _sensor([0.0, 0.45, 1.6], [0.0, 0.0, 0.0], 40.0, 32, 32),
        "grey": {"type": "diffuse", "reflectance": _rgb(0.6)},
        "glass": {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0},
        "floor": {"type": "rectangle", "to_world": rotate([1, 0, 0], -90) @ scale(2.0),
                  "bsdf": {"type": "ref", "id": "grey"}},
        "cube": {"type": "cube", "to_world": translate([0.0, 1.0, 0.0]) @ scale(0.3),
                 "bsdf": {"type": "ref", "id": "glass"}},
        "light": {"type": "rectangle", "to_world": translate([0.0, 2.0, 0.0]) @ rotate([1, 0, 0], 90) @ scale(0.5),
                  "bsdf": {"type": "ref", "id": "grey"},
                  "emitter": {"type": "area", "radiance": _rgb([8.0, 6.0, 4.0])}},
    }


def immersed_dict():
    """The camera and a diffuse floor inside a closed smooth dielectric cube,
    the light outside above it: every contributing light path crosses exactly
    one interface, so the radiance scale eta^2 of a refraction does not cancel
    as it does on the way in and out of the cube of glass_dict. path_test
    reaches the light by BSDF sampling alone (the shadow ray of its emitter
    sample stops at the glass), hence the large light."""
    return {
        "type": "scene",
        "sensor": _sensor([0.0, 0.6, 0.7], [0.0, -0.5, 0.0], 50.0, 32, 32),
        "grey": {"type": "diffuse", "reflectance": _rgb(0.6)},
        "glass": {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0},
        "floor": {"type": "rectangle", "to_world": translate([0.0, -0.5, 0.0]) @ rotate([1, 0, 0], -90) @ scale(0.9),
                  "bsdf": {"type": "ref", "id": "grey"}},
        "cube": {"type": "cube", "bsdf": {"type": "ref", "id": "glass"}},
        "light": {"type": "rectangle", "to_world": translate([0.0, 1.5, 0.0]) @ rotate([1, 0, 0], 90) @ scale(1.5),
                  "bsdf": {"type": "ref", "id": "grey"},
                  "emitter": {"type": "area", "radiance": _rgb([2.0, 1.5, 1.0])}},
    }


def bumpy_dict(dirname, n=6, tilt=0.45, seed=11):
    """A diffuse sheet of n x n quads in the plane y = 0 whose vertex normals
    are tilted at random (tangent components up to `tilt` before
    normalisation, about 30 degrees), a diffuse cube standing on it and a
    rectangle light above: the shading-normal correction of the adjoint BSDF
    differs from 1 at every hit of the sheet. Nothing lies below the sheet
    and there is no environment, so a direction on different sides of the two
    normals carries nothing in either estimator (it leaves downwards for
    good), and the particle tracer's light-leak mask removes no light that
    path_test keeps. Writes bumpy.obj into `dirname`."""
    import os

    rng = np.random.default_rng(seed)
    g = np.linspace(-1.5, 1.5, n + 1)
    with open(os.path.join(dirname, "bumpy.obj"), "w") as fh:
        for z in g:
            for x in g:
                fh.write("v %r 0.0 %r\n" % (float(x), float(z)))
                t = rng.uniform(-tilt, tilt, 2)
                fh.write("vn %r 1.0 %r\n" % (float(t[0]), float(t[1])))
        for j in range(n):
            for i in range(n):
                a, b, c, d = (j * (n + 1) + i + 1, j * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 2,
                              (j + 1) * (n + 1) + i + 1)
                fh.write("f %d//%d %d//%d %d//%d\n" % (a, a, c, c, b, b))  # wound for a geometric normal +y
                fh.write("f %d//%d %d//%d %d//%d\n" % (a, a, d, d, c, c))
    return {
        "type": "scene",
        "sensor": _sensor([0.0, 1.4, 2.6], [0.0, 0.0, 0.0], 45.0, 32, 32),
        "grey": {"type": "diffuse", "reflectance": _rgb(0.7)},
        "sheet": {"type": "obj", "filename": "bumpy.obj", "bsdf": {"type": "ref", "id": "grey"}},
        "box": {"type": "cube", "to_world": translate([-0.5, 0.26, -0.3]) @ rotate([0, 1, 0], 25) @ scale(0.25),
                "bsdf": {"type": "ref", "id": "grey"}},
        "light": {"type": "rectangle", "to_world": translate([0.4, 1.8, 0.0]) @ rotate([1, 0, 0], 90) @ scale(0.4),
                  "bsdf": {"type": "ref", "id": "grey"},
                  "emitter": {"type": "area", "radiance": _rgb([6.0, 5.0, 4.0])}},
    }


def connectable_bedroom_spec(face_normals=False):
    """The bedroom's spec with the lobes a particle tracer cannot connect
    through replaced in this copy: the lamp glass (roughdielectric, refused)
    becomes rough plastic, the mirror and the polished steel (smooth
    conductors) become rough conductors of alpha 0.1, the smooth glass
    (window pane, vases) becomes diffuse, and the one ``mask`` wrapper (its
    null lobe lets a camera ray pass straight through) leaves its nested
    BSDF. A pinhole is not connected through a delta or null lobe, and the
    connection's shadow ray stops at such a surface, so path_test would keep
    the paths camera - delta - ... that no particle tracer has. Vertex
    normals, textures, both plastics and the rough conductors stay as they
    are. `face_normals` shades every mesh with its geometric normals."""
    import copy

    from mtx.scene import load_bedroom_spec

    spec = copy.deepcopy(load_bedroom_spec())

    def become(b, **new):
        keep = {k: b[k] for k in ("id",) if k in b}
        b.clear()
        b.update(keep, **new)

    def swap(b):
        if b["type"] == "mask":
            become(b, **{k: v for k, v in b["nested"].items() if k != "id"})
            swap(b)
        elif b["type"] == "twosided":
            swap(b["nested"])
        elif b["type"] == "roughdielectric":
            become(b, type="roughplastic", alpha=b.get("alpha", 0.1), distribution=b.get("distribution", "beckmann"),
                   int_ior=b.get("int_ior", 1.5), ext_ior=b.get("ext_ior", 1.0), diffuse_reflectance=[0.6, 0.6, 0.6])
        elif b["type"] == "conductor":
            b.update(type="roughconductor", alpha=0.1, distribution="ggx")
        elif b["type"] == "dielectric":
            become(b, type="diffuse", reflectance=[0.5, 0.5, 0.5])

    for b in spec["bsdfs"].values():
        swap(b)
    for sd in spec["shapes"]:
        if "bsdf_inline" in sd:
            swap(sd["bsdf_inline"])
        if face_normals:
            sd["face_normals"] = True
    return spec


def samples(n, seed):
    """(4, n) float32 uniform samples: u_pos, u_dir."""
    return np.random.default_rng(seed).random((4, n), dtype=np.float32)


# ------------------------------------------------------- emitter geometry --
def emitter_count(sc):
    return len(sc.emitters) + (0 if getattr(sc, "env_radiance", None) is None else 1)


def env_sphere64(sc):
    """Centre and radius of the bounding sphere of the vertices' box, the
    radius grown by a ray epsilon (mtx.h, the constant environment)."""
    v = np.asarray(sc.vpos, np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    c = (lo + hi) * 0.5
    return c, max(RAY_EPS, np.linalg.norm(c - lo) * (1.0 + RAY_EPS))


def mesh_arrays(sc, e):
    """(pmf, cdf, prim, lo, hi, sum, norm) of mesh emitter e, float64."""
    m = sc.emitters[e].mesh
    n, off = m["count"], m["offset"]
    t = np.asarray(sc.tables)[off: off + 3 * n]
    return (t[:n].astype(np.float64), t[n: 2 * n].astype(np.float64), t[2 * n:].view(np.uint32), m["valid_lo"],
            m["valid_hi"], float(m["sum"]), float(m["norm"]))


def tri_points(sc, prim):
    vid = np.asarray(sc.tri_vidx).reshape(-1, 3)[prim]
    v = np.asarray(sc.vpos, np.float64).reshape(-1, 3)
    return v[vid[..., 0]], v[vid[..., 1]], v[vid[..., 2]]


def emitter_area_centroid(sc, e):
    """Area and area-weighted centroid of area emitter e, float64 from the
    vertices (a mesh) or from the rectangle's two half-edge columns."""
    em = sc.emitters[e]
    if em.is_mesh:
        p0, p1, p2 = tri_points(sc, mesh_arrays(sc, e)[2])
        a = 0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1)
        return a.sum(), ((p0 + p1 + p2) / 3.0 * a[:, None]).sum(0) / a.sum()
    c0, c1 = np.array(em.col0, np.float64), np.array(em.col1, np.float64)
    return 4.0 * np.linalg.norm(np.cross(c0, c1)), np.array(em.center, np.float64)


def radiance(sc, e):
    if e == len(sc.emitters):
        return np.array(sc.env_radiance, np.float64)
    return np.array(sc.emitters[e].radiance, np.float64)


# ---------------------------------------------------- sample_emitter_ray --
def _frame(n):
    """coordinate_system() of Duff et al. 2017 around unit normals (N, 3): s, t."""
    sign = np.where(np.signbit(n[:, 2]), -1.0, 1.0)
    a = -1.0 / (sign + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    s = np.stack([sign * n[:, 0] * n[:, 0] * a + 1.0, sign * b, -sign * n[:, 0]], 1)
    t = np.stack([b, n[:, 1] * n[:, 1] * a + sign, -n[:, 1]], 1)
    return s, t


def _cosine_hemisphere(u):
    """Shirley-Chiu concentric disk, z = sqrt(1 - r^2); (local (N, 3), bound (N,))."""
    x, y = 2.0 * u[0] - 1.0, 2.0 * u[1] - 1.0
    q13 = np.abs(x) < np.abs(y)
    r = np.where(q13, y, x)
    rp = np.where(q13, x, y)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = 0.25 * np.pi * rp / r
    phi = np.where(q13, 0.5 * np.pi - phi, phi)
    phi = np.where((x == 0) & (y == 0), 0.0, phi)
    px, py = r * np.cos(phi), r * np.sin(phi)
    z2 = 1.0 - (px * px + py * py)
    z = np.sqrt(np.maximum(z2, 0.0))
    # x, y: one fma (E each, |x| <= 1). phi: three roundings relative (|phi| < 2) and the argument's own
    # error moves sin / cos by as much: 3 * 2 E + E. sin / cos: SINCOS_E. The product r * cs: the sum of
    # those times |r| <= 1, plus r's E, plus its own rounding.
    d_xy = (1.0 + 7.0 + SINCOS_E + 1.0) * E
    # z^2 = 1 - fma(y, y, x x): 2 |p| d_xy from the inputs, three roundings on values <= 1; the square
    # root halves the relative error: dz = d(z^2) / (2 z) + E, and never more than sqrt(d(z^2)) + E
    # (at z -> 0, where sqrt(max(., 0)) is continuous but not differentiable).
    d_z2 = 2.0 * (np.abs(px) + np.abs(py)) * d_xy + 3.0 * E
    d_z = np.minimum(d_z2 / np.maximum(2.0 * z, 1e-300), np.sqrt(d_z2)) + E
    return np.stack([px, py, z], 1), d_xy, d_z


def emitter_ray_f64(sc, u):
    """The float64 value of sample_emitter_ray for the (4, N) float32 samples
    u. Returns a dict of arrays: o, d, weight, p, n (N, 3), maxt, emitter, and
    per lane the bounds b_p, b_n, b_d, b_o (absolute, every component),
    `ambiguous` (a discrete decision within its bound) and `side_ambiguous`
    (only the side of spawn_ray's offset is: o is not compared)."""
    u = np.asarray(u, np.float32).astype(np.float64)
    N = u.shape[1]
    count = emitter_count(sc)
    out = {k: np.zeros((N, 3)) for k in ("o", "d", "weight", "p", "n")}
    out["maxt"] = np.zeros(N)
    out["emitter"] = np.full(N, -1, np.int64)
    for k in ("b_p", "b_n", "b_d", "b_o"):
        out[k] = np.zeros(N)
    out["ambiguous"] = np.zeros(N, bool)
    out["side_ambiguous"] = np.zeros(N, bool)
    if count == 0:
        return out
    n_area = len(sc.emitters)
    scaled = u[0] * count
    index = np.minimum(scaled.astype(np.int64), count - 1)
    ux = scaled - index
    # scaled rounds once (<= count E); an index decision is ambiguous within that of an integer. The
    # subtraction of the integer part is exact or rounds once on a value < 1.
    d_ux = (count + 1.0) * E
    out["ambiguous"] |= np.abs(scaled - np.round(scaled)) <= count * E
    out["emitter"] = index
    local, d_xy, d_z = _cosine_hemisphere(u[2:4])
    for e in range(count):
        sel = np.flatnonzero(index == e)
        if len(sel) == 0:
            continue
        x, y = ux[sel], u[1, sel]
        rad = radiance(sc, e)
        if e == n_area:  # the environment: a point of the bounding sphere, the inward normal
            c, r = env_sphere64(sc)
            z = 1.0 - 2.0 * y
            rr = np.sqrt(np.maximum(1.0 - z * z, 0.0))
            phi = 2.0 * np.pi * x
            v0 = np.stack([rr * np.cos(phi), rr * np.sin(phi), z], 1)
            # z: one fma. r^2 = fma(-z, z, 1): 2 |z| E + E; sqrt as above. phi: one rounding of a value
            # < 2 pi (7 E) plus 2 pi d_ux from the reused sample, then the sincos kernel.
            d_r2 = 2.0 * np.abs(z) * E + E
            d_rr = np.minimum(d_r2 / np.maximum(2.0 * rr, 1e-300), np.sqrt(d_r2)) + E
            d_v0 = d_rr + rr * (7.0 * E + 2.0 * np.pi * d_ux + SINCOS_E * E) + E
            p = c + v0 * r
            nrm = -v0
            # the sphere itself: centre (one rounding per component) and radius (box corner difference,
            # the norm's 3 roundings halved by the square root, the growth factor's two) are fp32 on
            # the other side: 4 E relative on r, E |c| on the centre; then the fma's rounding.
            b_p = r * d_v0 + 4.0 * E * r + 2.0 * E * (np.abs(c).max() + r)
            b_n = d_v0
            w = rad * (4.0 * np.pi ** 2 * r * r) * count
            maxt = LARGEST
            offset = False
        else:
            em = sc.emitters[e]
            if em.is_mesh:
                pmf, cdf, prims, lo, hi, total, norm = mesh_arrays(sc, e)
                value = y * total
                k = np.minimum(lo + np.searchsorted(cdf[lo: hi + 1], value, side="left"), hi)
                # value rounds once; the entry is ambiguous when value is within that of a cdf entry
                near = np.minimum(np.abs(cdf[k] - value), np.abs(np.where(k > 0, cdf[np.maximum(k - 1, 0)], -1.0) - value))
                out["ambiguous"][sel] |= near <= total * E
                pmfn = pmf[k] * norm
                cdfn = np.where(k > 0, cdf[np.maximum(k - 1, 0)] * norm, 0.0)
                y2 = (y - cdfn) / pmfn
                # reuse: cdf * norm and pmf * norm round once each, the difference and the quotient once
                # each: (2 E + 2 E |y2| pmfn) / pmfn
                d_y2 = (2.0 * E + 2.0 * E * np.abs(y2) * pmfn) / pmfn + E
                t = np.sqrt(np.maximum(1.0 - x, 0.0))
                d_t1 = d_ux + E
                d_t = np.minimum(d_t1 / np.maximum(2.0 * t, 1e-300), np.sqrt(d_t1)) + E
                bx, by = 1.0 - t, t * y2
                d_bx, d_by = d_t + E, d_t * np.abs(y2) + t * d_y2 + E
                p0, p1, p2 = tri_points(sc, prims[k])
                e1, e2 = p1 - p0, p2 - p0
                p = p0 + e1 * bx[:, None] + e2 * by[:, None]
                a1, a2 = np.abs(e1).max(1), np.abs(e2).max(1)
                # the edges round once each; two fmas
                b_p = a1 * (d_bx + 2.0 * E) + a2 * (d_by + 2.0 * E) + 2.0 * E * np.abs(p).max(1)
                cr = np.cross(e1, e2)
                ln = np.linalg.norm(cr, axis=1)
                nrm = cr / ln[:, None]
                # cross: the edges' E each and two roundings per component, on the magnitude of the
                # terms, not of their difference: kappa = |e1| x |e2| / |cross|; normalize: the dot's
                # three roundings halved, sqrt, reciprocal, product
                kappa = (np.abs(e1)[:, [1, 2, 0]] * np.abs(e2)[:, [2, 0, 1]]
                         + np.abs(e1)[:, [2, 0, 1]] * np.abs(e2)[:, [1, 2, 0]]).max(1) / ln
                b_n = 2.0 * (4.0 * E * kappa) + 5.0 * E  # twice: the normalisation spreads one component's error
            else:
                c0, c1 = np.array(em.col0, np.float64), np.array(em.col1, np.float64)
                ctr = np.array(em.center, np.float64)
                lx, ly = 2.0 * x - 1.0, 2.0 * y - 1.0
                p = ctr + c0 * lx[:, None] + c1 * ly[:, None]
                nrm = np.tile(np.array(em.normal, np.float64), (len(sel), 1))
                # lx: 2 d_ux + E, ly: E; two fmas
                b_p = (np.abs(c0).max() * (2.0 * d_ux + E) + np.abs(c1).max() * E
                       + 2.0 * E * (np.abs(c0).max() + np.abs(c1).max() + np.abs(ctr).max())) + np.zeros(len(sel))
                b_n = np.zeros(len(sel))
            w = rad * np.pi / float(em.inv_area) * count
            maxt = LARGEST
            offset = True
        s, t_ = _frame(nrm)
        loc = local[sel]
        d = s * loc[:, [0]] + t_ * loc[:, [1]] + nrm * loc[:, [2]]
        # the frame: a = -1 / (sign + n.z) with |sign + n.z| >= 1, b and the six entries: at most four
        # roundings each on values <= 2, and its sensitivity to the normal is at most 4 per component
        # (|da/dn.z| <= 1, products of components <= 1); to_world: three fmas.
        b_frame = 8.0 * E + 4.0 * b_n
        b_d = 2.0 * (d_xy + b_frame) + d_z[sel] + b_n + b_frame + 3.0 * E
        if offset:
            mag = (1.0 + np.abs(p).max(1)) * RAY_EPS
            o = p + nrm * mag[:, None]  # dot(n, d) = local.z >= 0: the normal's side
            # side: dot(n, d) against 0. Its value is local.z up to the frame's error.
            out["side_ambiguous"][sel] = loc[:, 2] <= d_z[sel] + 3.0 * b_frame + 3.0 * E
            b_o = b_p + mag * (b_n + 4.0 * E) + 2.0 * E * np.abs(p).max(1)
        else:
            o, b_o = p, b_p
        out["o"][sel], out["d"][sel], out["p"][sel], out["n"][sel] = o, d, p, nrm
        out["weight"][sel] = w
        out["maxt"][sel] = maxt
        out["b_p"][sel], out["b_n"][sel], out["b_d"][sel], out["b_o"][sel] = b_p, b_n, b_d, b_o
    return out


# The weight: radiance * pi / inv_area * count is three roundings, the fp32
# constant pi a fourth (2.8e-8 < E): 4 E relative against the float64 value
# formed with the same inv_area. Against count * Le * pi * A_e with A_e from
# the vertices in float64, inv_area's own chain is added: a rectangle's is the
# float64 area rounded and inverted (2 E); a mesh's is the reciprocal (E) of
# the stored sum (E) of fp32 triangle areas, each the edges' roundings (2 E on
# a right-angled or well-shaped triangle), the cross product's two, the
# norm's (3 E halved + E) and an exact halving: 8 E. 4 + 8 = 12 E in all.
WEIGHT_REL = 4.0 * E
WEIGHT_AREA_REL = 12.0 * E


def unpack_emitter_ray(out):
    """The 17 planes of the probe / the kernel as the dict of emitter_ray_f64."""
    o = np.asarray(out)
    return {"o": o[0:3].T, "d": o[3:6].T, "maxt": o[6], "weight": o[7:10].T, "p": o[10:13].T, "n": o[13:16].T,
            "emitter": np.ascontiguousarray(o[16]).view(np.int32)}


def check_emitter_ray(got, ref):
    """Assert the fp32 result `got` (unpack_emitter_ray) against emitter_ray_f64's."""
    ok = ~ref["ambiguous"]
    assert ok.mean() > 0.99, "too many lanes within a bound of a discrete decision"
    assert np.array_equal(got["emitter"][ok], ref["emitter"][ok])
    g = {k: np.asarray(v, np.float64) for k, v in got.items()}
    for name, bound in (("p", "b_p"), ("n", "b_n"), ("d", "b_d")):
        err = np.abs(g[name][ok] - ref[name][ok]).max(1)
        assert np.all(err <= ref[bound][ok]), (name, float((err - ref[bound][ok]).max()))
    side = ok & ~ref["side_ambiguous"]
    err = np.abs(g["o"][side] - ref["o"][side]).max(1)
    assert np.all(err <= ref["b_o"][side]), ("o", float((err - ref["b_o"][side]).max()))
    assert np.array_equal(g["maxt"][ok], ref["maxt"][ok].astype(np.float32).astype(np.float64))
    rel = np.abs(g["weight"][ok] - ref["weight"][ok]) / ref["weight"][ok]
    assert np.all(rel <= WEIGHT_REL), ("weight", float(rel.max()))


# ----------------------------------------------- camera_sample_direction --
def camera64(sc):
    c = sc.camera
    return {"origin": np.array(c.origin, np.float64), "rows": np.array(c.inv_rows, np.float64).reshape(3, 3),
            "axes": np.array([list(c.axis_x), list(c.axis_y), list(c.axis_z)], np.float64),
            "tan": (float(c.tan_x), float(c.tan_y)), "clip": (float(c.near_clip), float(c.far_clip)),
            "size": (int(c.width), int(c.height))}


def camera_ray_f64(sc, pos01):
    """Origin and unit direction of the camera ray through the film-normalised
    positions pos01 (N, 2) (fov along x, +x of the camera to the image's left)."""
    c = camera64(sc)
    dl = np.stack([(1.0 - 2.0 * pos01[:, 0]) * c["tan"][0], (1.0 - 2.0 * pos01[:, 1]) * c["tan"][1],
                   np.ones(len(pos01))], 1)
    dl /= np.linalg.norm(dl, axis=1, keepdims=True)
    return c["origin"], dl @ c["axes"], dl[:, 2]


def sensor_direction_f64(sc, p):
    """The float64 value of camera_sample_direction for the (3, N) float32
    points p: dict of pos (N, 2), d (N, 3), dist, weight, valid, the bounds
    b_pos (pixels), b_d, rel_dist, rel_weight, and `ambiguous`."""
    c = camera64(sc)
    p = np.asarray(p, np.float32).astype(np.float64).T
    rel = p - c["origin"]
    R = c["rows"]
    l = rel @ R.T
    # rel: one rounding per component; each dot: three roundings on the magnitude of its terms
    mag = (np.abs(rel) @ np.abs(R).T)
    d_l = 4.0 * E * mag
    near, far = c["clip"]
    lz = l[:, 2]
    inside = (lz >= near) & (lz <= far)
    amb = (np.abs(lz - near) <= d_l[:, 2]) | (np.abs(lz - far) <= d_l[:, 2])
    W, H = c["size"]
    pos = np.zeros((len(p), 2))
    b_pos = np.zeros(len(p))
    valid = inside.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        for a, size in ((0, W), (1, H)):
            tan = c["tan"][a]
            q = l[:, a] / (lz * tan)
            # q: the numerator's d_l, the denominator's d_l tan + one rounding, the quotient's rounding
            d_q = (d_l[:, a] + np.abs(q) * tan * d_l[:, 2]) / np.abs(lz * tan) + 2.0 * E * np.abs(q)
            s = 0.5 * (1.0 - q)
            d_s = 0.5 * (d_q + E)
            amb |= inside & ((np.abs(s) <= d_s) | (np.abs(s - 1.0) <= d_s))
            valid &= (s >= 0.0) & (s <= 1.0)
            pos[:, a] = s * size
            b_pos = np.maximum(b_pos, size * (d_s + E * np.abs(s)))
    to = c["origin"] - p
    dist = np.linalg.norm(to, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = to / dist[:, None]
        ct = -(d @ R[2])
        weight = 1.0 / (4.0 * c["tan"][0] * c["tan"][1] * ct ** 3) / dist ** 2
    # d: the difference (E), the squared norm's three roundings and the difference's two halved by the
    # square root (2.5 E), sqrt, reciprocal, product: 6.5 E on a component <= 1, rounded up to 8 E.
    # dist: 2.5 E + E. cos: three roundings on terms <= |R2|_1 and d's error times |R2|_1. weight: five
    # products and two quotients (7 E), three times cos's relative error, twice dist's plus one.
    b_d = 8.0 * E
    rel_dist = 4.0 * E
    d_ct = (3.0 * E + b_d) * np.abs(R[2]).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_weight = 7.0 * E + 3.0 * d_ct / np.abs(ct) + 2.0 * rel_dist + E
    out = {"pos": np.where(valid[:, None], pos, 0.0), "d": np.where(valid[:, None], d, 0.0),
           "dist": np.where(valid, dist, 0.0), "weight": np.where(valid, weight, 0.0), "valid": valid,
           "b_pos": b_pos, "b_d": np.full(len(p), b_d), "rel_dist": rel_dist, "rel_weight": rel_weight,
           "ambiguous": amb}
    return out


def unpack_sensor_direction(out):
    o = np.asarray(out)
    return {"pos": o[0:2].T, "d": o[2:5].T, "dist": o[5], "weight": o[6],
            "valid": np.ascontiguousarray(o[7]).view(np.uint32) != 0}


def check_sensor_direction(got, ref):
    ok = ~ref["ambiguous"]
    assert np.array_equal(got["valid"][ok], ref["valid"][ok])
    v = ok & ref["valid"]
    g = {k: np.asarray(x, np.float64) for k, x in got.items()}
    err = np.abs(g["pos"][v] - ref["pos"][v]).max(1)
    assert np.all(err <= ref["b_pos"][v]), ("pos", float((err - ref["b_pos"][v]).max()))
    assert np.all(np.abs(g["d"][v] - ref["d"][v]).max(1) <= ref["b_d"][v])
    assert np.all(np.abs(g["dist"][v] / ref["dist"][v] - 1.0) <= ref["rel_dist"])
    rel = np.abs(g["weight"][v] / ref["weight"][v] - 1.0)
    assert np.all(rel <= ref["rel_weight"][v]), ("weight", float((rel / ref["rel_weight"][v]).max()))
    inv = ok & ~ref["valid"]
    for k in ("pos", "d"):
        assert not g[k][inv].any()
    assert not g["dist"][inv].any() and not g["weight"][inv].any()


def sensor_points(sc, n_grid=9, seed=5):
    """World points (3, N) float32 for the sensor tests: a film grid including
    the corners and edges times depths from the near to the far clip, plus
    points behind the camera, beyond the far clip and outside the frustum, and
    random points around the scene. Returns (points, grid positions (N, 2) in
    pixels or NaN, expected class: 1 inside, 0 outside, -1 either)."""
    c = camera64(sc)
    near, far = c["clip"]
    g = np.linspace(0.0, 1.0, n_grid)
    pos01 = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    depths = np.geomspace(near * 1.001, far * 0.999, 7)
    o, d, cz = camera_ray_f64(sc, np.repeat(pos01, len(depths), 0))
    z = np.tile(depths, len(pos01))
    pts = [o + d * (z / cz)[:, None]]
    grid = [np.repeat(pos01, len(depths), 0) * np.array(c["size"])]
    edge = (np.repeat(pos01, len(depths), 0) == 0).any(1) | (np.repeat(pos01, len(depths), 0) == 1).any(1)
    cls = [np.where(edge, -1, 1)]
    mid = np.array([[0.5, 0.5], [0.25, 0.75]])
    o, d, cz = camera_ray_f64(sc, mid)
    pts += [o - d * 2.0, o + d * (far * 1.5 / cz)[:, None], o + d * (near * 0.5 / cz)[:, None]]
    o, d, cz = camera_ray_f64(sc, np.array([[1.2, 0.5], [0.5, -0.3], [-0.1, 1.1]]))
    pts.append(o + d * 3.0)
    k = len(np.concatenate(pts[1:]))
    grid.append(np.full((k, 2), np.nan))
    cls.append(np.zeros(k, np.int64))
    rng = np.random.default_rng(seed)
    m = 2000
    pts.append(o + rng.uniform(-6.0, 6.0, (m, 3)))
    grid.append(np.full((m, 2), np.nan))
    cls.append(np.full(m, -1))
    return np.ascontiguousarray(np.concatenate(pts).T, np.float32), np.concatenate(grid), np.concatenate(cls)
