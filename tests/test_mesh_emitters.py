"""Mesh area emitters (an ``area`` emitter on an ``obj`` or ``cube``) on the
CPU: the loaders, the record and its tables, and the shared sampling code of
mtx_core/interaction.h through the oracle's probes, against a float64
transcription of Mitsuba's Mesh::sample_position, Shape::sample_direction,
AreaEmitter::sample_direction and Scene::sample_emitter_direction
(DiscreteDistribution::sample_reuse, warp::square_to_uniform_triangle).
Mitsuba is not importable here: parity with it is unpinned, the arithmetic is.

The fixture (tests/mesh_emitter_cases.py) is a closed diffuse box with (a) six
triangles of areas 2^-2 .. 2^-7 plus a zero-area one, (b) a 198-triangle
jittered patch and (c) a rectangle emitter."""
import os
from fractions import Fraction

import mesh_emitter_cases as mc
import numpy as np
import pytest

EPS = 2.0 ** -24  # fp32 unit roundoff


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("mesh_emitters"))
    mc.write_meshes(d)
    return d


# ------------------------------------------------------------------ loaders --
def test_emitting_cube_and_obj_load(fx):
    """An area emitter on a cube or an obj loads (it raised MtxError before),
    as a mesh record: zero normal, inv_area = 1 / total area, face normals on
    the shape, the distribution in `tables`. Delta lights stay refused."""
    from mtx import MtxError
    from mtx.mitsuba_dict import scene_from_dict, spec_from_dict
    from test_mitsuba_dict import T, cornell_box

    d = cornell_box(16, 16)
    d["lamp"] = {"type": "cube", "to_world": T().translate([0, 0.5, 0]).scale(0.125),
                 "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [5, 4, 3]}}}
    sc = scene_from_dict(d)
    rect, lamp = sc.emitters[0], sc.emitters[1]
    assert not rect.is_mesh and lamp.is_mesh
    m = lamp.mesh
    assert m["count"] == 12 and m["kind"] == 1 and (m["valid_lo"], m["valid_hi"]) == (0, 11)
    assert lamp.inv_area == pytest.approx(1.0 / (6 * 0.25 ** 2), rel=1e-6)  # six faces of side 0.25
    assert list(lamp.radiance) == [5.0, 4.0, 3.0]
    assert sc.n_tables == 36 and len(sc.tables) == 36
    lamp_shape = [s for s in sc.shapes if s.emitter == 1]
    assert len(lamp_shape) == 1 and lamp_shape[0].flags & 1
    sc2 = mc.build(fx, "full")
    assert [e.is_mesh for e in sc2.emitters] == [True, True, False]
    for bad in ({"type": "point", "position": [0, 0, 0]}, {"type": "spot"}, {"type": "envmap", "filename": "x.exr"}):
        d2 = dict(d, extra=bad)
        with pytest.raises(MtxError):
            spec_from_dict(d2)
    d3 = dict(d)
    d3["lamp"] = dict(d["lamp"], emitter={"type": "spot"})
    with pytest.raises(MtxError, match="area"):
        spec_from_dict(d3)


def test_distribution_tables(fx):
    """pmf = fp32 triangle area, cdf = inclusive prefix accumulated in double
    and stored as float, sum / normalization / valid range as Mitsuba's
    DiscreteDistribution; every triangle of the shape listed once, in leaf
    order; the zero-area triangle has pmf 0. For (a) every entry is exact."""
    sc = mc.build(fx, "full")
    tri = np.asarray(sc.vpos, np.float64).reshape(-1, 3)[np.asarray(sc.tri_vidx).reshape(-1, 3)]
    area64 = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    shape_em = np.array([s.emitter for s in sc.shapes])[np.asarray(sc.tri_shape)]
    off = 0
    for name in ("steps", "patch"):
        em = mc.emitter_of(sc, name)
        e = sc.emitters[em]
        m = e.mesh
        pmf, cdf, prim = mc.mesh_tables(sc, em)
        assert m["offset"] == off
        off += 3 * m["count"]
        np.testing.assert_array_equal(prim, np.flatnonzero(shape_em == em))
        np.testing.assert_allclose(pmf, area64[prim], rtol=8 * EPS)
        np.testing.assert_array_equal(cdf, np.cumsum(pmf.astype(np.float64)).astype(np.float32))
        nz = np.flatnonzero(pmf > 0)
        assert (m["valid_lo"], m["valid_hi"]) == (nz[0], nz[-1])
        assert np.float32(m["sum"]) == cdf[-1] and np.float32(m["norm"]) == np.float32(1.0) / cdf[-1]
        assert np.float32(e.inv_area) == np.float32(1.0) / cdf[-1]
    assert off == sc.n_tables
    pmf, cdf, _ = mc.mesh_tables(sc, mc.emitter_of(sc, "steps"))
    assert sorted(pmf.tolist()) == [0.0] + [2.0 ** -k for k in range(7, 1, -1)]
    assert cdf[-1] == 63.0 / 128.0
    assert mc.build(fx, "full").emitters[mc.emitter_of(sc, "patch")].mesh["count"] == 198


def test_dictionary_and_xml_forms_agree(fx):
    from mtx.scene import Scene

    for v in ("full", "env"):
        a = mc.build(fx, v)
        path = os.path.join(fx, v + ".xml")
        with open(path, "w") as fh:
            fh.write(mc.scene_xml(v))
        b = Scene.from_xml(path)
        for k in ("vpos", "tri_vidx", "tri_shape", "tables", "nodes", "tri_geom", "occ_nodes"):
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
        for k in ("emitters", "shapes", "materials", "camera"):
            assert bytes(getattr(a, k)) == bytes(getattr(b, k)), k
        assert a.n_tables == b.n_tables and a.env_radiance == b.env_radiance


def test_rectangle_only_scenes_keep_their_bytes(small_scene):
    """The emitter records and tables of rectangle-only scenes are those of
    the commit before mesh emitters (tests/golden/rect_emitter_records.npz,
    written from that commit): the bedroom proxy at its test scale and the
    transcription of mi.cornell_box()."""
    from conftest import ROOT
    from mtx.mitsuba_dict import scene_from_dict
    from test_mitsuba_dict import cornell_box

    z = np.load(os.path.join(ROOT, "tests", "golden", "rect_emitter_records.npz"))
    for name, sc in (("bedroom", small_scene), ("cornell", scene_from_dict(cornell_box()))):
        assert bytes(sc.emitters) == z[name + "_emitters"].tobytes(), name
        assert np.asarray(sc.tables).tobytes() == z[name + "_tables"].tobytes(), name
        assert sc.n_tables == int(z[name + "_n_tables"])
        assert not any(e.is_mesh for e in sc.emitters)


def test_npz_round_trip_and_vertex_updates(fx, tmp_path):
    from mtx import MtxError
    from mtx.scene import Scene

    sc = mc.build(fx, "env")
    sc.save(str(tmp_path / "s.npz"))
    b = Scene.load(str(tmp_path / "s.npz"))
    assert bytes(b.emitters) == bytes(sc.emitters) and b.n_tables == sc.n_tables
    np.testing.assert_array_equal(b.tables, sc.tables)
    assert [e.is_mesh for e in b.emitters] == [True, True, False]
    assert b.emitters[1].mesh == sc.emitters[1].mesh
    # a vertex of a mesh light may not move: its tables would need a rebuild
    _, _, prim = mc.mesh_tables(sc, mc.emitter_of(sc, "patch"))
    v = np.array(sc.vpos, np.float32).reshape(-1, 3)
    v[np.asarray(sc.tri_vidx).reshape(-1, 3)[prim[5], 0], 1] += 0.01
    with pytest.raises(MtxError, match="tables rebuilt"):
        sc.with_vertices(v)
    box = np.asarray(sc.tri_vidx).reshape(-1, 3)[np.asarray(sc.tri_shape) == 0]
    v = np.array(sc.vpos, np.float32).reshape(-1, 3)
    v[box[0, 0]] *= 1.01  # a wall vertex may
    assert sc.with_vertices(v).emitters is sc.emitters


# ----------------------------------------------------------------- sampling --
def _geometry(sc, em):
    """float64 vertices, edges, areas and cdf of mesh emitter `em`."""
    _, _, prim = mc.mesh_tables(sc, em)
    tri = np.asarray(sc.vpos, np.float64).reshape(-1, 3)[np.asarray(sc.tri_vidx).reshape(-1, 3)[prim]]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cr = np.cross(e1, e2)
    area = 0.5 * np.linalg.norm(cr, axis=1)
    return {"prim": prim, "p0": tri[:, 0], "e1": e1, "e2": e2, "cross": cr, "area": area, "cdf": np.cumsum(area)}


def _pick(sc, u0):
    """Scene::sample_emitter_direction's uniform pick. It is a discrete
    decision, so it is taken in the code's own fp32: index and rescaled u.x."""
    N = len(sc.emitters) + (0 if sc.env_radiance is None else 1)
    scaled = np.float32(u0) * np.float32(N)
    idx = min(int(scaled), N - 1)
    return N, idx, float(scaled - np.float32(idx))


def _reference(sc, g, em, N, ref, u0r, u1):
    """float64 Mesh::sample_position + Shape::sample_direction +
    AreaEmitter::sample_direction + the pick probability, and the first-order
    fp32 error bounds of the header's operation sequence (module docstring of
    test_sample_values)."""
    S = g["cdf"][-1]
    nz = np.flatnonzero(g["area"] > 0)
    k = int(nz[0] + np.searchsorted(g["cdf"][nz[0]: nz[-1] + 1], u1 * S, side="left"))
    q = g["area"][k] / S
    y2 = (u1 - (g["cdf"][k - 1] / S if k else 0.0)) / q
    t = np.sqrt(max(0.0, 1.0 - u0r))
    b = (1.0 - t, t * y2)
    e1, e2, p0 = g["e1"][k], g["e2"][k], g["p0"][k]
    p = p0 + e1 * b[0] + e2 * b[1]
    n = g["cross"][k] / np.linalg.norm(g["cross"][k])
    dv = p - ref
    dist = np.linalg.norm(dv)
    d = dv / dist
    cos = d @ n
    pdf = (1.0 / S) * dist * dist / abs(cos) / N
    rad = np.array(list(sc.emitters[em].radiance), np.float64)
    w = rad / pdf if cos < 0 else np.zeros(3)
    # ---- bounds
    l1, l2 = np.linalg.norm(e1), np.linalg.norm(e2)
    dy = 8 * EPS / q
    dp = l1 * 4 * EPS + l2 * (dy + 4 * EPS) + 2 * EPS * 2.0
    kappa = l1 * l2 / np.linalg.norm(g["cross"][k])
    dn = (9 * kappa + 4) * EPS
    ddist = np.sqrt(3) * dp + 3 * EPS * dist
    dd = (1 + np.sqrt(3)) * dp / dist + 5 * EPS
    dcos = np.sqrt(3) * (dd + dn) + 3 * EPS
    rpdf = 12 * EPS + 2 * ddist / dist + dcos / abs(cos)
    return {"k": k, "prim": int(g["prim"][k]), "p": p, "n": n, "d": d, "dist": dist, "pdf": pdf, "w": w, "cos": cos,
            "y2": y2, "dp": dp, "dn": dn, "dd": dd, "ddist": ddist, "rpdf": rpdf, "l": l1 + l2,
            "margin": np.abs(g["cdf"] - u1 * S).min() / S}


def test_triangle_choice_is_exact(fx, oracle):
    """(a): u.y on the grid (k + 0.5) / 4096. The areas are 2^-2 .. 2^-7 (sum
    63 / 128), so u.y * sum and every cdf entry are exact in fp32 and no grid
    point lies on a cdf boundary ((2k + 1) 63 = 8192 c has no solution: the
    left side is odd): nothing is excluded. The chosen triangle -- read off
    the returned point, which lies in exactly one of the disjoint triangles --
    equals the float64 choice for every draw; each triangle's count is the
    exact number of grid points in its cdf interval (rational arithmetic;
    within one of share x 4096, the shares being k / 63); the zero-area
    triangle is never chosen."""
    sc = mc.build(fx, "full")
    em = mc.emitter_of(sc, "steps")
    g = _geometry(sc, em)
    N = len(sc.emitters)
    u0 = (em + 0.37) / N
    _, idx, u0r = _pick(sc, u0)
    assert idx == em
    ref = [0.1, -0.4, 0.2]
    u1 = (np.arange(4096) + 0.5) / 4096
    out = oracle.probe(sc, "sample_emitter", [ref + [u0, y] for y in u1])
    assert (out[:, 14] == em).all()
    # which triangle holds the returned point: barycentrics in its plane
    chosen = np.full(4096, -1)
    p = out[:, 3:6].astype(np.float64)
    for k in range(len(g["prim"])):
        if g["area"][k] == 0:
            continue
        r = p - g["p0"][k]
        bx, bz = r[:, 0] / g["e1"][k][0], r[:, 2] / g["e2"][k][2]  # legs along x and z
        inside = (bx >= -1e-5) & (bz >= -1e-5) & (bx + bz <= 1 + 1e-5)
        assert (chosen[inside] == -1).all()
        chosen[inside] = k
    want = np.array([_reference(sc, g, em, N, np.array(ref), u0r, y)["k"] for y in u1])
    np.testing.assert_array_equal(chosen, want)
    S = Fraction(63, 128)
    cdf = [Fraction(float(c)) for c in np.cumsum(g["area"])]
    for k in range(len(cdf)):
        lo, hi = (cdf[k - 1] if k else Fraction(0)) / S, cdf[k] / S
        exact = sum(1 for j in range(4096) if lo < Fraction(2 * j + 1, 8192) <= hi)
        assert int((chosen == k).sum()) == exact
        assert abs(exact - float(hi - lo) * 4096) < 1
    zero = int(np.flatnonzero(g["area"] == 0)[0])
    assert (chosen != zero).all() and (chosen >= 0).all()


REFS = [[0.0, 0.0, 0.0], [0.5, -0.5, 0.3], [-0.3, -1.0, -0.6], [0.8, 0.6, 1.0]]


def _draws(sc, em, n, seed):
    """n draws (u.x, u.y) whose uniform pick is emitter `em`."""
    N = len(sc.emitters) + (0 if sc.env_radiance is None else 1)
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2))
    u[:, 0] = (em + 0.02 + 0.96 * u[:, 0]) / N
    return u.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("variant,name", [("full", "steps"), ("full", "patch"), ("env", "patch"), ("mesh", "patch"),
                                          ("single", "steps")])
def test_sample_values(fx, oracle, variant, name):
    """ds.p, ds.n, ds.d, ds.dist, ds.pdf and the weight against the float64
    transcription. Bounds, first order in eps = 2^-24, from the header's
    operations (lengths l1 = |e1|, l2 = |e2|, q = pmf / sum the chosen
    triangle's probability, coordinates <= 2):
      y' = (u.y - cdf[k-1] norm) / (pmf norm): the two products carry 3 eps
        each (stored value, norm, product), the difference eps, so
        |dy'| <= 8 eps / q (the cancellation the reuse pays for);
      t = sqrt(1 - u.x): 1.5 eps t; b = (1 - t, t y'): 2.5 eps, dy' + 2.5 eps;
      p = fma(e1, b.x, fma(e2, b.y, p0)), e = fp32 vertex differences:
        dp <= 4 eps l1 + (dy' + 4 eps) l2 + 2 eps 2;
      n = normalize(cross(e1, e2)): each cross component 5 eps l1 l2, the
        normalisation 4 eps: dn <= (9 kappa + 4) eps, kappa = l1 l2 / |e1 x e2|;
      dist: sqrt(3) dp + 3 eps dist; d: (1 + sqrt 3) dp / dist + 5 eps;
      cos = dot(d, n): sqrt(3) (dd + dn) + 3 eps;
      pdf = inv_area dist^2 / |cos| / N: relative 12 eps + 2 ddist / dist +
        dcos / |cos| (inv_area: 7 eps from the fp32 areas and their sum, the
        reciprocal, two products, the division); weight = radiance / pdf: + 2 eps.
    The uniform pick and the triangle choice are discrete: the pick is taken
    in the code's fp32, and every draw must sit at least 16 eps (relative to
    the sum) from a cdf boundary: a draw that does not is moved by 2^-16 before the
    code under test sees it (decided on the float64 reference alone)."""
    sc = mc.build(fx, variant)
    em = mc.emitter_of(sc, name, variant)
    g = _geometry(sc, em)
    draws = _draws(sc, em, 256, 11)
    items, want = [], []
    for i, (u0, u1) in enumerate(draws):
        ref = REFS[i % len(REFS)]
        N, idx, u0r = _pick(sc, u0)
        assert idx == em
        w = _reference(sc, g, em, N, np.array(ref), u0r, u1)
        if w["margin"] <= 16 * EPS:  # an input too close to a boundary: moved, on the reference alone
            u1 = float(np.float32(u1 + 2.0 ** -16))
            w = _reference(sc, g, em, N, np.array(ref), u0r, u1)
        items.append(ref + [u0, u1])
        want.append(w)
    out = oracle.probe(sc, "sample_emitter", items).astype(np.float64)
    for o, w in zip(out, want):
        assert w["margin"] > 16 * EPS and w["cos"] < -0.05
        assert int(o[14]) == em
        assert np.abs(o[3:6] - w["p"]).max() <= w["dp"]
        assert np.abs(o[6:9] - w["n"]).max() <= w["dn"]
        assert np.abs(o[9:12] - w["d"]).max() <= w["dd"]
        assert abs(o[12] - w["dist"]) <= w["ddist"]
        assert abs(o[13] / w["pdf"] - 1) <= w["rpdf"]
        assert np.abs(o[0:3] / w["w"] - 1).max() <= w["rpdf"] + 2 * EPS
    if name == "steps" and variant == "full":
        assert len({w["k"] for w in want}) >= 4
    if name == "patch":
        assert len({w["k"] for w in want}) >= 100  # most of the 198 triangles


@pytest.mark.parametrize("variant", ["full", "env"])
def test_sampling_and_pdf_are_one_density(fx, oracle, variant):
    """For every sample of both mesh lights from four reference points inside
    the box: the ray ref -> ds.p (orc_trace) hits the sampled emitter (the
    float64 reference has every sample front-facing; nothing between the
    reference points and the lights: nothing is excluded), and where it hits
    the sampled triangle itself (edge samples may land on the coplanar
    neighbour) pdf_emitter_direction of that hit's direction sample equals
    ds.pdf, and emitter_eval is the radiance exactly. The hit is another
    evaluation of the same point: its barycentrics (Moeller-Trumbore, about a
    dozen fp32 operations on well-conditioned rays, incidence within 60
    degrees) are taken to carry at most 16 eps, which moves the point by
    16 eps (l1 + l2); both sides then carry test_sample_values' relative pdf
    bound, evaluated with that displacement added to dp."""
    sc = mc.build(fx, variant)
    shape_em = np.array([s.emitter for s in sc.shapes])[np.asarray(sc.tri_shape)]
    V = np.asarray(sc.vpos, np.float64).reshape(-1, 3)[np.asarray(sc.tri_vidx).reshape(-1, 3)]
    n_same = n_all = 0
    for name in ("steps", "patch"):
        em = mc.emitter_of(sc, name, variant)
        g = _geometry(sc, em)
        draws = _draws(sc, em, 256, 5)
        items, want = [], []
        for i, (u0, u1) in enumerate(draws):
            ref = REFS[i % len(REFS)]
            N, idx, u0r = _pick(sc, u0)
            w = _reference(sc, g, em, N, np.array(ref), u0r, u1)
            if w["margin"] <= 16 * EPS:  # as in test_sample_values
                u1 = float(np.float32(u1 + 2.0 ** -16))
                w = _reference(sc, g, em, N, np.array(ref), u0r, u1)
            items.append(ref + [u0, u1])
            want.append(w)
        out = oracle.probe(sc, "sample_emitter", items)
        rays = np.zeros((len(items), 8), np.float32)
        rays[:, 0:3] = np.array(items)[:, :3]
        rays[:, 3] = np.float32(3.0e38)
        rays[:, 4:7] = out[:, 9:12]
        hits, _ = oracle.trace(sc, rays, False)
        hits = hits.reshape(-1, 4)
        prim = hits[:, 1]
        buv = hits[:, 2:4].copy().view(np.float32).astype(np.float64)
        assert (prim != 0xFFFFFFFF).all() and (shape_em[prim] == em).all()
        tri = V[prim]
        ph = tri[:, 0] * (1 - buv[:, :1] - buv[:, 1:]) + tri[:, 1] * buv[:, :1] + tri[:, 2] * buv[:, 1:]
        cr = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        nh = cr / np.linalg.norm(cr, axis=1, keepdims=True)
        dv = ph - rays[:, 0:3]
        dist = np.linalg.norm(dv, axis=1)
        q = np.zeros((len(items), 11))
        q[:, 0], q[:, 1:4], q[:, 4], q[:, 5:8], q[:, 8:11] = em, dv / dist[:, None], dist, nh, [0.0, 0.0, 1.0]
        pe = oracle.probe(sc, "pdf_emitter", q)
        rad = np.array(list(sc.emitters[em].radiance), np.float32)
        for i, w in enumerate(want):
            assert w["cos"] < -0.05
            np.testing.assert_array_equal(pe[i, 1:4], rad)
            n_all += 1
            if prim[i] != w["prim"]:
                continue
            n_same += 1
            extra = 16 * EPS * w["l"]
            scale = (w["dp"] + extra) / w["dp"]
            assert abs(float(pe[i, 0]) / float(out[i, 13]) - 1) <= 2 * scale * w["rpdf"]
    assert n_same >= 0.98 * n_all


def test_nee_and_bsdf_sampling_agree_on_the_oracle(fx, oracle):
    """The mesh-light-only variant: path_test (NEE + MIS, which samples the
    mesh lights and weighs their pdf) and the BSDF-only `integrator` estimate
    the same image. K = 16 oracle renders x spp 64 each of the 32 x 16 film,
    4x4-pixel blocks (the criterion of test_gpu_convergence.py): every
    |z| < 5.5 and the image means within 1 %; NEE has the lower variance."""
    from mtx import develop, load_dict

    sc = mc.build(fx, "mesh", 32, 16)
    res = {}
    for j, name in enumerate(["path_test", "integrator"]):
        integ = load_dict({"type": name, "max_depth": 12})
        x = []
        for k in range(16):
            img = develop(oracle.render(sc, integ.render_args(sc, 1000 * j + k, 64))).astype(np.float64)
            H, W, _ = img.shape
            x.append(img.reshape(H // 4, 4, W // 4, 4, 3).mean(axis=(1, 3)))
        x = np.stack(x)
        res[name] = (x.mean(0), x.std(0, ddof=1) / np.sqrt(len(x)))
    (ma, sa), (mb, sb) = res["path_test"], res["integrator"]
    z = (ma - mb) / np.sqrt(sa ** 2 + sb ** 2 + 1e-30)
    assert np.abs(z).max() < 5.5, float(np.abs(z).max())
    assert abs(ma.mean() / mb.mean() - 1) < 1e-2, (ma.mean(), mb.mean())
    assert sa.mean() < sb.mean()
