"""Animated mesh lights on the host: Scene.with_vertices(..., move_emitters=True) rebuilds the tables
(pmf | cdf) and the record words of every mesh emitter whose vertices moved,
by the loader's own code, so that the refit scene is a complete parity
reference for the device (test_moving_emitters_gpu.py). Rectangle emitters
stay refused. Fixtures: mesh_emitter_cases.py, moving_emitter_cases.py."""
import ctypes as C
import os

import mesh_emitter_cases as mc
import moving_emitter_cases as mv
import numpy as np
import pytest

from test_mesh_emitters import EPS, REFS, _draws, _geometry, _pick, _reference


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("moving_emitters"))
    mc.write_meshes(d)
    return d


def _record(scene, em):
    e = scene.emitters[em]
    return e.mesh, np.float32(e.inv_area), list(e.radiance)


# ------------------------------------------------------------- exact case --
def test_steps_scaled_is_exact(fx):
    """``steps`` scaled by 2 about a lattice point: every pmf entry is exactly
    four times the loader's (areas 2^0 .. 2^-5 and the zero one), the cdf, sum
    and norm are exact sums of powers of two, the valid range and every other
    word of the record stay, and ``patch`` (not moved) keeps its bits."""
    s = mc.build(fx, "full")
    em = mc.emitter_of(s, "steps")
    t = s.with_vertices(mv.steps_scaled(s), move_emitters=True)
    pmf0, cdf0, prim0 = mc.mesh_tables(s, em)
    pmf, cdf, prim = mc.mesh_tables(t, em)
    assert np.array_equal(pmf, np.float32(4.0) * pmf0) and np.array_equal(prim, prim0)
    assert sorted(pmf.tolist()) == [0.0, 2.0 ** -5, 2.0 ** -4, 2.0 ** -3, 2.0 ** -2, 2.0 ** -1, 1.0]
    assert np.array_equal(cdf.astype(np.float64), np.cumsum(pmf.astype(np.float64)))  # exact: no rounding anywhere
    assert np.array_equal(cdf, np.float32(4.0) * cdf0) and cdf[-1] == 63.0 / 32.0
    m0, _, rad0 = _record(s, em)
    m, inv_area, rad = _record(t, em)
    assert m["sum"] == 1.96875 and np.float32(m["norm"]) == np.float32(1.0) / np.float32(1.96875)
    assert np.float32(m["norm"]).view(np.uint32) == np.float32(32.0 / 63.0).view(np.uint32)
    assert inv_area == np.float32(m["norm"]) and rad == rad0
    for k in ("offset", "count", "kind", "valid_lo", "valid_hi"):
        assert m[k] == m0[k], k
    zero = np.flatnonzero(pmf0 == 0)
    assert len(zero) == 1 and pmf[zero[0]] == 0 and m["valid_lo"] <= zero[0] <= m["valid_hi"]
    pe = mc.emitter_of(s, "patch")
    for a, b in zip(mc.mesh_tables(s, pe), mc.mesh_tables(t, pe)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert bytes(s.emitters[pe]) == bytes(t.emitters[pe])


# ------------------------------------------------------ collapsing the ends --
def test_collapsed_ends_move_the_valid_range(fx, oracle):
    """The first and the last triangle with an area collapsed onto a line:
    valid_lo / valid_hi move inward, and sample_emitter_direction (the oracle's
    probe) never returns those entries -- u.y = 0 and u.y = 1 - 2^-24 included,
    where only the valid range keeps the search off them."""
    s = mc.build(fx, "full")
    em = mc.emitter_of(s, "steps")
    v, ends = mv.steps_ends_collapsed(s)
    t = s.with_vertices(v, move_emitters=True)
    m0, m = s.emitters[em].mesh, t.emitters[em].mesh
    pmf, cdf, prim = mc.mesh_tables(t, em)
    assert pmf[ends[0]] == 0 and pmf[ends[1]] == 0
    nz = np.flatnonzero(pmf > 0)
    assert (m["valid_lo"], m["valid_hi"]) == (nz[0], nz[-1])
    assert m["valid_lo"] > m0["valid_lo"] and m["valid_hi"] < m0["valid_hi"]
    assert np.float32(m["sum"]) == cdf[-1] == np.float32(pmf.astype(np.float64).sum())
    g = _geometry(t, em)
    N = len(t.emitters)
    u0 = (em + 0.37) / N
    u1 = np.concatenate([[0.0, 1.0 - 2.0 ** -24], (np.arange(2048) + 0.5) / 2048])
    ref = [0.1, -0.4, 0.2]
    out = oracle.probe(t, "sample_emitter", [ref + [u0, y] for y in u1])
    assert (out[:, 14] == em).all()
    chosen = np.full(len(u1), -1)
    p = out[:, 3:6].astype(np.float64)
    for k in range(len(prim)):
        if g["area"][k] == 0:
            continue
        r = p - g["p0"][k]
        bx, bz = r[:, 0] / g["e1"][k][0], r[:, 2] / g["e2"][k][2]  # legs along x and z
        inside = (bx >= -1e-5) & (bz >= -1e-5) & (bx + bz <= 1 + 1e-5)
        assert (chosen[inside] == -1).all()
        chosen[inside] = k
    assert (chosen >= 0).all()  # every sample lies in a triangle that has an area
    assert not np.isin(chosen, ends).any()
    assert chosen[0] == nz[0] and chosen[1] == nz[-1]
    assert np.isfinite(out[:, :14]).all()


# ------------------------------------------------- against a fresh load --
def _fresh_load(s, v, dirname):
    """The scene loaded from scratch from OBJ files that hold the moved
    vertices: each light's vertices in the scene's order and its faces in
    input order (leaf triangle j is input triangle tri_perm[j])."""
    from mtx.mitsuba_dict import scene_from_dict

    os.makedirs(dirname, exist_ok=True)
    faces = np.zeros((s.n_tris, 3), np.int64)
    faces[np.asarray(s.tri_perm)] = np.asarray(s.tri_vidx).reshape(-1, 3)
    inp_shape = np.zeros(s.n_tris, np.int64)
    inp_shape[np.asarray(s.tri_perm)] = np.asarray(s.tri_shape)
    for name in ("steps", "patch"):
        idx = mv.verts_of(s, name)
        assert np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx)))  # one shape, one vertex range
        with open(os.path.join(dirname, name + ".obj"), "w") as fh:
            for p in v[idx]:
                fh.write("v %r %r %r\n" % tuple(float(x) for x in p))
            for t in faces[inp_shape == mv.shape_index(name)] - idx[0] + 1:
                fh.write("f %d %d %d\n" % tuple(t))
    return scene_from_dict(mc.scene_dict("full"), base_dir=dirname)


@pytest.mark.parametrize("move", ["steps", "patch", "both"])
def test_refit_tables_equal_a_fresh_load(fx, tmp_path, move):
    """Independent of the refit path: the moved vertices written as OBJ files
    and loaded from scratch. Mapped through tri_perm, each input triangle's
    pmf is bit-identical; the sums agree within one fp32 ulp (another leaf
    order is another order of the double accumulation, and the one final
    rounding can differ by an ulp) -- on ``steps`` bit for bit, every sum there
    being exact."""
    s = mc.build(fx, "full")
    v = {"steps": mv.steps_scaled, "patch": mv.patch_sheared, "both": mv.lights_and_wall}[move](s)
    if move == "both":  # the fresh files hold the lights only; keep the wall
        w = mv.base_vertices(s)
        for name in ("steps", "patch"):
            w[mv.verts_of(s, name)] = v[mv.verts_of(s, name)]
        v = w
    t = s.with_vertices(v, move_emitters=True)
    f = _fresh_load(s, v, str(tmp_path / move))
    assert np.array_equal(f.vpos.view(np.uint32), t.vpos.view(np.uint32))
    first_tri = np.cumsum([0] + [int((np.asarray(s.tri_shape) == k).sum()) for k in range(len(s.shapes))])
    for name in ("steps", "patch"):
        em = mc.emitter_of(s, name)
        assert mc.emitter_of(f, name) == em
        per_input = []
        for sc in (t, f):
            pmf, _, prim = mc.mesh_tables(sc, em)
            inp = np.asarray(sc.tri_perm)[prim].astype(np.int64) - first_tri[mv.shape_index(name)]
            assert sorted(inp.tolist()) == list(range(len(prim)))
            per_input.append(pmf[np.argsort(inp)])
        assert np.array_equal(per_input[0].view(np.uint32), per_input[1].view(np.uint32))
        a, b = np.float32(t.emitters[em].mesh["sum"]), np.float32(f.emitters[em].mesh["sum"])
        if name == "steps":
            assert a == b
        else:
            assert abs(float(a) - float(b)) <= float(np.spacing(min(a, b)))
        for k in ("offset", "count", "kind"):
            assert t.emitters[em].mesh[k] == f.emitters[em].mesh[k]


# ------------------------------------------------------------ one density --
@pytest.mark.parametrize("variant", ["full", "env"])
def test_moved_patch_sampling_and_pdf_are_one_density(fx, oracle, variant):
    """test_mesh_emitters.py::test_sampling_and_pdf_are_one_density, its method
    and its tolerance, on the sheared and translated ``patch`` of the refit
    scene: the rebuilt tables (sampling) and the refit triangles (the hit
    side's pdf) describe one density."""
    s = mc.build(fx, variant)
    sc = s.with_vertices(mv.patch_sheared(s, variant), move_emitters=True)
    shape_em = np.array([x.emitter for x in sc.shapes])[np.asarray(sc.tri_shape)]
    V = np.asarray(sc.vpos, np.float64).reshape(-1, 3)[np.asarray(sc.tri_vidx).reshape(-1, 3)]
    em = mc.emitter_of(sc, "patch", variant)
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
    n_same = 0
    for i, w in enumerate(want):
        assert w["cos"] < -0.05
        np.testing.assert_array_equal(pe[i, 1:4], rad)
        if prim[i] != w["prim"]:
            continue
        n_same += 1
        extra = 16 * EPS * w["l"]
        scale = (w["dp"] + extra) / w["dp"]
        assert abs(float(pe[i, 0]) / float(out[i, 13]) - 1) <= 2 * scale * w["rpdf"]
    assert n_same >= 0.98 * len(want)


# ------------------------------------------------- identity and base scene --
def test_identity_and_base_scene_untouched(fx):
    s = mc.build(fx, "env")
    tables0, emitters0, vpos0 = np.array(s.tables), bytes(s.emitters), np.array(s.vpos)
    same = s.with_vertices(s.vpos, move_emitters=True)
    assert mv.tables_equal(same, s)
    t = s.with_vertices(mv.lights_and_wall(s, "env"), move_emitters=True)
    assert not mv.tables_equal(t, s)
    assert t.tables is not s.tables and t.emitters is not s.emitters
    assert np.array_equal(np.asarray(s.tables).view(np.uint32), tables0.view(np.uint32))
    assert bytes(s.emitters) == emitters0 and np.array_equal(s.vpos, vpos0)
    back = t.with_vertices(s.vpos, move_emitters=True)  # and back: the loader's bits again
    assert mv.tables_equal(back, s)
    assert np.array_equal(back.nodes, s.nodes) and np.array_equal(back.tri_geom, s.tri_geom)


# --------------------------------------------------- header against loader --
def _header_area(tris):
    from mtx._lib import check, lib

    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    out = np.zeros(len(tris), np.float32)
    check(lib().mtx_tri_area_f32(tris.ctypes.data, len(tris), out.ctypes.data), "mtx_tri_area_f32")
    return out


def test_header_area_equals_the_loader(fx):
    """mtx::tri_area (mtx_core/discrete.h, through mtx_tri_area_f32: the code
    the device's areas pass compiles) against scene._tri_area_f32 (the
    loader's numpy), bit for bit: the 198 ``patch`` triangles, before and after
    the shear; degenerate triangles; tiny ones, down to squared cross
    products that are denormal or underflow (the area itself, a square root,
    is never denormal); edges of 2^36 .. 2^64, whose squared
    cross product overflows (inf on both sides)."""
    from mtx.scene import _tri_area_f32

    s = mc.build(fx, "full")
    _, _, prim = mc.mesh_tables(s, mc.emitter_of(s, "patch"))
    assert len(prim) == 198
    vid = np.asarray(s.tri_vidx).reshape(-1, 3)[prim]
    cases = [np.asarray(v, np.float32).reshape(-1, 3)[vid].reshape(-1, 9) for v in (s.vpos, mv.patch_sheared(s))]
    rng = np.random.default_rng(3)
    p = rng.uniform(-1, 1, (64, 3, 3))
    deg = p.copy()
    deg[:, 2] = deg[:, 0] + 0.25 * (deg[:, 1] - deg[:, 0])  # collinear
    deg[:8, 1] = deg[:8, 0]  # a repeated vertex
    deg[8:16, 1] = deg[8:16, 2] = deg[8:16, 0]  # a point
    cases.append(deg.reshape(-1, 9))
    for e in (-20, -31, -34, -36, -37, -60, -70):  # cross ~ 2^(2e): its square from 2^-80 through the denormals to 0
        cases.append((p * 2.0 ** e).reshape(-1, 9))
    for e in (30, 36, 50, 63):
        cases.append((p * 2.0 ** e).reshape(-1, 9))
    tris = np.concatenate(cases).astype(np.float32)
    with np.errstate(all="ignore"):
        want = _tri_area_f32(tris[:, 0:3], tris[:, 3:6], tris[:, 6:9])
    got = _header_area(tris)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isinf(want).any() and (want == 0).any() and (want[: 2 * 198] > 0).all()
    small = want[(want > 0) & (want < 2.0 ** -60)]
    assert len(small) > 50  # the tiny class is alive, not all flushed to zero


# ---------------------------------------------------------------- refusals --
def test_refusals(fx):
    from mtx import MtxError

    s = mc.build(fx, "full")
    em = mc.emitter_of(s, "steps")
    with pytest.raises(MtxError, match=f"mesh emitter {em}"):
        s.with_vertices(mv.all_collapsed(s, "steps"), move_emitters=True)
    with pytest.raises(MtxError, match="no finite positive area"):
        s.with_vertices(mv.overflowing(s), move_emitters=True)
    with pytest.raises(MtxError, match="emitter"):
        s.with_vertices(mv.rectangle_moved(s), move_emitters=True)
    with pytest.raises(MtxError, match="rectangle"):
        s.with_vertices(mv.rectangle_moved(s), move_emitters=True)
    # without the keyword a moved mesh light is refused as it always was, and the message names the keyword
    with pytest.raises(MtxError, match="move_emitters=True"):
        s.with_vertices(mv.steps_scaled(s))
    assert mv.tables_equal(s.with_vertices(s.vpos), s)  # nothing moved: nothing to opt into


# -------------------------------------------------- order-sensitive input --
@pytest.mark.parametrize("n_slivers", [512, 1500])
def test_order_sensitive_emitter_on_the_host(tmp_path, n_slivers):
    """Areas 1, 2^-24 and slivers of 2^-60: in the scene's own entry order
    the sequential double prefix and a blocked one differ in an fp32 cdf entry
    and the exactness predicate is false (order_scene asserts both); the host
    tables are the sequential ones, before and after every vertex moved."""
    s = mv.order_scene(str(tmp_path), n_slivers)
    pmf, cdf, prim = mc.mesh_tables(s, 0)
    assert len(pmf) == n_slivers + 2
    assert sorted(set(pmf.tolist())) == [2.0 ** -60, 2.0 ** -24, 1.0]  # all exact in fp32
    assert mv.order_premise(pmf)
    seq = np.cumsum(pmf.astype(np.float64)).astype(np.float32)
    assert np.array_equal(cdf, seq) and not np.array_equal(seq, mv.blocked_cdf(pmf, 256))
    t = s.with_vertices(mv.order_moved(s), move_emitters=True)
    assert (t.vpos.reshape(-1, 3) != s.vpos.reshape(-1, 3)).any(1).all()
    pmf_t, cdf_t, _ = mc.mesh_tables(t, 0)
    assert np.array_equal(pmf_t, pmf) and np.array_equal(cdf_t, seq)
    assert bytes(t.emitters) == bytes(s.emitters)
    # a realistic light passes the predicate: the strips of the GPU tests
    assert mv.order_free(mc.mesh_tables(mv.strip_scene(str(tmp_path), 257), 0)[0])


def test_bound_scene_check_follows_the_tables(fx):
    """integrators._bind_scene takes a with_vertices scene through the device
    update only if its emitters and tables derive from the bound scene's: a
    copy that was given other tables is its own root (and is uploaded)."""
    import copy

    s = mc.build(fx, "full")
    t = s.with_vertices(mv.steps_scaled(s), move_emitters=True)
    u = t.with_vertices(mv.patch_sheared(s), move_emitters=True)
    for x in (s, t, u):
        r = x._emitter_root()
        assert r[0] is s.emitters and r[1] is s.tables
    c = copy.copy(t)
    c.tables = np.array(t.tables)
    r = c._emitter_root()
    assert r[0] is c.emitters and r[1] is c.tables
    assert C.sizeof(type(t.emitters)) == C.sizeof(type(s.emitters))
