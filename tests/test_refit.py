"""Vertex updates on the host: mtx_bvh_refit / mtx_bvh_refit_occlusion and
Scene.with_vertices (no GPU). The refit keeps topology, leaf order and slot
order and recomputes the quantised child boxes exactly as the builder does, so
unchanged vertices must give back the builder's nodes bit for bit."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from refit_cases import KINDS, deform, emitter_vertices
from test_scene import _check_bvh4, _check_occ, _random_rays, _tiny_mesh


def _refit_both(L, vpos, tri_vidx, nodes, occ_perm, occ_nodes):
    """(rc, nodes, tri_geom, rc_occ, occ_nodes, occ_tri_geom) of the two host refits on copies."""
    n = len(tri_vidx) // 3
    nodes, occ_nodes = nodes.copy(), occ_nodes.copy()
    geom, ogeom = np.full(12 * n, 7.0, np.float32), np.full(12 * n, 7.0, np.float32)
    vpos = np.ascontiguousarray(vpos, np.float32)
    rc = L.mtx_bvh_refit(vpos.ctypes.data, len(vpos.reshape(-1, 3)), tri_vidx.ctypes.data, n, nodes.ctypes.data,
                         len(nodes) // 16, geom.ctypes.data)
    assert rc == 0, L.mtx_last_error()
    rc = L.mtx_bvh_refit_occlusion(geom.ctypes.data, occ_perm.ctypes.data, n, occ_nodes.ctypes.data,
                                   len(occ_nodes) // 20, ogeom.ctypes.data)
    assert rc == 0, L.mtx_last_error()
    return nodes, geom, occ_nodes, ogeom


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_identity_small_scene(small_scene):
    from mtx import _lib

    s = small_scene
    nodes, geom, onodes, ogeom = _refit_both(_lib.lib(), s.vpos, s.tri_vidx, s.nodes,
                                             np.ascontiguousarray(s.occ_perm, np.uint32), s.occ_nodes)
    assert np.array_equal(nodes, s.nodes)
    assert np.array_equal(_bits(geom), _bits(s.tri_geom))
    assert np.array_equal(onodes, s.occ_nodes)
    assert np.array_equal(_bits(ogeom), _bits(s.occ_tri_geom))


@pytest.mark.parametrize("cnode", ["1", "4"])
@pytest.mark.parametrize("kind", ["one", "two", "nine", "identical", "planar", "random"])
def test_identity_tiny_meshes(kind, cnode, monkeypatch):
    """The builder's trees of the tiny and degenerate meshes of test_scene.py
    (two collapse node costs: other trees), refit with the vertices they were
    built from."""
    from mtx import _lib

    monkeypatch.setenv("MTX_BVH_CNODE", cnode)
    L = _lib.lib()
    v, idx = _tiny_mesh(kind)
    n = len(idx)
    idx = np.ascontiguousarray(idx)
    nodes = np.zeros((n + 1) * 16, np.int32)
    geom = np.zeros(12 * n, np.float32)
    perm = np.zeros(n, np.uint32)
    nn, dep = C.c_uint32(), C.c_uint32()
    assert L.mtx_bvh_build(v.ctypes.data, len(v), idx.ctypes.data, n, nodes.ctypes.data, C.byref(nn),
                           geom.ctypes.data, perm.ctypes.data, C.byref(dep)) == 0
    nodes = nodes[: 16 * nn.value].copy()
    onodes = np.zeros((n + 1) * 20, np.int32)
    ogeom = np.zeros(12 * n, np.float32)
    operm = np.zeros(n, np.uint32)
    assert L.mtx_bvh_build_occlusion(geom.ctypes.data, n, onodes.ctypes.data, C.byref(nn), ogeom.ctypes.data,
                                     operm.ctypes.data, C.byref(dep)) == 0
    onodes = onodes[: 20 * nn.value].copy()
    leaf_vidx = np.ascontiguousarray(idx[perm].reshape(-1))
    r_nodes, r_geom, r_onodes, r_ogeom = _refit_both(L, v, leaf_vidx, nodes, operm, onodes)
    assert np.array_equal(r_nodes, nodes)
    assert np.array_equal(_bits(r_geom), _bits(geom))
    assert np.array_equal(r_onodes, onodes)
    assert np.array_equal(_bits(r_ogeom), _bits(ogeom))


@pytest.fixture(scope="module")
def brute_base(small_scene, oracle):
    """Brute-force hit records of the undeformed scene (shared, never modified)."""
    rays, _ = _random_rays(6000, 11)
    b, _ = oracle.trace(small_scene, rays, brute=True)
    b.setflags(write=False)
    return b


@pytest.mark.parametrize("kind", KINDS)
def test_deformations(kind, small_scene, oracle, brute_base):
    s = small_scene
    v = deform(s, kind)
    t = s.with_vertices(v)
    assert t._geom_token is s._geom_token
    # shares topology and materials, owns the moved arrays
    assert t.tri_vidx is s.tri_vidx and t.tri_shape is s.tri_shape and t.materials is s.materials
    assert np.array_equal(_bits(t.vpos.reshape(-1, 3)), _bits(v)) and t.vpos is not s.vpos
    # same references, counts, slots: everything but origins, exponents and bounds
    n4, m4 = s.nodes.reshape(-1, 16), t.nodes.reshape(-1, 16)
    assert np.array_equal(n4[:, 4:8], m4[:, 4:8]) and np.array_equal(n4[:, 14:], m4[:, 14:])
    assert np.array_equal(n4[:, 3].view(np.uint32) >> 24, m4[:, 3].view(np.uint32) >> 24)
    n8, m8 = s.occ_nodes.reshape(-1, 20), t.occ_nodes.reshape(-1, 20)
    assert np.array_equal(n8[:, 4:8], m8[:, 4:8])
    assert np.array_equal(n8[:, 3].view(np.uint32) >> 24, m8[:, 3].view(np.uint32) >> 24)
    assert np.array_equal(_bits(t.occ_tri_geom.reshape(-1, 12)), _bits(t.tri_geom.reshape(-1, 12)[t.occ_perm]))
    # the records are the new vertices'
    p = v[t.tri_vidx.reshape(-1, 3)]
    g = t.tri_geom.reshape(-1, 12)
    assert np.array_equal(_bits(g[:, 0:3]), _bits(p[:, 0]))
    assert np.array_equal(_bits(g[:, 4:7]), _bits(p[:, 1] - p[:, 0]))
    assert np.array_equal(_bits(g[:, 8:11]), _bits(p[:, 2] - p[:, 0]))
    _check_bvh4(t.nodes, t.tri_geom, t.n_tris, t.bvh_depth)
    _check_occ(t.occ_nodes, t.occ_tri_geom, t.n_tris, t.occ_depth)
    rays, _ = _random_rays(6000, 11)
    h, _ = oracle.trace(t, rays)
    b, _ = oracle.trace(t, rays, brute=True)
    assert np.array_equal(h, b)
    changed = (b.reshape(-1, 4) != brute_base.reshape(-1, 4)).any(1).mean()
    print(f"{kind}: {changed:.3f} of the rays' hit records differ from the undeformed scene's")
    if kind == "sine":  # a refit that does nothing cannot pass
        assert changed >= 0.5
    else:
        assert changed > 0
    rays, rng = _random_rays(6000, 12)
    rays[::2, 3] = rng.uniform(0.05, 2.0, 3000).astype(np.float32)
    a, _ = oracle.trace(t, rays, any_hit=True)
    b, _ = oracle.trace(t, rays, brute=True)
    assert 0 < a.sum() < len(a)
    assert np.array_equal(a.astype(bool), b.reshape(-1, 4)[:, 1] != 0xFFFFFFFF)


def _digest(s):
    h = hashlib.sha256()
    for a in (s.vpos, s.vnormal, s.nodes, s.occ_nodes, s.tri_geom, s.occ_tri_geom, s.occ_perm, s.tri_vidx):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_refusals(small_scene):
    from mtx._lib import MtxError

    s = small_scene
    before = _digest(s)
    v = s.vpos.reshape(-1, 3).copy()
    with pytest.raises(MtxError, match="vertex count"):
        s.with_vertices(v[:-1])
    movable = np.setdiff1d(np.arange(len(v)), emitter_vertices(s))
    bad = v.copy()
    bad[movable[5], 1] = np.nan
    with pytest.raises(MtxError, match="non-finite"):
        s.with_vertices(bad)
    bad = v.copy()
    bad[movable[5], 2] = np.inf
    with pytest.raises(MtxError, match="non-finite"):
        s.with_vertices(bad)
    bad = v.copy()
    bad[movable[7], 0] = 2.0 ** 37 * 1.001  # just beyond the bound derived from the exponent range
    with pytest.raises(MtxError, match="magnitude bound"):
        s.with_vertices(bad)
    ok = v.copy()
    ok[movable[7], 0] = 2.0 ** 37  # the bound itself quantises
    t = s.with_vertices(ok)
    _check_bvh4(t.nodes, t.tri_geom, t.n_tris, t.bvh_depth)
    _check_occ(t.occ_nodes, t.occ_tri_geom, t.n_tris, t.occ_depth)
    bad = v.copy()
    bad[emitter_vertices(s)[0], 1] += 0.01
    with pytest.raises(MtxError, match="emitter"):
        s.with_vertices(bad)
    with pytest.raises(MtxError, match="normals"):
        s.with_vertices(v, vnormal=s.vnormal.reshape(-1, 3)[:-1])
    assert _digest(s) == before


def test_host_refit_refuses_malformed_input_and_writes_nothing(small_scene):
    """The C entry points check every reference before the first write."""
    from mtx import _lib

    L = _lib.lib()
    s = small_scene
    n = s.n_tris
    vidx = np.ascontiguousarray(s.tri_vidx)
    geom = np.full(12 * n, 7.0, np.float32)

    def refit(vpos, nodes, n_verts=None):
        return L.mtx_bvh_refit(vpos.ctypes.data, n_verts or len(vpos), vidx.ctypes.data, n, nodes.ctypes.data,
                               s.n_nodes, geom.ctypes.data)

    v = np.ascontiguousarray(s.vpos.reshape(-1, 3))
    nodes = s.nodes.copy()
    nodes.reshape(-1, 16)[3, 4] = s.n_nodes + 5  # a child that does not exist
    broken = nodes.copy()
    assert refit(v, nodes) == -1 and b"malformed" in L.mtx_last_error()
    assert np.array_equal(nodes, broken) and (geom == 7.0).all()
    nodes = s.nodes.copy()
    assert refit(v, nodes, n_verts=10) == -1 and b"out of range" in L.mtx_last_error()
    bad = v.copy()
    bad[0, 0] = np.nan
    assert refit(bad, nodes) == -1 and b"non-finite" in L.mtx_last_error()
    assert np.array_equal(nodes, s.nodes) and (geom == 7.0).all()
    onodes = s.occ_nodes.copy()
    ogeom = np.full(12 * n, 7.0, np.float32)
    perm = np.ascontiguousarray(s.occ_perm, np.uint32).copy()
    perm[9] = n
    assert L.mtx_bvh_refit_occlusion(s.tri_geom.ctypes.data, perm.ctypes.data, n, onodes.ctypes.data, s.n_occ_nodes,
                                     ogeom.ctypes.data) == -1
    assert b"out of range" in L.mtx_last_error()
    assert np.array_equal(onodes, s.occ_nodes) and (ogeom == 7.0).all()


def test_vnormal_kept_or_replaced(small_scene):
    s = small_scene
    v = deform(s, "translate")
    assert np.array_equal(_bits(s.with_vertices(v).vnormal), _bits(s.vnormal))
    nrm = np.ascontiguousarray(s.vnormal.reshape(-1, 3)[:, [1, 2, 0]])
    t = s.with_vertices(v, vnormal=nrm)
    assert np.array_equal(t.vnormal.reshape(-1, 3), nrm) and not np.array_equal(s.vnormal.reshape(-1, 3), nrm)


def test_environment_sphere_follows_the_vertices(small_scene):
    """The constant environment's bounding sphere is that of the new vertices'
    box (interaction.h env_bsphere): centre exact, the radius against an fp64
    evaluation (two fp32 ulps: the square, two fmas whose errors the root
    halves, the root and the product round once each, at most 0.5 ulp apiece)."""
    s = small_scene
    t = s.with_vertices(deform(s, "scale50"))
    v = t.vpos.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    sph = t.env_sphere()
    c32 = ((lo.astype(np.float32) + hi.astype(np.float32)) * np.float32(0.5))
    assert np.array_equal(sph[:3], c32)
    eps = 1500.0 * 2.0 ** -24
    r = np.linalg.norm(c32.astype(np.float64) - lo) * (1.0 + eps)
    assert abs(float(sph[3]) - r) <= 2 * np.spacing(np.float32(r))
    assert not np.array_equal(sph, s.env_sphere())  # the x50 shape grew the box
