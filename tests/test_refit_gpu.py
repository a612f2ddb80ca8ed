"""Vertex updates on the device (mtx_scene_update_vertices, refit.hip): the
device's arrays after an update equal the host refit (Scene.with_vertices) bit
for bit, traces and films equal the oracle on the refit scene, and refusals
are caught by the read-only pre-pass (no test provokes a fault)."""
import copy
import ctypes as C

import numpy as np
import pytest

from refit_cases import KINDS, deform, emitter_vertices
from test_mitsuba_dict import cornell_box
from test_scene import _random_rays

pytestmark = pytest.mark.gpu

ARRAYS = ("nodes", "occ_nodes", "tri", "occ_tri", "shade_rec", "vpos", "vnormal", "env_sphere")
_cache = {}


def _base(kind, small_scene):
    """small_scene (~37 k triangles, multi-level trees) or the converted
    Cornell box (a few dozen triangles: one or two levels, sparse slots)."""
    if kind == "small":
        return small_scene
    if "cornell" not in _cache:
        from mtx.mitsuba_dict import scene_from_dict

        _cache["cornell"] = scene_from_dict(cornell_box(64, 36))
    return _cache["cornell"]


def _refit(base_kind, kind, small_scene):
    """The host refit of one deformation (computed once, never modified)."""
    key = (base_kind, kind)
    if key not in _cache:
        s = _base(base_kind, small_scene)
        _cache[key] = s.with_vertices(deform(s, kind))
    return _cache[key]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def _pack9(geom):
    return np.ascontiguousarray(geom.reshape(-1, 12)[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]])


def _bound(scene):
    """A fresh context with `scene` uploaded in full."""
    from mtx import _lib
    from mtx.integrators import _bind_scene

    ctx = _lib.Context(0)
    _bind_scene(ctx, scene)
    return ctx


def _expect_host(ctx, t):
    """Every device array a host refit also produces equals it bit for bit."""
    for name, host in (("nodes", t.nodes), ("occ_nodes", t.occ_nodes), ("tri", _pack9(t.tri_geom)),
                       ("occ_tri", _pack9(t.occ_tri_geom)), ("vpos", t.vpos), ("vnormal", t.vnormal)):
        got = ctx.scene_read(name)
        assert np.array_equal(_u32(got), _u32(host)), name


@pytest.mark.parametrize("source", ["numpy", "torch"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("base_kind", ["small", "cornell"])
def test_device_state_equals_host_refit(base_kind, kind, source, small_scene):
    import torch

    s = _base(base_kind, small_scene)
    t = _refit(base_kind, kind, small_scene)
    ctx = _bound(s)
    fresh = _bound(t)  # mtx_scene_upload of the refit scene: shading records and sphere by the host loops
    try:
        v = t.vpos.reshape(-1, 3)
        ctx.update_vertices(torch.as_tensor(v, device="cuda") if source == "torch" else v)
        _expect_host(ctx, t)
        for name in ("shade_rec", "env_sphere"):
            assert np.array_equal(_u32(ctx.scene_read(name)), _u32(fresh.scene_read(name))), name
        assert np.array_equal(ctx.scene_read("env_sphere")[:3], t.env_sphere()[:3])
    finally:
        ctx.close()
        fresh.close()


def test_normals_follow_when_given(small_scene):
    """vnormal rewrites the normal rows of the records that use normals, and
    only those; without it they stay."""
    s = small_scene
    nrm = np.ascontiguousarray(s.vnormal.reshape(-1, 3)[:, [1, 2, 0]])
    t = s.with_vertices(deform(s, "sine"), vnormal=nrm)
    ctx, fresh = _bound(s), _bound(t)
    try:
        ctx.update_vertices(t.vpos, nrm)
        _expect_host(ctx, t)
        rec = ctx.scene_read("shade_rec")
        assert np.array_equal(_u32(rec), _u32(fresh.scene_read("shade_rec")))
        flags = rec.view(np.uint32).reshape(-1, 32)[:, 11]
        assert (flags & 1).any() and not (flags & 1).all()  # both kinds of record are exercised
    finally:
        ctx.close()
        fresh.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("base_kind", ["small", "cornell"])
def test_trace_after_update_equals_oracle(base_kind, kind, small_scene, oracle):
    """Closest hit and any hit through the process context: binding the refit
    scene after its base goes through the device refit, and hits and visit
    counts equal the oracle's on the refit scene (the same tree)."""
    from mtx import context, trace_rays

    s = _base(base_kind, small_scene)
    t = _refit(base_kind, kind, small_scene)
    rays, rng = _random_rays(6000, 11)
    trace_rays(s, rays[:1])  # binds (or re-binds) the base scene
    ctx = context()
    before = ctx.n_refits
    hits, vis = trace_rays(t, rays, visits=True)
    assert ctx.n_refits == before + 1
    c_hits, c_vis = oracle.trace(t, rays)
    assert np.array_equal(hits.reshape(-1), c_hits) and np.array_equal(vis, c_vis)
    rays[::2, 3] = rng.uniform(0.05, 2.0, 3000).astype(np.float32)
    occ, ovis = trace_rays(t, rays, any_hit=True, visits=True)
    assert ctx.n_refits == before + 1  # still bound
    c_occ, c_ovis = oracle.trace(t, rays, any_hit=True)
    assert np.array_equal(occ, c_occ) and np.array_equal(ovis, c_ovis)


@pytest.mark.parametrize("env", [False, True])
def test_film_fast_path_round_trip(env, small_scene, oracle, monkeypatch):
    """path_test at 64x36, spp 2: scene A, then A.with_vertices through the
    fast path (equal to the oracle and to a full upload, different from A),
    then back to A's vertices (A's nodes and film again). With a constant
    environment the bounding sphere matters."""
    from mtx import _lib, load_dict

    A = small_scene
    if env:
        A = copy.copy(small_scene)
        A.env_radiance = (0.4, 0.5, 0.6)
    B = A.with_vertices(deform(A, "sine" if not env else "scale50"))
    integ = load_dict({"type": "path_test"})
    ctx = _lib.Context(0)
    try:
        fA = integ.render_film(A, seed=1, spp=2, ctx=ctx)
        assert np.array_equal(fA, oracle.render(A, integ.render_args(A, 1, 2)))
        fB = integ.render_film(B, seed=1, spp=2, ctx=ctx)
        assert ctx.n_refits == 1
        assert np.array_equal(fB, oracle.render(B, integ.render_args(B, 1, 2)))
        assert not np.array_equal(fB, fA)
        monkeypatch.setenv("MTX_REFIT_UPLOAD", "1")
        full = _lib.Context(0)
        try:
            assert np.array_equal(integ.render_film(B, seed=1, spp=2, ctx=full), fB)
            integ.render_film(A, seed=1, spp=2, ctx=full)
            assert full.n_refits == 0  # forced full uploads
        finally:
            full.close()
        monkeypatch.delenv("MTX_REFIT_UPLOAD")
        A2 = B.with_vertices(A.vpos)
        fA2 = integ.render_film(A2, seed=1, spp=2, ctx=ctx)
        assert ctx.n_refits == 2
        assert np.array_equal(_u32(ctx.scene_read("nodes")), _u32(A.nodes))
        assert np.array_equal(_u32(ctx.scene_read("occ_nodes")), _u32(A.occ_nodes))
        assert np.array_equal(fA2, fA)
    finally:
        ctx.close()


def test_refusals_leave_the_device_scene_untouched(small_scene, oracle):
    """A moved emitter triangle, a NaN, a huge coordinate and a wrong count are
    MTX_E_ARG from the pre-pass; every device array is as before and the
    still-bound scene renders bit-exactly."""
    from mtx import _lib, load_dict

    s = small_scene
    integ = load_dict({"type": "path_test"})
    ctx = _lib.Context(0)
    L = _lib.lib()
    try:
        film = integ.render_film(s, seed=1, spp=2, ctx=ctx)
        state = {k: ctx.scene_read(k) for k in ARRAYS}
        v = s.vpos.reshape(-1, 3)
        movable = np.setdiff1d(np.arange(len(v)), emitter_vertices(s))
        cases = {}
        bad = v.copy()
        bad[emitter_vertices(s)[0], 1] += 0.01
        cases["emitter"] = bad
        bad = v.copy()
        bad[movable[5], 1] = np.nan
        cases["non-finite"] = bad
        bad = v.copy()
        bad[movable[7], 0] = 2.0 ** 37 * 1.001
        cases["magnitude bound"] = bad
        cases["vertices given"] = v[:-1].copy()
        for reason, arr in cases.items():
            rc = L.mtx_scene_update_vertices(ctx.handle, arr.ctypes.data, None, len(arr), 0)
            assert rc == -1 and reason.encode() in L.mtx_last_error(), (reason, L.mtx_last_error())
            for k in ARRAYS:
                assert np.array_equal(_u32(ctx.scene_read(k)), _u32(state[k])), (reason, k)
        rc = L.mtx_scene_update_vertices(ctx.handle, v.ctypes.data, None, len(v), 1)  # host memory as device memory
        assert rc == -1 and b"not device memory" in L.mtx_last_error()
        with pytest.raises(_lib.MtxError, match="emitter"):
            ctx_scene = ctx.scene
            ctx.update_vertices(cases["emitter"])
        # the wrapper forgot the binding; the C-level refusals above did not touch the device scene
        assert ctx_scene is s and ctx.n_refits == 0
        for k in ARRAYS:
            assert np.array_equal(_u32(ctx.scene_read(k)), _u32(state[k])), k
        a = integ.render_args(s, 1, 2)
        again = np.zeros_like(film)
        assert L.mtx_render(ctx.handle, C.byref(a), again.ctypes.data, 0, None) == 0  # no re-upload in between
        assert np.array_equal(again, film)
    finally:
        ctx.close()


def test_identity_update_on_the_device(small_scene):
    """Unchanged vertices give back the builder's nodes on the device too."""
    s = small_scene
    ctx = _bound(s)
    try:
        ctx.update_vertices(s.vpos)
        _expect_host(ctx, s)
    finally:
        ctx.close()
