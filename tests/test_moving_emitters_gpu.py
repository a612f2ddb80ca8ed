"""Animated mesh lights on the device: mtx_scene_update_vertices rebuilds the
tables and records of every mesh emitter (refit.hip: areas, the double prefix
-- block-parallel where its order provably cannot matter, in entry order
otherwise -- and the commit) bit for bit as Scene.with_vertices does on the
host and as a fresh upload of that scene gives; renders after an update equal
the oracle's; refusals come from the read-only pre-pass (no test provokes a
fault)."""
import ctypes as C
import os

import lattice_cases as lc
import mesh_emitter_cases as mc
import moving_emitter_cases as mv
import numpy as np
import pytest

from test_mesh_emitters_gpu import _rays
from test_refit_gpu import ARRAYS, _bound, _expect_host, _u32

pytestmark = pytest.mark.gpu

W, H = 32, 18
STATE = ARRAYS + ("tables", "emitters")


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("moving_emitters_gpu"))
    mc.write_meshes(d)
    return d


_moved = {}


def _host(fx, variant, move):
    """The host refit of one move (computed once, never modified)."""
    key = (fx, variant, move)
    if key not in _moved:
        s = mc.build(fx, variant, W, H)
        v = {"steps": mv.steps_scaled, "patch": mv.patch_sheared, "all": mv.lights_and_wall}[move](s, variant)
        _moved[key] = s.with_vertices(v, move_emitters=True)
    return _moved[key]


def _expect_tables(ctx, t):
    """The device's tables (every emitter's pmf | cdf | prim range, the
    roughplastic tables before them) and emitter records equal the host
    scene's bit for bit."""
    assert np.array_equal(_u32(ctx.scene_read("tables")), _u32(np.asarray(t.tables)[: t.n_tables])), "tables"
    assert ctx.scene_read("emitters").tobytes() == bytes(t.emitters), "emitters"


def _expect_state(ctx, other):
    for k in STATE:
        assert np.array_equal(_u32(ctx.scene_read(k)), _u32(other.scene_read(k))), k


def _update_and_compare(s, t, source="numpy"):
    """s uploaded, updated to t's vertices: equal to the host's t and to a
    fresh upload of t."""
    import torch

    ctx, fresh = _bound(s), _bound(t)
    try:
        v = t.vpos.reshape(-1, 3)
        ctx.update_vertices(torch.as_tensor(v, device="cuda") if source == "torch" else v)
        _expect_host(ctx, t)
        _expect_tables(ctx, t)
        _expect_state(ctx, fresh)
    finally:
        ctx.close()
        fresh.close()


# ------------------------------------------------------ device equals host --
@pytest.mark.parametrize("source", ["numpy", "torch"])
@pytest.mark.parametrize("move", ["steps", "patch", "all"])
def test_device_tables_equal_host(fx, move, source):
    s = mc.build(fx, "full", W, H)
    t = _host(fx, "full", move)
    assert not mv.tables_equal(s, t)
    _update_and_compare(s, t, source)


def test_update_and_back(fx):
    """An update followed by the update back to the original vertices: the
    state of the first upload, the identity update included."""
    s = mc.build(fx, "env", W, H)
    t = _host(fx, "env", "all")
    ctx, first = _bound(s), _bound(s)
    try:
        ctx.update_vertices(s.vpos)
        _expect_state(ctx, first)
        _expect_tables(ctx, s)
        ctx.update_vertices(t.vpos)
        _expect_tables(ctx, t)
        ctx.update_vertices(s.vpos)
        _expect_state(ctx, first)
        _expect_tables(ctx, s)
    finally:
        ctx.close()
        first.close()


# ------------------------------------------------------- the scan's edges --
# the areas and scan kernels work in blocks of 256 entries (255, 256, 257 and
# 511 .. 513 are their edges, 600 spans three blocks); 63 .. 65 are wave edges
STRIP_N = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 600, 1025)


@pytest.mark.parametrize("n", STRIP_N)
def test_strip_lights(tmp_path_factory, n):
    d = str(tmp_path_factory.getbasetemp() / "moving_strips")
    os.makedirs(d, exist_ok=True)
    s = mv.strip_scene(d, n)
    t = s.with_vertices(mv.strip_moved(s), move_emitters=True)
    pmf, cdf, _ = mc.mesh_tables(t, 0)
    assert len(pmf) == n and mv.order_free(pmf) and (pmf > 0).all()
    assert not np.array_equal(pmf, mc.mesh_tables(s, 0)[0])
    _update_and_compare(s, t)


# ------------------------------------------------------------ many emitters --
def test_lattice_sheets_move_and_scale(tmp_path_factory):
    """lattice_cases ``emit`` (18 mesh emitters of 128 triangles): every
    vertex moved by the lattice vector MOVE and the z stack scaled by 2. The
    tables are exact -- areas 1/8, or 1/2 on the z stack, cdf their multiples --
    and the closest-hit radiance of lattice_cases (L the hit sheet's radiance
    on its emitting side, valid = hit) holds on the updated device scene."""
    from mtx import context

    d = str(tmp_path_factory.mktemp("moving_lattice"))
    s = lc.build(d, "emit")
    v = mv.base_vertices(s)
    for k in range(12, 18):  # the z stack: scaled about the origin, in its plane and along z
        idx = mv.shape_vertices(s, k)
        v[idx] *= np.float32(2.0)
    v += np.array(lc.MOVE, np.float32)
    t = s.with_vertices(v, move_emitters=True)
    for em in range(18):
        pmf, cdf, _ = mc.mesh_tables(t, em)
        a = 0.5 if em >= 12 else 0.125
        assert len(pmf) == 128 and np.array_equal(pmf, np.full(128, a, np.float32))
        assert np.array_equal(cdf, (a * np.arange(1, 129)).astype(np.float32))
        m = t.emitters[em].mesh
        assert (m["valid_lo"], m["valid_hi"], m["sum"], m["norm"]) == (0, 127, 128 * a, 1.0 / (128 * a))
    _update_and_compare(s, t)
    rays = lc.rays_a(lc.MOVE)[::4]
    ref = lc.lattice_reference(t.tri_geom, rays)
    L, valid = lc.expected_radiance(t, t.tri_geom, rays, ref)
    lc.sample_closest(s, rays[:1])  # binds (or re-binds) the base scene
    ctx = context()
    before = ctx.n_refits
    got_L, got_valid = lc.sample_closest(t, rays)
    assert ctx.n_refits == before + 1  # through the device update, not an upload
    assert np.array_equal(got_valid, valid) and np.array_equal(got_L, L)
    assert (L > 0).any() and valid.any()


# -------------------------------------------------- order-sensitive emitter --
@pytest.mark.parametrize("n_slivers,with_patch", [(512, False), (1500, False), (512, True)])
def test_order_sensitive_emitter(tmp_path, n_slivers, with_patch):
    """The emitter of test_moving_emitters.py::test_order_sensitive_emitter_on_the_host
    fails the exactness predicate and a blocked summation gives another cdf
    (order_scene asserts both), so the device must take the ordered fallback;
    1500 slivers pass its 1024-entry staging chunk; beside ``patch`` the fast
    and the fallback emitter share one update."""
    s = mv.order_scene(str(tmp_path), n_slivers, with_patch)
    v = mv.order_moved(s)
    if with_patch:
        idx = mv.shape_vertices(s, 1)
        v[idx] = (v[idx].astype(np.float64) * [1.0, 1.1, 0.9] + [0.02, 0.0, 0.1]).astype(np.float32)
    t = s.with_vertices(v, move_emitters=True)
    pmf, cdf, _ = mc.mesh_tables(t, 0)
    assert mv.order_premise(pmf) and not np.array_equal(cdf, mv.blocked_cdf(pmf, 256))
    if with_patch:
        assert mv.order_free(mc.mesh_tables(t, 1)[0])
    _update_and_compare(s, t)


# ------------------------------------------------ renders after an update --
@pytest.mark.parametrize("variant", ["full", "env"])
@pytest.mark.parametrize("name", ["path_test", "mypath", "integrator", "nrc"])
def test_renders_after_a_device_update(fx, oracle, name, variant):
    """mtx_sample_rays and a 32 x 18 spp-2 film on a context that took the
    moved lights through the device update: bit-exact against the oracle on
    the host scene and against a fresh context that uploaded it."""
    from mtx import IndependentSampler, _lib, context, load_dict

    s = mc.build(fx, variant, W, H)
    t = _host(fx, variant, "all")
    integ = load_dict({"type": name})
    o, d = _rays(t, 2048, seed=3)
    lanes = np.arange(len(o), dtype=np.uint32) * 5 + 2
    integ.sample(s, IndependentSampler(7, lanes[:1], skip=2), (o[:1], d[:1]))  # binds (or re-binds) the base scene
    before = context().n_refits
    L, valid, _ = integ.sample(t, IndependentSampler(7, lanes, skip=2), (o, d))
    assert context().n_refits == before + 1
    Lc, vc = oracle.sample_rays(t, integ.render_args(t, 7, 1), np.concatenate([o, d], 1), lanes, 2)
    np.testing.assert_array_equal(valid, vc.astype(bool))
    np.testing.assert_array_equal(L, Lc)
    assert np.isfinite(L).all() and (L > 0).any()
    ctx, fresh = _lib.Context(0), _lib.Context(0)
    try:
        base = integ.render_film(s, seed=5, spp=2, ctx=ctx)
        film = integ.render_film(t, seed=5, spp=2, ctx=ctx)
        assert ctx.n_refits == 1
        np.testing.assert_array_equal(film, oracle.render(t, integ.render_args(t, 5, 2)))
        np.testing.assert_array_equal(film, integ.render_film(t, seed=5, spp=2, ctx=fresh))
        assert fresh.n_refits == 0 and not np.array_equal(film, base)
    finally:
        ctx.close()
        fresh.close()


# ---------------------------------------------------------------- refusals --
def test_refusals_leave_the_device_scene_untouched(fx):
    from mtx import _lib, load_dict

    s = mc.build(fx, "full", W, H)
    em = mc.emitter_of(s, "steps")
    integ = load_dict({"type": "path_test"})
    ctx = _lib.Context(0)
    L = _lib.lib()
    try:
        film = integ.render_film(s, seed=1, spp=2, ctx=ctx)
        state = {k: ctx.scene_read(k) for k in STATE}
        cases = {b"mesh emitter %d" % em: mv.all_collapsed(s, "steps"),
                 b"no finite positive area": mv.overflowing(s),
                 b"emitter": mv.rectangle_moved(s),
                 b"rectangle": mv.rectangle_moved(s)}
        for reason, arr in cases.items():
            rc = L.mtx_scene_update_vertices(ctx.handle, arr.ctypes.data, None, len(arr), 0)
            assert rc == -1 and reason in L.mtx_last_error(), (reason, L.mtx_last_error())
            for k in STATE:
                assert np.array_equal(_u32(ctx.scene_read(k)), _u32(state[k])), (reason, k)
        with pytest.raises(_lib.MtxError, match="mesh emitter"):
            ctx.update_vertices(mv.all_collapsed(s, "patch"))
        a = integ.render_args(s, 1, 2)
        again = np.zeros_like(film)
        assert L.mtx_render(ctx.handle, C.byref(a), again.ctypes.data, 0, None) == 0  # no re-upload in between
        assert np.array_equal(again, film)
    finally:
        ctx.close()
