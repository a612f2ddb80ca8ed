"""Mesh area emitters on the GPU: every kernel that samples an emitter (the
NEE of k_shade for path_test / mypath / nrc / the nerad RHS, the PSSMLT-path
emitter vertex, the ReSTIR GI secondary paths in the wavefront and in the path
megakernel) bit for bit against the oracle, on the fixture of
tests/mesh_emitter_cases.py and its variants. The 198-triangle patch is in
every scene, so the lanes of a wave search its cdf along different paths.
mtx_scene_upload's refusals of a damaged mesh record and of a bad tree are
here as a context's caller sees them; tests/test_scene_check.py pins the host
check itself, case by case, without a GPU."""
import copy
import ctypes as C
import os
import subprocess
import sys

import mesh_emitter_cases as mc
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 32, 18


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("mesh_emitters_gpu"))
    mc.write_meshes(d)
    return d


def _rays(scene, n, seed):
    """Camera rays through random film positions, then random rays inside the box."""
    rng = np.random.default_rng(seed)
    cam = scene.camera
    pos = rng.random((n, 2)).astype(np.float32)
    dl = np.stack([(1 - 2 * pos[:, 0]) * np.float32(cam.tan_x), (1 - 2 * pos[:, 1]) * np.float32(cam.tan_y),
                   np.ones(n, np.float32)], 1)
    dl /= np.linalg.norm(dl, axis=1, keepdims=True)
    M = np.stack([np.array(cam.axis_x), np.array(cam.axis_y), np.array(cam.axis_z)], 1).astype(np.float32)
    d = dl @ M.T
    o = np.tile(np.array(cam.origin, np.float32), (n, 1))
    h = n // 2
    o[h:] = rng.uniform(-1.6, 1.4, (n - h, 3)).astype(np.float32)
    v = rng.normal(size=(n - h, 3)).astype(np.float32)
    d[h:] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("variant", mc.VARIANTS)
@pytest.mark.parametrize("name", ["path_test", "mypath", "integrator", "nrc"])
def test_sample_rays_lanes(fx, oracle, name, variant):
    from mtx import IndependentSampler, load_dict

    sc = mc.build(fx, variant, W, H)
    integ = load_dict({"type": name})
    o, d = _rays(sc, 4096, seed=3)
    lanes = np.arange(len(o), dtype=np.uint32) * 5 + 2
    L, valid, _ = integ.sample(sc, IndependentSampler(7, lanes, skip=2), (o, d))
    Lc, vc = oracle.sample_rays(sc, integ.render_args(sc, 7, 1), np.concatenate([o, d], 1), lanes, 2)
    np.testing.assert_array_equal(valid, vc.astype(bool))
    np.testing.assert_array_equal(L, Lc)
    assert np.isfinite(L).all() and (L > 0).any()


@pytest.mark.parametrize("variant", mc.VARIANTS)
@pytest.mark.parametrize("name", ["path_test", "mypath"])
def test_films(fx, oracle, name, variant):
    from mtx import load_dict

    sc = mc.build(fx, variant, W, H)
    integ = load_dict({"type": name, "max_depth": 8})
    film = integ.render_film(sc, seed=5, spp=4)
    np.testing.assert_array_equal(film, oracle.render(sc, integ.render_args(sc, 5, 4)))
    assert film[..., :3].sum() > 0


@pytest.mark.parametrize("variant", mc.VARIANTS)
@pytest.mark.parametrize("name,iterations", [("pssmlt", 1), ("pssmlt", 8), ("pssmlt", 60), ("pssmlt_simple", 60)])
def test_pssmlt_films(fx, oracle, name, iterations, variant):
    """PSSMLT-path's mutated emitter sample feeds sample_emitter_direction:
    the film after 1, 8 and 60 Metropolis iterations; pssmlt_simple too.
    Pssmlt.render adds to the film only in iterations 41-49, so the films
    after 1 and 8 iterations are empty on both sides and it is the 60-iteration
    film (past the window and the large-step reset at 50) that carries the
    chains' radiance."""
    from mtx import load_dict

    sc = mc.build(fx, variant, W, H)
    integ = load_dict({"type": name, "iterations": iterations})
    film = integ.render_film(sc, seed=4, spp=2)
    np.testing.assert_array_equal(film, oracle.pssmlt_render(sc, integ.render_args(sc, 4, 2), iterations))
    if iterations > 41:
        assert film[..., :3].sum() > 0


RESTIR = {"jacobian": True, "bias_correction": True, "max_M_spatial": 500, "max_M_temporal": 30}


@pytest.mark.parametrize("variant", ["full", "mesh", "single"])  # ReSTIR GI refuses an environment
def test_restir_frames_and_reservoirs(fx, oracle, variant):
    from mtx import load_dict
    from test_restir import _oracle_frames

    sc = mc.build(fx, variant, W, H)
    refs, orc = _oracle_frames(oracle, sc, RESTIR, 3)
    integ = load_dict({"type": "restirgi", **RESTIR})
    for fr, ref in enumerate(refs):
        np.testing.assert_array_equal(integ.render_film(sc, seed=fr, spp=1), ref, err_msg=f"frame {fr}")
    np.testing.assert_array_equal(integ.state("sample"), orc.cur)
    np.testing.assert_array_equal(integ.state("temporal"), orc.tres)
    np.testing.assert_array_equal(integ.state("spatial"), orc.sres)
    np.testing.assert_array_equal(integ.state("radius"), orc.radius)
    assert ref[..., :3].sum() > 0


_RESTIR_CHILD = """
import sys
sys.path[:0] = [{pkg!r}, {orc!r}, {tests!r}]
import numpy as np
import binding as oracle
import mesh_emitter_cases as mc
from mtx import load_dict
from test_restir import _oracle_frames
oracle.build()
sc = mc.build({fx!r}, "full", 32, 18)
props = {props!r}
refs, orc = _oracle_frames(oracle, sc, props, 3)
integ = load_dict({{"type": "restirgi", **props}})
for fr, ref in enumerate(refs):
    assert np.array_equal(integ.render_film(sc, seed=fr, spp=1), ref), fr
assert np.array_equal(integ.state("temporal"), orc.tres)
assert np.array_equal(integ.state("spatial"), orc.sres)
print("CHILD OK")
"""


@pytest.mark.parametrize("mega_paths", ["4000000", "0"])
def test_restir_path_megakernel_forced(fx, oracle, mega_paths):
    """The secondary paths in the path megakernel (forced on for every band:
    MTX_MEGA_PATHS above the frame's paths) and in the wavefront kernels
    (megakernel off: 0). The switch is read at context creation, hence the
    child process."""
    from conftest import ROOT

    code = _RESTIR_CHILD.format(pkg=os.path.join(ROOT, "mitsuba3-experiments_amd"), orc=os.path.join(ROOT, "oracle"),
                                tests=os.path.join(ROOT, "tests"), fx=fx, props=RESTIR)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MTX_MEGA_PATHS=mega_paths),
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("variant", ["full", "env"])
def test_nerad_probes_and_render(fx, oracle, variant):
    """The nerad LHS points, the RHS lanes (whose NEE samples the mesh lights)
    and one "nerad" render, composed with the same field evaluation."""
    from mtx import load_dict
    from mtx.field import Field
    from mtx.nerad import IntersectionSampler, Integrator

    sc = mc.build(fx, variant, W, H)
    isamp = IntersectionSampler(sc)
    got = isamp.sample(3, 1000)
    assert np.array_equal(got.view(np.uint32), oracle.nerad_lhs(sc, isamp.tables, 3, 1000).view(np.uint32))
    field = Field(sc, seed=2, log2_table=12)
    batch, M = 600, 4
    L_rhs, lanes = Integrator(field, batch_size=batch, M=M).sample_rhs(sc, isamp, 5, 6, lanes=True)
    ref = oracle.nerad_rhs(sc, isamp.tables, 5, 6, batch, M)
    valid = ref[:, 9] > 0
    fv = np.zeros((len(ref), 3), np.float32)
    fv[valid] = field(ref[valid, 10:13], ref[valid, 13:16])
    L_ref, mean_ref = oracle.nerad_compose(ref, fv, M)
    np.testing.assert_array_equal(lanes, L_ref)
    np.testing.assert_array_equal(L_rhs, mean_ref)
    assert (ref[:, 0:3] > 0).any()  # the NEE term is alive
    integ = load_dict({"type": "nerad", "field": field})
    film = integ.render_film(sc, seed=2, spp=3)
    rl, pos = oracle.nerad_render_samples(sc, integ.render_args(sc, 2, 3))
    v2 = rl[:, 9] > 0
    f2 = np.zeros((len(rl), 3), np.float32)
    f2[v2] = field(rl[v2, 10:13], rl[v2, 13:16])
    L = f2 * rl[:, 3:6] + rl[:, 6:9]
    np.testing.assert_array_equal(film, oracle.film(sc.width, 0, sc.height, 3, np.ascontiguousarray(L, np.float32), pos))


def test_device_pointer_run(fx, oracle):
    """mtx_sample_rays_dev with torch tensors: equal to the host-pointer run
    and to the oracle."""
    import types

    import torch

    from mtx import IndependentSampler, load_dict

    sc = mc.build(fx, "env", W, H)
    integ = load_dict({"type": "path_test"})
    o, d = _rays(sc, 4096, seed=8)
    lanes = np.arange(len(o), dtype=np.uint32) * 3 + 1
    ray = types.SimpleNamespace(o=torch.as_tensor(o.T.copy(), device="cuda"), d=torch.as_tensor(d.T.copy(), device="cuda"))
    L, valid, _ = integ.sample(sc, IndependentSampler(9, lanes, skip=2), ray)
    assert L.is_cuda and valid.is_cuda
    Lh, vh, _ = integ.sample(sc, IndependentSampler(9, lanes, skip=2), (o, d))
    np.testing.assert_array_equal(L.cpu().numpy(), Lh)
    np.testing.assert_array_equal(valid.cpu().numpy(), vh)
    Lc, vc = oracle.sample_rays(sc, integ.render_args(sc, 9, 1), np.concatenate([o, d], 1), lanes, 2)
    np.testing.assert_array_equal(Lh, Lc)
    np.testing.assert_array_equal(vh, vc.astype(bool))


def test_rebinding_serves_the_new_emitters(fx, oracle):
    """A mesh-light scene bound after a rectangle-only scene of the same film
    size in the same context renders its own film, and the rectangle-only
    scene its own again afterwards."""
    from mtx import load_dict
    from mtx.mitsuba_dict import scene_from_dict
    from test_mitsuba_dict import cornell_box

    integ = load_dict({"type": "path_test", "max_depth": 6})
    rect = scene_from_dict(cornell_box(W, H))
    mesh = mc.build(fx, "mesh", W, H)
    f0 = integ.render_film(rect, seed=1, spp=2)
    f1 = integ.render_film(mesh, seed=1, spp=2)
    f2 = integ.render_film(rect, seed=1, spp=2)
    np.testing.assert_array_equal(f0, oracle.render(rect, integ.render_args(rect, 1, 2)))
    np.testing.assert_array_equal(f1, oracle.render(mesh, integ.render_args(mesh, 1, 2)))
    np.testing.assert_array_equal(f2, f0)


# -------------------------------------------------------- upload validation --
@pytest.mark.parametrize("corrupt,match", mc.MESH_RECORD_CORRUPTIONS)
def test_upload_refuses_inconsistent_mesh_records(fx, corrupt, match):
    """mtx_scene_upload checks a mesh record on the host before anything
    reaches the device: each inconsistency is MTX_E_ARG with a message, and
    the context still renders the intact scene afterwards."""
    from mtx import _abi, context, load_dict
    from mtx._lib import lib

    good = mc.build(fx, "full", W, H)
    sc = mc.with_corrupt_patch(good, corrupt)
    d = sc.desc()
    rc = lib().mtx_scene_upload(context(0).handle, C.byref(d))
    assert rc < 0 and _abi.ERRORS[rc] == "MTX_E_ARG"
    assert match in lib().mtx_last_error().decode()
    integ = load_dict({"type": "path_test", "max_depth": 4})
    assert integ.render_film(good, seed=0, spp=1)[..., 3].sum() > 0


def test_upload_refuses_a_bad_tree_and_keeps_the_scene(fx):
    """A structural refusal reaches mtx_scene_upload's caller with the words of
    the host check (tests/test_scene_check.py pins every such refusal on the
    CPU), no kernel sees the bad tree, and the scene bound before the refused
    call renders the same film after it."""
    from mtx import _abi, context, load_dict
    from mtx._lib import lib

    good = mc.build(fx, "full", 64, 36)
    integ = load_dict({"type": "path_test"})
    before = integ.render_film(good, seed=0, spp=1)
    sc = copy.copy(good)
    sc.nodes = np.array(good.nodes, np.int32)
    k = int(np.flatnonzero(sc.nodes.reshape(-1, 16)[0, 4:8] >= 0)[0])  # an inner child of the root
    sc.nodes[4 + k] = sc.n_nodes
    d = sc.desc()
    check = lib().mtx_diag_scene_check
    check.argtypes, check.restype = [C.POINTER(_abi.SceneDesc), C.POINTER(C.c_uint32)], C.c_int
    rc = check(C.byref(d), None)
    said = lib().mtx_last_error().decode()
    assert rc < 0 and _abi.ERRORS[rc] == "MTX_E_ARG" and "out of range" in said
    rc = lib().mtx_scene_upload(context(0).handle, C.byref(d))
    assert rc < 0 and _abi.ERRORS[rc] == "MTX_E_ARG"
    assert lib().mtx_last_error().decode() == said
    np.testing.assert_array_equal(integ.render_film(good, seed=0, spp=1), before)
    assert before[..., 3].sum() > 0
