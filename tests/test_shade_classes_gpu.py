"""The class queues of the shade kernel on the GPU (csrc/shade.hip
shade_loop<INT, CAM, CLS>): a block sorts its queue windows by shading class in LDS
and shades one class per step. What a path computes does not depend on the
lane or the step that shades it, so every film is compared bit for bit: the
class queues (MTX_SHADE_CLASSES=1, the default) against the mixed loop
(MTX_SHADE_CLASSES=0) and both against the CPU oracle, and the two forms'
ray counters and launch counts against each other.

Cases, the smallest that reach each branch of the loop:

* tiny: 50 paths, fewer than one block step: no ring ever fills, drain only;
* cornell: the all-diffuse Cornell box at 16 x 16 x 2 = 512 paths: whole
  windows of one class, two rings stay empty;
* metal: that box closed by a front wall, the camera inside, every surface
  a rough conductor: no path leaves, every hit is class 2, and whole windows
  of class 2 are shaded from its ring;
* small2 / small16: the small bedroom (all three classes) at 64 x 36, spp 2
  and 16: several blocks with one window each (the shade grid is 3 blocks
  per CU, so its stride is far above these queues), a window's three classes
  shaded as one packed step, windows past the queue's end;
* windows: the same film at spp 512 on one stream, 1,179,648 paths in one
  chunk: every block ingests several windows per bounce, rings fill across
  windows, wrap, and full one-class steps alternate with ingests -- the path
  the benchmark runs. Compared between the two forms (films and counters),
  not against the oracle;
* depth1 (nothing continues) beside the depth-8 renders;
* chunks: spp 16 in chunks of 4096 paths;
* mypath beside path_test (k_shade<path> beside k_shade<path-mis>).

The knob is read when the context is created, so each form is a fresh child
process; renders this small would otherwise run in the path megakernel, which
MTX_MEGA_PATHS=0 turns off. The oracle's films are computed once.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

# name -> (scene, integrator properties, film width, height, spp, chunk_paths)
CASES = {
    "tiny": ("small", {"type": "path_test", "max_depth": 8, "rr_depth": 2}, 10, 5, 1, 0),
    "cornell": ("cornell", {"type": "path_test", "max_depth": 8, "rr_depth": 2}, 16, 16, 2, 0),
    "cornell_mypath": ("cornell", {"type": "mypath", "max_depth": 8, "rr_depth": 2}, 16, 16, 2, 0),
    "metal": ("metal", {"type": "path_test", "max_depth": 8, "rr_depth": 2}, 32, 16, 2, 0),
    "small2": ("small", {"type": "path_test", "max_depth": 8, "rr_depth": 2}, 64, 36, 2, 0),
    "small16": ("small", {"type": "path_test", "max_depth": 8, "rr_depth": 2}, 64, 36, 16, 0),
    "depth1": ("small", {"type": "path_test", "max_depth": 1}, 64, 36, 2, 0),
    "chunks": ("small", {"type": "path_test", "max_depth": 8, "rr_depth": 2}, 64, 36, 16, 4096),
    "mypath": ("small", {"type": "mypath", "max_depth": 8, "rr_depth": 2}, 64, 36, 2, 0),
    "windows": ("small", {"type": "path_test", "max_depth": 8, "rr_depth": 2}, 64, 36, 512, 0),
}
NO_ORACLE = {"windows"}  # 1.2 M paths: the mixed loop is its reference
COUNTERS = ["rays_closest", "rays_shadow", "nodes_closest", "tris_closest", "nodes_shadow", "tris_shadow",
            "trace_launches", "shadow_launches"]


def build_scene(kind, width, height):
    from blocks_light_cases import _sensor, cornell_dict, rotate, translate
    from mtx import scene
    from mtx.mitsuba_dict import scene_from_dict

    if kind == "small":
        return scene.bedroom(width=64, height=36, scale=0.02, tex_res=64).with_film(width, height)
    d = cornell_dict(width, height)
    if kind == "metal":
        for name in ("white", "green", "red"):
            d[name] = {"type": "roughconductor", "alpha": 0.3}
        d["front"] = {"type": "rectangle", "to_world": translate([0.0, 0.0, 1.0]) @ rotate([0, 1, 0], 180),
                      "bsdf": {"type": "ref", "id": "white"}}
        d["sensor"] = _sensor([0.0, 0.0, 0.9], [0.0, -0.2, -1.0], 70.0, width, height)
    return scene_from_dict(d)


@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    from mtx import load_dict

    out = {}
    for name, (kind, props, w, h, spp, chunk) in CASES.items():
        if name in NO_ORACLE:
            continue
        twin = {"chunks": "small16"}.get(name)  # a film does not depend on its chunks
        if twin in out:
            out[name] = out[twin]
            continue
        sc = build_scene(kind, w, h)
        integ = load_dict(props)
        out[name] = oracle.render(sc, integ.render_args(sc, 11, spp))
    path = str(tmp_path_factory.mktemp("shade_classes") / "refs.npz")
    np.savez(path, **out)
    return path


_CHILD = r"""
import json, sys, numpy as np
sys.path[:0] = [{pkg!r}, {orc!r}, {tests!r}]
from mtx import load_dict
from test_shade_classes_gpu import CASES, COUNTERS, NO_ORACLE, build_scene
ref = np.load(sys.argv[1])
films, counters = {{}}, {{}}
for name, (kind, props, w, h, spp, chunk) in CASES.items():
    sc = build_scene(kind, w, h)
    integ = load_dict(props)
    film = integ.render_film(sc, seed=11, spp=spp, chunk_paths=chunk)
    if name not in NO_ORACLE:
        assert np.array_equal(film, ref[name]), ("film", name, int((film != ref[name]).sum()))
    film2, st = integ.render_film(sc, seed=11, spp=spp, chunk_paths=chunk, stats=True, counters=True)
    assert np.array_equal(film2, film), ("film with counters", name)
    films[name] = film
    counters[name] = {{k: int(st[k]) for k in COUNTERS}}
np.savez(sys.argv[2], **films)
print("COUNTERS " + json.dumps(counters))
print("CHILD OK")
"""


def _paths():
    return dict(pkg=os.path.join(ROOT, "mitsuba3-experiments_amd"), orc=os.path.join(ROOT, "oracle"),
                tests=os.path.join(ROOT, "tests"))


@pytest.mark.gpu
def test_class_queues_match_the_mixed_loop_and_the_oracle(refs, tmp_path):
    """The mixed loop first, then the class queues; a child that fails ends
    the test, so nothing more starts on the GPU after a failure."""
    code = _CHILD.format(**_paths())
    got = {}
    for knob in ("0", "1"):
        films = str(tmp_path / f"films{knob}.npz")
        env = dict(os.environ, MTX_MEGA_PATHS="0", MTX_STREAMS="1", MTX_SHADE_CLASSES=knob)
        r = subprocess.run([sys.executable, "-c", code, refs, films], env=env, capture_output=True, text=True,
                           timeout=120, cwd=ROOT)
        assert r.returncode == 0 and "CHILD OK" in r.stdout, (knob, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        line = [x for x in r.stdout.splitlines() if x.startswith("COUNTERS ")][-1]
        got[knob] = (np.load(films), json.loads(line[len("COUNTERS "):]))
    for name in CASES:
        assert np.array_equal(got["1"][0][name], got["0"][0][name]), name
        assert got["1"][1][name] == got["0"][1][name], (name, got["1"][1][name], got["0"][1][name])
        cnt = got["1"][1][name]
        assert cnt["rays_closest"] > 0 and cnt["trace_launches"] > 0, (name, cnt)
    assert got["1"][1]["small16"]["rays_shadow"] > 0
    # windows: the bounce-1 queue alone gives every block of a 3-blocks-per-CU grid several windows
    assert got["1"][1]["windows"]["rays_closest"] > 2 * 64 * 36 * 512
    assert np.isfinite(got["1"][0]["windows"]).all() and got["1"][0]["windows"][..., 3].sum() > 0
    # metal: a closed box, nothing escapes: every path is traced again until its depth or roulette ends it
    assert got["1"][1]["metal"]["rays_closest"] > 3 * 32 * 16 * 2
    # depth 1: one bounce, nothing continues
    assert got["1"][1]["depth1"]["rays_closest"] == 64 * 36 * 2


_GRID = r"""
import ctypes as C, sys
sys.path[:0] = [{pkg!r}]
from mtx import context
from mtx._lib import lib
fn = lib().mtx_diag_shade_grid
fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_uint32)], C.c_int
out = (C.c_uint32 * 2)()
assert fn(context(0).handle, out) == 0
print("GRID", out[0], out[1])
"""


@pytest.mark.gpu
def test_shade_grid_stays_three_blocks_per_cu():
    """The rings are 36 KB of a block's LDS: the occupancy query that sizes
    the persistent shade grid must still give 3 blocks per CU with them (and
    without), not its fallback."""
    for knob in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", _GRID.format(**_paths())], env=dict(os.environ, MTX_SHADE_CLASSES=knob),
                           capture_output=True, text=True, timeout=60, cwd=ROOT)
        assert r.returncode == 0, (knob, r.stdout[-500:], r.stderr[-1500:])
        grid, n_cu = (int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("GRID ")][-1].split()[1:])
        assert n_cu > 0 and grid == 3 * n_cu, (knob, grid, n_cu)


_BAD_KNOB = r"""
import sys
sys.path[:0] = [{pkg!r}]
from mtx import context
try:
    context(0)
except Exception as e:
    assert "MTX_SHADE_CLASSES" in str(e), str(e)
    print("REFUSED")
"""


@pytest.mark.gpu
def test_other_knob_values_are_refused():
    for bad in ("2", "yes"):
        r = subprocess.run([sys.executable, "-c", _BAD_KNOB.format(**_paths())],
                           env=dict(os.environ, MTX_SHADE_CLASSES=bad), capture_output=True, text=True, timeout=60,
                           cwd=ROOT)
        assert r.returncode == 0 and "REFUSED" in r.stdout, (bad, r.stdout[-500:], r.stderr[-1500:])


@pytest.mark.gpu
def test_record_flag_words_carry_the_class(small_scene):
    """What the kernel reads: bits 8..12 of word 11 of every uploaded shading
    record decode to the class of the triangle's material."""
    import ctypes as C

    from mtx import _abi, load_dict
    from mtx._lib import context, lib

    sc = small_scene
    load_dict({"type": "path_test", "max_depth": 1}).render_film(sc, seed=0, spp=1)  # binds the scene
    rec = context().scene_read("shade_rec").view(np.uint32).reshape(-1, 32)
    bits = (rec[:, 11] >> 8) & 0x1F
    assert (bits > 0).all()
    fn = lib().mtx_diag_shade_classes
    fn.argtypes, fn.restype = [C.POINTER(_abi.SceneDesc), C.c_void_p], C.c_int
    want = np.zeros(len(rec), np.uint8)
    d = sc.desc()
    assert fn(C.byref(d), want.ctypes.data) == 0
    t = (bits - 1) >> 2
    got = np.where(t == _abi.MTX_MAT_DIFFUSE, 0, np.where(t == _abi.MTX_MAT_ROUGHPLASTIC, 1, 2))
    assert np.array_equal(got, want)
