"""The prepared-ray ring of the closest-hit traversal (k_trace_closest,
csrc/device_common.h RayRing): results are per-ray quantities, the ring only
changes which lane runs a ray and when.

A lost ray, a ray run twice or a wrong ring slot shows up as a film or a
counter that differs from the CPU oracle, so every check is bit for bit:

* queues of 1, R-1, R, R+1 (R = 16 and 32), 63, 64, 65, 127, 128, 129 and
  4096 rays: a partial last fill, an empty ring with lanes still running, a
  reservoir drained in the middle of a fill, a queue shorter than a claim.
  Stored rays (integ.sample through mtx_sample_rays) put exactly that many
  into k_trace_closest's bounce-0 queue; path_test films of width x height
  x spp = that many paths start from the camera kernel (which keeps its
  whole-wave refill) and hand k_trace_closest the shorter queues of the
  later bounces;
* one ReSTIR GI frame with MTX_MEGA_PATHS=0, so that its stage A runs the
  wavefront kernels (k_trace_closest on stored rays) and its visibility tests
  k_trace_test, an any-hit loop (threshold refill);
* the counters of the STATS twins: the camera kernel's rays, nodes and
  triangles equal the oracle's traversal of the same camera rays (max_depth
  1), and the closest-hit and shadow counters of a depth-5 render -- for
  which the oracle has no ray list -- equal, under every knob variant, those
  of MTX_TRACE_RING=0 (k_trace_closest_refill, the threshold refill), whose
  film is checked against the oracle like every other.

The knobs are read when the context is created, so each variant is a fresh
child process with its own time limit; the children run one after the other
and the first failure, in a child or between two of them, ends the test. The
oracle's references are computed once and handed to the children in a file.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

# bounce-0 queue length -> (width, height, spp)
QUEUES = {1: (1, 1, 1), 15: (5, 3, 1), 16: (4, 4, 1), 17: (17, 1, 1), 31: (31, 1, 1), 32: (8, 4, 1), 33: (11, 3, 1),
          63: (9, 7, 1), 64: (8, 8, 1), 65: (13, 5, 1), 127: (127, 1, 1), 128: (16, 8, 1), 129: (43, 3, 1),
          4096: (64, 32, 2)}

VARIANTS = {  # in this order; ring0 gives the reference counters
    "ring0": {"MTX_TRACE_RING": "0"},
    "default": {},
    "ring16": {"MTX_TRACE_RING": "16"},
    "ring32": {"MTX_TRACE_RING": "32"},
    "spill-all": {"MTX_LDS_STACK": "1"},
    "notop": {"MTX_LDS_TOP": "0", "MTX_OCC_LDS_TOP": "0"},
    "noxcd": {"MTX_XCD_CLAIM": "0"},
}


def _small():
    from mtx import scene

    return scene.bedroom(width=64, height=36, scale=0.02, tex_res=64)


def _sample_case(sc):
    from mtx import IndependentSampler
    from test_gpu_parity import _camera_rays

    o, d = _camera_rays(sc, max(QUEUES), seed=3)
    lanes = np.arange(len(o), dtype=np.uint32) * 5 + 1
    return o, d, lanes, lambda n: IndependentSampler(4, lanes[:n], skip=2)


@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    """The oracle's side of every check, in one .npz for the children."""
    from mtx import load_dict
    from test_restir import CONFIGS, _oracle_frames

    sc = _small()
    integ = load_dict({"type": "path_test", "max_depth": 5})
    out = {}
    for n, (w, h, spp) in QUEUES.items():
        assert w * h * spp == n
        f = sc.with_film(w, h)
        out[f"film{n}"] = oracle.render(f, integ.render_args(f, 7, spp))
    o, d, lanes, _ = _sample_case(sc)
    L, v = oracle.sample_rays(sc, integ.render_args(sc, 4, 1), np.concatenate([o, d], 1), lanes, 2)
    out["sample_L"], out["sample_valid"] = L, v.astype(bool)
    rs = sc.with_film(40, 24)
    out["restir"] = _oracle_frames(oracle, rs, CONFIGS["unbiased"], 1)[0][0]
    # the camera rays of a max_depth-1 render, traversed by the oracle
    cam = load_dict({"type": "path_test", "max_depth": 1})
    a = cam.render_args(sc, 9, 3)
    _, pos = oracle.render_samples(sc, a)
    adj = (pos / np.array([sc.width, sc.height], np.float32)).astype(np.float32)
    cr = oracle.probe(sc, "camera_ray", adj)
    rays = np.zeros((len(pos), 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = cr[:, 0:3], cr[:, 6], cr[:, 3:6]
    _, visits = oracle.trace(sc, rays, False)
    out["cam_counts"] = np.array([len(pos), visits[:, 0].astype(np.uint64).sum(), visits[:, 1].astype(np.uint64).sum()],
                                 np.uint64)
    out["cam_film"] = oracle.render(sc, a)
    out["film_depth5"] = oracle.render(sc, integ.render_args(sc, 2, 3))
    path = str(tmp_path_factory.mktemp("trace_ring") / "refs.npz")
    np.savez(path, **out)
    return path


_CHILD = r"""
import json, sys, numpy as np
sys.path[:0] = [{pkg!r}, {orc!r}, {tests!r}]
from mtx import load_dict
from test_restir import CONFIGS
from test_trace_ring_gpu import QUEUES, _sample_case, _small
ref = np.load(sys.argv[1])
sc = _small()
integ = load_dict({{"type": "path_test", "max_depth": 5}})
for n, (w, h, spp) in QUEUES.items():
    f = sc.with_film(w, h)
    assert np.array_equal(integ.render_film(f, seed=7, spp=spp), ref[f"film{{n}}"]), ("film", n)
o, d, lanes, sampler = _sample_case(sc)
for n in QUEUES:  # the ring kernel's bounce-0 queue holds exactly n stored rays
    L, valid, _ = integ.sample(sc, sampler(n), (o[:n], d[:n]))
    assert np.array_equal(valid, ref["sample_valid"][:n]) and np.array_equal(L, ref["sample_L"][:n]), ("sample_rays", n)
rs = load_dict({{"type": "restirgi", **CONFIGS["unbiased"]}})
assert np.array_equal(rs.render_film(sc.with_film(40, 24), seed=0, spp=1), ref["restir"]), "restir"
cam = load_dict({{"type": "path_test", "max_depth": 1}})
film, st = cam.render_film(sc, seed=9, spp=3, stats=True, counters=True)
assert np.array_equal(film, ref["cam_film"]), "camera film"
got = [st["rays_closest"], st["nodes_closest"], st["tris_closest"]]
assert got == [int(x) for x in ref["cam_counts"]], ("camera counters", got)
film, st = integ.render_film(sc, seed=2, spp=3, stats=True, counters=True)
assert np.array_equal(film, ref["film_depth5"]), "depth-5 film with counters"
keys = ["rays_closest", "nodes_closest", "tris_closest", "rays_shadow", "nodes_shadow", "tris_shadow"]
print("COUNTERS " + json.dumps({{k: int(st[k]) for k in keys}}))
print("CHILD OK")
"""

def _paths():
    return dict(pkg=os.path.join(ROOT, "mitsuba3-experiments_amd"), orc=os.path.join(ROOT, "oracle"),
                tests=os.path.join(ROOT, "tests"))


@pytest.mark.gpu
def test_ring_variants_bit_exact(refs):
    """One child per variant, one after the other, the threshold refill
    (ring0) first: its counters are what every other variant must equal. The
    first child that fails ends the test, so nothing more starts on the GPU
    after a failure."""
    code = _CHILD.format(**_paths())
    want = None
    for variant, knobs in VARIANTS.items():
        env = dict(os.environ, MTX_MEGA_PATHS="0", **knobs)
        r = subprocess.run([sys.executable, "-c", code, refs], env=env, capture_output=True, text=True, timeout=120,
                           cwd=ROOT)
        assert r.returncode == 0 and "CHILD OK" in r.stdout, (variant, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        line = [x for x in r.stdout.splitlines() if x.startswith("COUNTERS ")][-1]
        cnt = json.loads(line[len("COUNTERS "):])
        assert cnt["rays_closest"] > 3 * 64 * 36 and cnt["rays_shadow"] > 0, (variant, cnt)
        if want is None:
            want = cnt  # ring0
        # per-ray quantities: the same whichever lane ran a ray
        assert cnt == want, (variant, cnt, want)


_BAD_KNOB = r"""
import sys
sys.path[:0] = [{pkg!r}]
from mtx import context
try:
    context(0)
except Exception as e:
    assert "MTX_TRACE_RING" in str(e), str(e)
    print("REFUSED")
"""


@pytest.mark.gpu
def test_other_ring_sizes_are_refused():
    """A ring of 8 rays would get slots the split never sized: context
    creation refuses every value but 0, 16 and 32 instead of rounding it."""
    for bad in ("8", "24", "32x"):
        r = subprocess.run([sys.executable, "-c", _BAD_KNOB.format(**_paths())], env=dict(os.environ, MTX_TRACE_RING=bad),
                           capture_output=True, text=True, timeout=60, cwd=ROOT)
        assert r.returncode == 0 and "REFUSED" in r.stdout, (bad, r.stdout[-500:], r.stderr[-1500:])


def _lds(ring, lds_stack, lds_top):
    """(LDS bytes, stack entries in LDS) of a k_trace_closest block."""
    import ctypes as C

    from mtx._lib import lib

    fn = lib().mtx_diag_trace_lds
    fn.argtypes = [C.c_uint32] * 3 + [C.POINTER(C.c_uint32)]
    fn.restype = C.c_int
    out = (C.c_uint32 * 2)()
    assert fn(ring, lds_stack, lds_top, out) == 0
    return out[0], out[1]


def test_trace_block_lds_fits_eight_blocks_per_cu():
    """A closest-hit block with rings takes at most 20 KB of LDS (8 blocks in
    a CU's 160 KB) whatever MTX_LDS_STACK and MTX_LDS_TOP ask for (clamps:
    context.cpp read_knobs), keeps at least one stack entry there, and gives
    up tree-top nodes only where that entry would not fit; without rings the
    defaults take the 20 KB."""
    for ring in (16, 32):
        rings = ring * 14 * 4 * 4  # 14 words an entry, 4 waves a block
        for stack in (1, 2, 8, 9, 16, 65):
            for top in (0, 1, 56, 64, 200, 256):
                size, entries = _lds(ring, stack, top)
                assert size <= 20 * 1024, (ring, stack, top, size)
                assert 1 <= entries <= stack
                nodes = (size - rings - entries * 1024) // 64
                assert size == rings + entries * 1024 + nodes * 64 and nodes <= top
                if nodes < top:  # the top gave way: nothing else could
                    assert entries == 1 and size + 64 > 20 * 1024
                elif entries < stack:  # the stack gave way: one more entry would not fit
                    assert size + 1024 > 20 * 1024
    assert _lds(32, 16, 64) == (20 * 1024, 9)
    assert _lds(16, 16, 64) == (12 * 1024 + 4096 + 3584, 12)
    assert _lds(0, 16, 64) == (20 * 1024, 16)
