"""The class queues of the shade kernel (csrc/shade.hip shade_loop<INT, CAM, CLS>,
include/mtx_core/shade_class.h), the parts that need no GPU:

* the material type -> shading class mapping covers every MTX_MAT_*;
* the class of every triangle of the small bedroom, as mtx_scene_upload
  writes it into the shading records, equals a numpy restatement from
  tri_shape -> shapes.material -> materials.type;
* the rings of a shade block fit three blocks into a CU's 160 KB of LDS;
* MTX_SHADE_CLASSES takes 0 and 1 and nothing else;
* the ring bookkeeping of a block (ingest ranks, pick rule, drain), restated
  in numpy over synthetic class sequences: every queue position is shaded
  exactly once, no ring ever holds more than its 512 slots or overwrites a
  live entry, a ring stays in queue order, every step before the drain holds
  one class, and the drain takes at most ceil(remaining / 256) steps.
"""
import ctypes as C

import numpy as np
import pytest

from mtx import _abi
from mtx._lib import lib

BLOCK = 256
MAT_TYPES = {name: getattr(_abi, name) for name in dir(_abi) if name.startswith("MTX_MAT_")}


def _class_of_type(t):
    fn = lib().mtx_diag_shade_class_of_type
    fn.argtypes, fn.restype = [C.c_uint32], C.c_uint32
    return int(fn(t))


def _knob(value):
    fn = lib().mtx_diag_shade_classes_knob
    fn.argtypes, fn.restype = [C.c_char_p, C.POINTER(C.c_uint32)], C.c_int
    out = (C.c_uint32 * 4)()
    rc = fn(value, out)
    return rc, list(out)


def test_every_material_type_has_a_class():
    assert len(MAT_TYPES) == 6, MAT_TYPES
    n_classes = _knob(b"1")[1][3]
    assert n_classes == 3
    want = {"MTX_MAT_DIFFUSE": 0, "MTX_MAT_ROUGHPLASTIC": 1, "MTX_MAT_CONDUCTOR": 2, "MTX_MAT_ROUGHCONDUCTOR": 2,
            "MTX_MAT_DIELECTRIC": 2, "MTX_MAT_ROUGHDIELECTRIC": 2}
    assert set(want) == set(MAT_TYPES)
    for name, t in MAT_TYPES.items():
        assert _class_of_type(t) == want[name], name
        assert _class_of_type(t) < n_classes


def test_triangle_classes_of_the_small_bedroom(small_scene):
    sc = small_scene
    fn = lib().mtx_diag_shade_classes
    fn.argtypes, fn.restype = [C.POINTER(_abi.SceneDesc), C.c_void_p], C.c_int
    n = len(sc.tri_shape)
    got = np.full(n, 255, np.uint8)
    d = sc.desc()
    assert fn(C.byref(d), got.ctypes.data) == 0
    shape_mat = np.array([sh.material for sh in sc.shapes], np.int64)
    mat_type = np.array([m.type for m in sc.materials], np.int64)
    t = mat_type[shape_mat[sc.tri_shape]]
    want = np.where(t == _abi.MTX_MAT_DIFFUSE, 0, np.where(t == _abi.MTX_MAT_ROUGHPLASTIC, 1, 2)).astype(np.uint8)
    assert np.array_equal(got, want)
    assert set(np.unique(want)) == {0, 1, 2}  # the scene the GPU tests sort has all three


def test_rings_fit_three_blocks_per_cu():
    rc, (knob, lds, ring, classes) = _knob(b"1")
    assert rc == 0 and knob == 1
    assert ring == 2 * BLOCK and lds == classes * ring * 24
    # three blocks' rings and the static LDS of the shade step (the append's
    # counters: below 256 B) in a CU's 160 KB
    assert 3 * (lds + 256) <= 160 * 1024
    assert lds <= 64 * 1024  # a launch needs no opt-in to large dynamic LDS


def test_knob_takes_zero_and_one_only():
    assert _knob(b"0")[:1] == (0,) and _knob(b"0")[1][0] == 0
    assert _knob(b"1")[1][0] == 1
    for bad in (b"2", b"-1", b"", b"01", b"1x", b"on", b" 1"):
        rc, _ = _knob(bad)
        assert rc == -1, bad  # MTX_E_ARG
        assert b"MTX_SHADE_CLASSES" in lib().mtx_last_error()


# ---------------------------------------------------------------------------
# The CLS form of shade_loop for one block, restated: `cls` holds the class of every
# queue position of the block's windows in the order the block ingests them.
# ---------------------------------------------------------------------------
def _run_block(cls, n_classes=3, ring=2 * BLOCK):
    cls = np.asarray(cls, np.int64)
    n = len(cls)
    store = np.full((n_classes, ring), -1, np.int64)  # queue position per slot, -1: free
    head = [0] * n_classes
    fill = [0] * n_classes
    nbase = 0
    steps = []  # (drain, positions)
    max_fill = 0
    while True:
        while True:
            c = max(range(n_classes), key=lambda k: (fill[k], -k))  # the fullest ring, the lowest class on a tie
            most, held = fill[c], sum(fill)
            if most >= BLOCK or nbase >= n:
                break
            pos = np.arange(nbase, min(nbase + BLOCK, n))
            for k in range(n_classes):
                mine = pos[cls[pos] == k]  # in lane order: the rank is stable in the queue position
                slots = (head[k] + fill[k] + np.arange(len(mine))) % ring
                assert (store[k, slots] == -1).all(), "an ingest overwrote a live entry"
                store[k, slots] = mine
                fill[k] += len(mine)
                assert fill[k] <= ring
            max_fill = max(max_fill, max(fill))
            nbase += BLOCK
        if held == 0:
            break
        took = []
        if most >= BLOCK:
            slots = (head[c] + np.arange(BLOCK)) % ring
            took = list(store[c, slots])
            store[c, slots] = -1
            head[c] = (head[c] + BLOCK) % ring
            fill[c] -= BLOCK
            steps.append((False, took))
        else:
            assert nbase >= n, "a packed step while the queue still has windows"
            room = BLOCK
            for k in range(n_classes):
                take = min(fill[k], room)
                slots = (head[k] + np.arange(take)) % ring
                took += list(store[k, slots])
                store[k, slots] = -1
                head[k] = (head[k] + take) % ring
                fill[k] -= take
                room -= take
            steps.append((True, took))
    assert (store == -1).all()
    return steps, max_fill


def _sequences():
    rng = np.random.default_rng(5)
    yield "empty", np.zeros(0, np.int64)
    yield "one", np.array([2])
    yield "below a step", rng.choice(3, 200, p=[0.73, 0.25, 0.02])
    yield "one class, 4 windows", np.zeros(4 * BLOCK, np.int64)
    yield "one class, partial last window", np.full(3 * BLOCK + 17, 1)
    yield "bedroom shares", rng.choice(3, 40 * BLOCK + 99, p=[0.729, 0.251, 0.02])
    yield "even thirds", rng.choice(3, 25 * BLOCK, p=[1 / 3, 1 / 3, 1 / 3])
    yield "round robin", np.arange(12 * BLOCK + 5) % 3
    # two rings one short of a step after two windows (255 / 255 / 2), then a
    # whole window of one of those classes: the fullest a ring gets
    yield "rings nearly full", np.concatenate([np.repeat([0, 1], 128), np.repeat([0, 1, 2], [127, 127, 2]),
                                               np.full(BLOCK, 0), np.full(BLOCK, 1), np.full(BLOCK, 2)])
    yield "runs", np.repeat(rng.choice(3, 60), rng.integers(1, 700, 60))


@pytest.mark.parametrize("name,cls", list(_sequences()), ids=[n for n, _ in _sequences()])
def test_ring_bookkeeping(name, cls):
    steps, max_fill = _run_block(cls)
    n = len(cls)
    shaded = np.concatenate([np.asarray(t, np.int64) for _, t in steps]) if steps else np.zeros(0, np.int64)
    assert len(shaded) == n and np.array_equal(np.sort(shaded), np.arange(n)), "every position exactly once"
    assert max_fill <= 2 * BLOCK
    drains = [t for d, t in steps if d]
    for d, t in steps:
        if not d:
            assert len(t) == BLOCK and len(set(cls[t])) == 1, "a step before the drain holds one class"
    # the drain comes last and packs what is left
    flags = [d for d, _ in steps]
    assert flags == sorted(flags)
    left = sum(len(t) for t in drains)
    assert len(drains) == -(-left // BLOCK)
    # inside a class the queue order is kept
    for k in range(3):
        mine = shaded[cls[shaded] == k]
        assert np.array_equal(mine, np.sort(mine))
    if name == "rings nearly full":
        assert max_fill == 2 * BLOCK - 1  # 255 held, a window of 256 of that class on top
