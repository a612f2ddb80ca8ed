"""Reconstruction filters of the film (include/mtx_core/film.h): the host
entry points, the ABI mirror, the Python plumbing and the row-band stitch.
No GPU: mtx_rfilter_info / mtx_rfilter_eval are host-only and evaluate the
same MTX_HD functions the film kernels do."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_mitsuba_dict import cornell_box

FILTERS = {"tent": 0, "box": 1, "gaussian": 2}


def _eval(fid, r):
    from mtx._lib import lib

    r = np.ascontiguousarray(r, np.float32)
    w = np.full(r.shape, np.nan, np.float32)
    rc = lib().mtx_rfilter_eval(fid, r.ctypes.data, w.ctypes.data, r.size)
    assert rc == 0
    return w


def _grid():
    """r in [-3, 3] in steps of 1/32 (so ±0.5, ±1 and ±2 exactly) plus a few
    offsets that are no multiple of the step."""
    g = np.arange(-96, 97, dtype=np.float64) / 32.0
    extra = np.array([-1.9999, -1.37, -0.5000001, -0.4999999, 0.123456, 0.4999999, 0.5000001, 0.77, 1.9999])
    r = np.concatenate([g, extra]).astype(np.float32)
    for v in (0.5, 1.0, 2.0):
        assert (r == v).any() and (r == -v).any()
    return r


def test_rfilter_info():
    from mtx._lib import lib

    for fid, expect in ((0, (1, 1.0)), (1, (0, 0.5)), (2, (2, 2.0))):
        b, rad = C.c_uint32(99), C.c_float(-1)
        assert lib().mtx_rfilter_info(fid, C.byref(b), C.byref(rad)) == 0
        assert (b.value, rad.value) == expect
    b = C.c_uint32(99)
    assert lib().mtx_rfilter_info(3, C.byref(b), None) < 0
    assert b.value == 99
    assert b"filter" in lib().mtx_last_error()
    r = np.zeros(1, np.float32)
    assert lib().mtx_rfilter_eval(7, r.ctypes.data, r.ctypes.data, 1) < 0


def test_python_border_table_matches_the_library():
    from mtx import _abi, rfilter_border
    from mtx._lib import lib

    for name, fid in FILTERS.items():
        b = C.c_uint32()
        assert lib().mtx_rfilter_info(fid, C.byref(b), None) == 0
        assert _abi.RFILTERS[name] == fid
        assert rfilter_border(name) == rfilter_border(fid) == b.value == _abi.RFILTER_BORDER[fid]


def test_tent_and_box_are_exact():
    r = _grid()
    r64 = r.astype(np.float64)
    # 1 - |r| is exact in float64 for a float32 r, and its float32 rounding is
    # what the correctly rounded float32 subtraction returns
    tent = np.maximum(0.0, 1.0 - np.abs(r64))
    np.testing.assert_array_equal(_eval(0, r), tent.astype(np.float32))
    np.testing.assert_array_equal(_eval(1, r), (np.abs(r64) <= 0.5).astype(np.float32))


def test_gaussian_against_float64():
    r = _grid()
    r64 = r.astype(np.float64)
    ref = np.maximum(0.0, np.exp(-2.0 * r64 * r64) - np.exp(-8.0))
    w = _eval(2, r)
    # derived, not measured: weights <= 1, dexp is pinned to 5e-7 relative
    # (test_core_math.py), two exp terms plus one rounding of the subtraction
    np.testing.assert_allclose(w, ref, rtol=0, atol=1.2e-6)
    assert (w[np.abs(r) >= 2] == 0).all()
    assert (w[np.abs(r) < 1.99] > 0).all()
    np.testing.assert_array_equal(w, _eval(2, -r))


def test_render_args_mirror():
    from mtx import _abi, load_dict
    from mtx._lib import MtxError

    names = [n for n, _ in _abi.RenderArgs._fields_]
    assert "rfilter" in names and "reserved" not in names
    assert _abi.RenderArgs.rfilter.offset == 76 and _abi.RenderArgs.rfilter.size == 4
    assert names[-1] == "rfilter"
    assert C.sizeof(_abi.RenderArgs) == 80
    assert _abi.MTX_ABI_VERSION == 8

    class S:  # render_args reads the size and the declared filter only
        width, height, rfilter = 8, 4, "gaussian"

    integ = load_dict({"type": "path_test"})
    assert integ.render_args(S, 1, 2).rfilter == 0  # the default stays the tent
    assert integ.render_args(S, 1, 2, rfilter="gaussian").rfilter == 2
    assert integ.render_args(S, 1, 2, rfilter="box").rfilter == 1
    assert integ.render_args(S, 1, 2, rfilter="scene").rfilter == 2
    assert load_dict({"type": "restirgi", "rfilter": "box"}).render_args(S, 1, 1).rfilter == 1
    assert load_dict({"type": "pssmlt", "rfilter": "scene"}).render_args(S, 1, 1).rfilter == 2
    assert load_dict({"type": "nrc", "rfilter": "scene"}).render_args(S, 1, 1, rfilter="tent").rfilter == 0
    with pytest.raises(MtxError, match="mitchell"):
        integ.render_args(S, 1, 2, rfilter="mitchell")


def test_scene_resolves_the_declared_filter(small_scene):
    from mtx import load_dict
    from mtx._lib import MtxError
    from mtx.mitsuba_dict import scene_from_dict

    sc = scene_from_dict(cornell_box(16, 16))
    assert sc.rfilter == "gaussian"
    assert small_scene.rfilter == "tent"
    assert sc.with_film(8, 8).rfilter == "gaussian"
    assert sc.with_camera(sc.camera).rfilter == "gaussian"
    assert copy.copy(sc).rfilter == "gaussian"
    integ = load_dict({"type": "path_test", "rfilter": "scene"})
    assert integ.render_args(sc, 1, 1).rfilter == 2
    assert integ.render_args(small_scene, 1, 1).rfilter == 0
    d = cornell_box(16, 16)
    d["sensor"]["film"]["rfilter"] = {"type": "box"}
    assert integ.render_args(scene_from_dict(d), 1, 1).rfilter == 1
    d["sensor"]["film"]["rfilter"] = {"type": "mitchell"}
    other = scene_from_dict(d)
    assert other.rfilter == "mitchell"
    with pytest.raises(MtxError, match="mitchell"):
        integ.render_args(other, 1, 1)
    # an explicit filter overrides the declaration; the default ignores it
    assert integ.render_args(other, 1, 1, rfilter="box").rfilter == 1
    assert load_dict({"type": "path_test"}).render_args(other, 1, 1).rfilter == 0


def test_scene_filter_survives_save_and_load(tmp_path):
    from mtx.mitsuba_dict import scene_from_dict
    from mtx.scene import Scene

    sc = scene_from_dict(cornell_box(8, 8))
    sc.save(str(tmp_path / "s.npz"))
    assert Scene.load(str(tmp_path / "s.npz")).rfilter == "gaussian"


@pytest.mark.parametrize("border", [0, 1, 2])
def test_develop_crops_by_the_border(border):
    from mtx import develop
    from mtx._lib import MtxError

    H, W = 5, 7
    rng = np.random.default_rng(border)
    film = rng.random((H + 2 * border, W + 2 * border, 4)).astype(np.float32) + 0.5
    film[border, border, 3] = 0.0  # a pixel without weight develops to 0
    inner = film[border: border + H, border: border + W]
    img = develop(film, border=border)
    assert img.shape == (H, W, 3) and img.dtype == np.float32
    expect = inner[..., :3] / np.where(inner[..., 3:4] != 0, inner[..., 3:4], 1)
    expect[0, 0] = 0
    np.testing.assert_array_equal(img, expect.astype(np.float32))
    if border == 1:
        np.testing.assert_array_equal(develop(film), img)  # the default border is the tent's
    with pytest.raises(MtxError):
        develop(film, border=(H + 2 * border + 1) // 2)  # nothing would be left


@pytest.mark.parametrize("border", [0, 1, 2])
def test_band_stitch(border):
    """Band films cut from a known decomposition add up to the full film:
    band i's film is the part of the full film its own pixels contribute,
    i.e. non-zero only on rows [y0 - border, y1 + border)."""
    import torch

    from mtx.distributed import row_bands, stitch_bands

    H, W, b = 11, 5, border
    bands = row_bands(H, 3)
    assert bands[0][0] == 0 and bands[-1][1] == H
    g = torch.Generator().manual_seed(7 + b)
    maxrows = max(y1 - y0 for y0, y1 in bands) + 2 * b
    parts, full = [], torch.zeros((H + 2 * b, W + 2 * b, 4), dtype=torch.float64)
    for y0, y1 in bands:
        rows = y1 - y0 + 2 * b
        # integers: the sum is exact in any order
        band = torch.randint(1, 100, (rows, W + 2 * b, 4), generator=g).to(torch.float64)
        full[y0: y0 + rows] += band
        padded = torch.full((maxrows, W + 2 * b, 4), float("nan"), dtype=torch.float64)  # padding is never read
        padded[:rows] = band
        parts.append(padded)
    out = stitch_bands(parts, bands, H, b)
    assert out.shape == full.shape
    assert torch.equal(out, full)
    if b == 0:  # the bands abut: every row comes from exactly one band
        for (y0, y1), p in zip(bands, parts):
            assert torch.equal(out[y0:y1], p[: y1 - y0])
