"""Box and gaussian reconstruction filters on the GPU (mtx_render_args.rfilter).

The reference film is a numpy float32 restatement, written here, of the order
in DESIGN.md "Film": samples fall into slots by film_slot, each source pixel
sums its samples (ascending) into K = (2n+1)^2 accumulators, a film pixel
gathers its K neighbours in (dy, dx) order, and the slots combine by
film_tree8. Every step is one elementwise float32 operation, so there is no
fused multiply-add in it. Its inputs are the oracle's per-sample (L, pos);
the gaussian's exp is the oracle's dexp. With the tent it equals the oracle's
own film bit for bit (test_restatement_equals_the_oracle_film), which anchors
the helper before it judges the new filters.

ReSTIR GI and PSSMLT put at integer positions, so every tap's weight is a
constant: the tent film follows exactly from the box film (weights 1/4,
a power of two), and the gaussian film is a fixed 5x5 convolution of it.
"""
import ctypes as C

import numpy as np
import pytest

F32 = np.float32
TENT, BOX, GAUSSIAN = 0, 1, 2
REACH = {TENT: 1, BOX: 0, GAUSSIAN: 2}
NAMES = {"tent": TENT, "box": BOX, "gaussian": GAUSSIAN}


# ------------------------------------------------------------ restatement --
def _weight(oracle, fid, r):
    """rfilter_eval (mtx_core/film.h) on a float32 array, one axis."""
    assert r.dtype == F32
    if fid == TENT:
        return np.maximum(F32(0), F32(1) - np.abs(r))
    if fid == BOX:
        return (np.abs(r) <= F32(0.5)).astype(F32)
    alpha = F32(-2.0)
    bias = oracle.dmath("exp", np.array([alpha * F32(4.0)], F32))[0]
    e = oracle.dmath("exp", (alpha * (r * r)).astype(F32).reshape(-1)).reshape(r.shape)
    return np.maximum(F32(0), e - bias)


def _film_slot(g, T):
    k = 0
    while k < 7 and (((k + 1) * T) >> 3) <= g:
        k += 1
    return k


def _gather(acc, n):
    """acc [D, D, rows, W, 4] -> film [rows + 2n, W + 2n, 4]: a film pixel adds
    its neighbours' accumulators in (dy, dx) ascending order, starting at 0."""
    D = 2 * n + 1
    rows, W = acc.shape[2], acc.shape[3]
    film = np.zeros((rows + 2 * n, W + 2 * n, 4), F32)
    for dy in range(D):
        for dx in range(D):
            film[dy: dy + rows, dx: dx + W] = film[dy: dy + rows, dx: dx + W] + acc[dy, dx]
    return film


def film_np(oracle, fid, width, y0, y1, spp, L, pos, spp_total=None, sample_offset=0, nslots=8):
    n = REACH[fid]
    D = 2 * n + 1
    rows, W = y1 - y0, width
    T = spp if spp_total is None else spp_total
    L = np.asarray(L, F32).reshape(rows, W, spp, 3)
    pos = np.asarray(pos, F32).reshape(rows, W, spp, 2)
    xs = np.broadcast_to(np.arange(W, dtype=np.int64)[None, :], (rows, W))
    ys = np.broadcast_to(np.arange(y0, y1, dtype=np.int64)[:, None], (rows, W))
    NS = 8 if nslots == 8 else 1
    acc = np.zeros((NS, D, D, rows, W, 4), F32)
    for k in range(spp):
        s = _film_slot(sample_offset + k, T) if NS == 8 else 0
        sx, sy = pos[:, :, k, 0], pos[:, :, k, 1]
        wx = [_weight(oracle, fid, sx - ((xs + dx - n).astype(F32) + F32(0.5))) for dx in range(D)]
        wy = [_weight(oracle, fid, sy - ((ys + dy - n).astype(F32) + F32(0.5))) for dy in range(D)]
        for dy in range(D):
            for dx in range(D):
                w = wx[dx] * wy[dy]
                a = acc[s, dy, dx]
                for c in range(3):
                    a[..., c] = a[..., c] + L[:, :, k, c] * w
                a[..., 3] = a[..., 3] + w
    assert acc.dtype == F32
    sl = [_gather(acc[s], n) for s in range(NS)]
    if NS == 1:
        return sl[0]
    return ((sl[0] + sl[1]) + (sl[2] + sl[3])) + ((sl[4] + sl[5]) + (sl[6] + sl[7]))


# name -> render arguments (all on the 64x36 small scene)
CASES = {
    "plain_spp3": dict(spp=3),                                 # k_film_src, some slots empty
    "staged_spp12": dict(spp=12),                              # staged kernel, stages of 8 + 4
    "sample_shard": dict(spp=4, spp_total=16, sample_offset=4),
    "row_band": dict(spp=5, y0=8, y1=20),
    "odd_chunks": dict(spp=4, y0=0, y1=36, chunk_paths=400),   # 100-pixel chunks: no multiple of 64
}


@pytest.fixture(scope="module")
def samples(small_scene, oracle):
    """The oracle's per-sample (L, pos) of a case, computed once per case."""
    from mtx import load_dict

    cache = {}

    def get(integrator, case):
        key = (integrator, case)
        if key not in cache:
            kw = {k: v for k, v in CASES[case].items() if k != "chunk_paths"}
            a = load_dict({"type": integrator}).render_args(small_scene, 3, **kw)
            L, pos = oracle.render_samples(small_scene, a)
            L.setflags(write=False)
            pos.setflags(write=False)
            cache[key] = (a, L, pos)
        return cache[key]

    return get


def _restated(oracle, fid, scene, a, L, pos):
    return film_np(oracle, fid, scene.width, a.y0, a.y1, a.spp, L, pos, a.spp_total, a.sample_offset, 8)


@pytest.mark.parametrize("case", ["plain_spp3", "sample_shard", "row_band"])
def test_restatement_equals_the_oracle_film(small_scene, oracle, samples, case):
    """Anchor: with the tent, the numpy restatement is the oracle's film."""
    a, L, pos = samples("path_test", case)
    np.testing.assert_array_equal(_restated(oracle, TENT, small_scene, a, L, pos), oracle.render(small_scene, a))


@pytest.mark.gpu
@pytest.mark.parametrize("rfilter", ["box", "gaussian"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_path_test_film_bit_exact(small_scene, oracle, samples, case, rfilter):
    from mtx import load_dict

    a, L, pos = samples("path_test", case)
    ref = _restated(oracle, NAMES[rfilter], small_scene, a, L, pos)
    film = load_dict({"type": "path_test"}).render_film(small_scene, seed=3, rfilter=rfilter, **CASES[case])
    b = REACH[NAMES[rfilter]]
    assert film.shape == (a.y1 - a.y0 + 2 * b, small_scene.width + 2 * b, 4)
    np.testing.assert_array_equal(film, ref)
    assert film[..., 3].sum() > 0 and film[..., :3].sum() > 0
    if rfilter == "box":  # every sample lands in its own pixel with weight 1
        np.testing.assert_array_equal(film[..., 3], F32(a.spp))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mypath", "nrc", "integrator"])
def test_other_integrators_gaussian_bit_exact(small_scene, oracle, name):
    from mtx import load_dict

    integ = load_dict({"type": name, "rfilter": "gaussian"})  # the property, not the argument
    a = integ.render_args(small_scene, 5, 4)
    assert a.rfilter == GAUSSIAN
    L, pos = oracle.render_samples(small_scene, a)
    film = integ.render_film(small_scene, seed=5, spp=4)
    np.testing.assert_array_equal(film, _restated(oracle, GAUSSIAN, small_scene, a, L, pos))
    assert film[..., :3].sum() > 0


# ------------------------------------------- integer positions: ReSTIR, MLT --
def _check_box_precondition(B):
    """Scaling by 1/4 commutes with float32 rounding unless it underflows."""
    assert np.isfinite(B).all()
    nz = np.abs(B[B != 0])
    assert nz.size and nz.min() >= 2.0 ** -120


def tent_from_box(B):
    """The tent film of puts at integer positions from their box film: the
    position (x, y) is the corner of pixels x-1..x, y-1..y, so the taps
    (dy, dx) in {0, 1}^2 of the 3x3 footprint weigh 1/2 * 1/2 and the others
    0; gathered in (dy, dx) order."""
    rows, W = B.shape[0], B.shape[1]
    acc = np.zeros((3, 3, rows, W, 4), F32)
    q = B * F32(0.25)
    for dy in (0, 1):
        for dx in (0, 1):
            acc[dy, dx] = q
    return _gather(acc, 1)


def gaussian_from_box64(oracle, B):
    """float64 5x5 convolution of the box film with the gaussian's constant
    tap weights at an integer position: offsets 1.5 - d, d = 0..4."""
    g = _weight(oracle, GAUSSIAN, (F32(1.5) - np.arange(5, dtype=F32)).astype(F32))
    assert g[4] == 0 and (g[:4] > 0).all()
    w = (g[:, None] * g[None, :]).astype(np.float64)  # the float32 products the kernel forms
    rows, W = B.shape[0], B.shape[1]
    out = np.zeros((rows + 4, W + 4, 4), np.float64)
    B64 = B.astype(np.float64)
    for dy in range(5):
        for dx in range(5):
            out[dy: dy + rows, dx: dx + W] += w[dy, dx] * B64
    return out


RESTIR = {"jacobian": False, "bias_correction": True, "max_M_spatial": 500, "max_M_temporal": 30}


def _restir_oracle(oracle, scene, frames, spp):
    from mtx import load_dict

    integ = load_dict({"type": "restirgi", **RESTIR})
    orc = oracle.RestirOracle(scene, spp)
    out = []
    for fr in range(frames):
        integ.n = fr
        out.append(orc.frame(scene, integ.render_args(scene, fr, spp)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 2])
def test_restir_box_and_gaussian(small_scene, oracle, spp):
    from mtx import load_dict

    sc, frames = small_scene, 3
    ref = _restir_oracle(oracle, sc, frames, spp)
    box = load_dict({"type": "restirgi", "rfilter": "box", **RESTIR})
    B = [box.render_film(sc, seed=fr, spp=spp) for fr in range(frames)]
    for fr in range(frames):
        assert B[fr].shape == (sc.height, sc.width, 4)
        _check_box_precondition(B[fr])
        np.testing.assert_array_equal(tent_from_box(B[fr]), ref[fr], err_msg=f"frame {fr}")
        np.testing.assert_array_equal(B[fr][..., 3], F32(spp))  # spp = 1: all ones
    gauss = load_dict({"type": "restirgi", **RESTIR})
    rtol = (spp + 25) * 2.0 ** -23  # P = spp puts per pixel, 25 taps, all terms >= 0
    for fr in range(frames):
        G = gauss.render_film(sc, seed=fr, spp=spp, rfilter="gaussian")
        assert G.shape == (sc.height + 4, sc.width + 4, 4)
        assert (B[fr] >= 0).all()
        np.testing.assert_allclose(G, gaussian_from_box64(oracle, B[fr]), rtol=rtol, atol=0, err_msg=f"frame {fr}")


@pytest.mark.gpu
@pytest.mark.parametrize("rfilter", ["box", "gaussian"])
def test_restir_row_bands_stitch(small_scene, rfilter):
    """A row-banded frame (stage A, halo exchange, stage B; two contexts stand
    in for two ranks) stitched with the filter's border is the whole frame:
    bit for bit with the box (the bands abut), and within the summation bound
    of non-negative terms where the gaussian's borders overlap."""
    import torch

    from mtx import distributed, load_dict
    from mtx._lib import Context

    sc = small_scene.with_film(40, 26)
    props = dict(RESTIR, initial_search_radius=6.0, rfilter=rfilter)
    b = REACH[NAMES[rfilter]]
    frames = 2
    full = load_dict({"type": "restirgi", **props})
    ref = [full.render_film(sc, seed=fr, spp=1) for fr in range(frames)]
    bands = distributed.row_bands(sc.height, 2)
    ctxs = [Context(0), Context(0)]
    integs = [load_dict({"type": "restirgi", **props}) for _ in bands]
    halo = distributed.restir_halo(integs[0])
    io = [distributed.device_row_io(integs[k], sc, 1, ctxs[k]) for k in range(2)]
    for fr in range(frames):
        for k, (y0, y1) in enumerate(bands):
            integs[k].render_film(sc, seed=fr, spp=1, y0=y0, y1=y1, stage="A", ctx=ctxs[k])
        for k, (y0, y1) in enumerate(bands):
            _, _, recv_up, recv_down = distributed.halo_plan(y0, y1, sc.height, halo)
            for which in ("sample", "temporal"):
                for row0, nrows in (recv_up, recv_down):
                    if nrows:
                        io[k][1](which, row0, io[1 - k][0](which, row0, nrows))
        parts = []
        for k, (y0, y1) in enumerate(bands):
            f = integs[k].render_film(sc, seed=fr, spp=1, y0=y0, y1=y1, stage="B", ctx=ctxs[k])
            assert f.shape == (y1 - y0 + 2 * b, sc.width + 2 * b, 4)
            parts.append(torch.from_numpy(f))
        stitched = distributed.stitch_bands(parts, bands, sc.height, b).numpy()
        assert ref[fr][..., :3].sum() > 0
        if b == 0:
            np.testing.assert_array_equal(stitched, ref[fr], err_msg=f"frame {fr}")
        else:
            assert (ref[fr] >= 0).all()
            np.testing.assert_allclose(stitched, ref[fr], rtol=(1 + 25) * 2.0 ** -23, atol=0, err_msg=f"frame {fr}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pssmlt_simple", "pssmlt"])
def test_pssmlt_box_and_gaussian(small_scene, oracle, name):
    from mtx import load_dict

    sc, iters, chains, y0, y1 = small_scene, 60, 4, 12, 20
    integ = load_dict({"type": name, "iterations": iters})
    ref = oracle.pssmlt_render(sc, integ.render_args(sc, 2, chains, y0=y0, y1=y1), iters)
    B = integ.render_film(sc, seed=2, spp=chains, y0=y0, y1=y1, rfilter="box")
    assert B.shape == (y1 - y0, sc.width, 4)
    _check_box_precondition(B)
    np.testing.assert_array_equal(tent_from_box(B), ref)
    puts = chains * sum(1 for it in range(iters) if it % 50 > 40)  # per pixel (pssmlt.py:210)
    np.testing.assert_array_equal(B[..., 3], F32(puts))
    G = integ.render_film(sc, seed=2, spp=chains, y0=y0, y1=y1, rfilter="gaussian")
    assert G.shape == (y1 - y0 + 4, sc.width + 4, 4)
    assert (B >= 0).all()
    np.testing.assert_allclose(G, gaussian_from_box64(oracle, B), rtol=(puts + 25) * 2.0 ** -23, atol=0)


# ------------------------------------------------------------- the default --
@pytest.mark.gpu
def test_default_is_the_tent_and_unknown_ids_are_refused(small_scene, oracle, samples):
    from mtx import _abi, load_dict
    from mtx._lib import context, lib

    integ = load_dict({"type": "path_test"})
    a, _, _ = samples("path_test", "plain_spp3")
    plain = integ.render_film(small_scene, seed=3, spp=3)
    tent = integ.render_film(small_scene, seed=3, spp=3, rfilter="tent")
    np.testing.assert_array_equal(plain, tent)
    np.testing.assert_array_equal(plain, oracle.render(small_scene, a))
    # declared filters change nothing unless asked for
    assert plain.shape == (small_scene.height + 2, small_scene.width + 2, 4)

    bad = integ.render_args(small_scene, 3, 3)
    bad.rfilter = 7
    film = np.full((small_scene.height + 4, small_scene.width + 4, 4), -1.0, F32)
    rc = lib().mtx_render(context().handle, C.byref(bad), film.ctypes.data, 0, None)
    assert rc < 0 and _abi.ERRORS[rc] == "MTX_E_ARG"
    assert b"filter" in lib().mtx_last_error()
    assert (film == -1.0).all()
