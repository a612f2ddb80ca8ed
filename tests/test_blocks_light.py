"""The two light-path functions of mtx_core (sample_emitter_ray,
camera_sample_direction) through the host probe mtx_blocks_light_host, the
bit-exact CPU twin of the kernels (tests/test_blocks_light_gpu.py holds the
kernels to it): against a float64 transcription within derived bounds,
against closed forms, and by the statistics of their distributions. No GPU.

z-tests use the project's threshold |z| < 5.5 (a normal tail beyond it has
probability 4e-8) with the sample count N written in each test."""
import numpy as np
import pytest

import blocks_light_cases as blc
from mtx import _abi, blocks
from mtx._lib import MtxError

N_STAT = 1 << 16


@pytest.fixture(scope="module")
def lat(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lattice_light"))


_RAYS = {}


def _emitter_rays(kind, lat):
    """(samples, probe result, transcription) of N_STAT samples, computed once."""
    if kind not in _RAYS:
        sc = blc.scene(kind, lat)
        u = blc.samples(N_STAT, 11 + blc.KINDS.index(kind))
        got = blc.unpack_emitter_ray(blocks.light_host(sc, _abi.MTX_LIGHT_EMITTER_RAY, u))
        _RAYS[kind] = (u, got, blc.emitter_ray_f64(sc, u))
    return _RAYS[kind]


@pytest.mark.parametrize("kind", blc.KINDS)
def test_emitter_ray_matches_float64_transcription(kind, lat):
    _, got, ref = _emitter_rays(kind, lat)
    blc.check_emitter_ray(got, ref)
    assert ref["side_ambiguous"].mean() < 0.01


@pytest.mark.parametrize("kind", blc.KINDS)
def test_emitter_ray_weight_is_the_emitter_power(kind, lat):
    """weight = count * Le * pi * A_e for every sample of emitter e (4 pi^2
    r^2 for the sky): constant per emitter, so the mean weight is the scene's
    total power. Bound: blocks_light_cases.WEIGHT_AREA_REL."""
    sc = blc.scene(kind, lat)
    _, got, _ = _emitter_rays(kind, lat)
    count = blc.emitter_count(sc)
    power = 0.0
    for e in range(count):
        sel = got["emitter"] == e
        assert sel.any()
        if e == len(sc.emitters):
            _, r = blc.env_sphere64(sc)
            want = blc.radiance(sc, e) * 4.0 * np.pi ** 2 * r * r
        else:
            want = blc.radiance(sc, e) * np.pi * blc.emitter_area_centroid(sc, e)[0]
        power += want
        w = got["weight"][sel].astype(np.float64)
        assert np.all(w == w[0]), "the weight of one emitter's samples is one value"
        assert np.all(np.abs(w[0] / (want * count) - 1.0) <= blc.WEIGHT_AREA_REL), (e, w[0], want * count)
    mean = got["weight"].astype(np.float64).mean(0)
    # the mean over N samples of the per-emitter constants: pick frequencies within 5.5 sigma
    p = 1.0 / count
    tol = 5.5 * np.sqrt(p * (1 - p) / N_STAT) * count if count > 1 else 16 * blc.E
    assert np.all(np.abs(mean / power - 1.0) <= tol + 16 * blc.E)


@pytest.mark.parametrize("kind", blc.KINDS)
def test_emitter_ray_distributions(kind, lat):
    """N = 65536 samples: pick frequencies against 1 / count, the mean position
    of every emitter against its area-weighted centroid, E[cos] = 2 / 3 of the
    cosine-hemisphere directions (variance 1 / 18); every direction leaves on
    the normal's side, and the sky's point inwards."""
    sc = blc.scene(kind, lat)
    _, got, _ = _emitter_rays(kind, lat)
    count, n_area = blc.emitter_count(sc), len(sc.emitters)
    em = got["emitter"]
    assert em.min() >= 0 and em.max() == count - 1
    p = 1.0 / count
    if count > 1:
        z = (np.bincount(em, minlength=count) - N_STAT * p) / np.sqrt(N_STAT * p * (1 - p))
        assert np.abs(z).max() < 5.5, z
    pos = got["p"].astype(np.float64)
    for e in range(n_area):
        x = pos[em == e]
        _, centroid = blc.emitter_area_centroid(sc, e)
        se = x.std(0, ddof=1) / np.sqrt(len(x))
        flat = se < 1e-6  # the coordinate the emitter's plane fixes
        assert np.all(np.abs(x.mean(0) - centroid)[flat] < 1e-5)
        assert np.all(np.abs((x.mean(0) - centroid)[~flat] / se[~flat]) < 5.5), (e, x.mean(0), centroid)
    d, n = got["d"].astype(np.float64), got["n"].astype(np.float64)
    cos = np.sum(d * n, 1)
    assert np.all(cos > 0)
    assert abs(cos.mean() - 2.0 / 3.0) / np.sqrt(1.0 / 18.0 / N_STAT) < 5.5
    assert np.all(np.abs(np.linalg.norm(d, axis=1) - 1.0) < 1e-5)
    if n_area < count:
        c, r = blc.env_sphere64(sc)
        sky = em == n_area
        o = got["o"].astype(np.float64)[sky]
        assert np.all(np.sum(d[sky] * (o - c), 1) < 0)
        assert np.all(np.abs(np.linalg.norm(o - c, axis=1) / r - 1.0) < 1e-5)
        # uniform on the sphere: the mean of the unit position vector is 0, each component's variance 1 / 3
        z = ((o - c) / r).mean(0) / np.sqrt(1.0 / 3.0 / sky.sum())
        assert np.abs(z).max() < 5.5


def test_emitter_ray_without_emitters_gives_zeros():
    import copy

    sc = copy.copy(blc.scene("furnace"))
    sc.emitters = (_abi.Emitter * 0)()
    sc.env_radiance = None
    out = blocks.light_host(sc, _abi.MTX_LIGHT_EMITTER_RAY, blc.samples(64, 1))
    assert not out[:16].any()
    assert np.all(np.ascontiguousarray(out[16]).view(np.int32) == -1)


def test_probe_refuses_bad_arguments():
    sc = blc.scene("furnace")
    with pytest.raises(MtxError, match="unknown op"):
        blocks.light_host(sc, 7, np.zeros((3, 4), np.float32))
    with pytest.raises(MtxError, match="expected"):
        blocks.light_host(sc, _abi.MTX_LIGHT_EMITTER_RAY, np.zeros((3, 4), np.float32))


@pytest.mark.parametrize("kind", blc.KINDS)
def test_sensor_direction_round_trip(kind, lat):
    """Points on the camera rays of a 9 x 9 film grid (corners and edges
    included) at seven depths from the near to the far clip project back to
    their film position; points behind the camera, beyond the far clip, before
    the near clip and outside the frustum are invalid with weight 0; random
    points around the camera agree with the transcription; the film position
    equals project_prev's bit for bit."""
    sc = blc.scene(kind, lat)
    pts, grid, cls = blc.sensor_points(sc)
    raw = blocks.light_host(sc, _abi.MTX_LIGHT_SENSOR_DIRECTION, pts)
    got = blc.unpack_sensor_direction(raw)
    ref = blc.sensor_direction_f64(sc, pts)
    blc.check_sensor_direction(got, ref)
    assert ref["ambiguous"].mean() < 0.2  # the film's edges and corners are thresholds by construction
    assert got["valid"][cls == 1].all() and not got["valid"][cls == 0].any()
    assert not got["weight"][cls == 0].any()
    # the round trip: the transcription's position for the fp32 point is the grid position up to the
    # point's rounding (E |p| per component) through the projection: d pos = size / (2 lz tan) per unit
    # of lx, (1 + |q| tan) with the depth's share; the probe is within b_pos of the transcription.
    c = blc.camera64(sc)
    inner = cls == 1
    lz = ((pts.T.astype(np.float64) - c["origin"]) @ c["rows"][2])[inner]
    reach = np.sqrt(3.0) * blc.E * np.abs(pts.T.astype(np.float64)).max(1)[inner]
    slack = max(c["size"]) * reach * (1.0 + 1.0) / (2.0 * lz * min(c["tan"]))
    err = np.abs(got["pos"][inner].astype(np.float64) - grid[inner]).max(1)
    assert np.all(err <= ref["b_pos"][inner] + slack), float((err - ref["b_pos"][inner] - slack).max())
    proj = blocks.light_host(sc, _abi.MTX_LIGHT_PROJECT, pts)
    assert np.array_equal(proj[:2].view(np.uint32), raw[:2].view(np.uint32))
    assert np.array_equal(proj[2].view(np.uint32), raw[7].view(np.uint32))


def test_importance_integrates_to_one():
    """int W_e dA over the image plane = 1. On the plane z = 1 of the camera
    frame a film cell of area dA subtends cos^3 dA, and importance = 1 / (A
    cos^3): the integrand importance * cos^3 is the constant 1 / A, so the
    midpoint rule on a 64 x 64 grid has no quadrature error and the tolerance
    is rounding alone: per term the weight's bound (rel_weight, about 70 E at
    the corners) plus the point's own rounding through cos^3 and dist^2
    (5 sqrt(3) E); 128 E covers both. cos is computed here from the film
    position, not from the probe's direction."""
    sc = blc.scene("furnace")
    c = blc.camera64(sc)
    g = (np.arange(64) + 0.5) / 64
    pos01 = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    o, d, cz = blc.camera_ray_f64(sc, pos01)
    pts = np.ascontiguousarray((o + d * 0.75).T, np.float32)
    got = blc.unpack_sensor_direction(blocks.light_host(sc, _abi.MTX_LIGHT_SENSOR_DIRECTION, pts))
    assert got["valid"].all()
    importance = got["weight"].astype(np.float64) * got["dist"].astype(np.float64) ** 2
    x = (1.0 - 2.0 * pos01[:, 0]) * c["tan"][0]
    y = (1.0 - 2.0 * pos01[:, 1]) * c["tan"][1]
    cos3 = (1.0 + x * x + y * y) ** -1.5
    cell = 4.0 * c["tan"][0] * c["tan"][1] / len(pos01)
    terms = importance * cos3 * cell * len(pos01)
    assert np.all(np.abs(terms - 1.0) <= 128 * blc.E), float(np.abs(terms - 1.0).max())
    assert abs((importance * cos3 * cell).sum() - 1.0) <= 128 * blc.E
