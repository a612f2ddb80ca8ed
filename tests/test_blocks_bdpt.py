"""Connecting subpaths on the CPU: the host twin mtx_blocks_bdpt_host (the
per-lane functions of mtx_core/bdpt.h, which the kernel shares) against an
independent float64 restatement of contributions and Veach weights on fixed
polylines in the white furnace, the delta / connectability rules on hand-made
stores, the refusals and the ABI mirrors. No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import blocks_light_cases as blc
from conftest import ROOT
from mtx import _abi, blocks
from mtx._lib import MtxError

RHO, LE = 0.5, 1.5
D = 8  # vertex slots per store: polylines of up to 6 segments have 7 vertices

# The largest relative deviation of the twin (fp32 walk over fp32 stores) from
# the float64 restatement on the polylines below, measured on the CPU; the
# tests assert 4x this value (see test_weights_and_contributions_...).
MEASURED_REL = 9.4e-7
BOUND = 4.0 * MEASURED_REL


# ------------------------------------------------------------ the polylines --
def _walls(sc):
    """(centre, normal, two half-edge columns) of the furnace's six emitters, float64."""
    out = []
    for e in sc.emitters:
        out.append((np.array(e.center, np.float64), np.array(e.normal, np.float64), np.array(e.col0, np.float64),
                    np.array(e.col1, np.float64)))
    return out


def _cos(n, a, b):
    """cosine at a point with normal n of the direction a -> b."""
    d = b - a
    return float(n @ d / np.linalg.norm(d))


def polylines(sc, k, count, seed):
    """`count` polylines x_0 = camera, x_1 .. x_k on the walls, consecutive
    points on different walls, every cosine >= 0.2. Returns points
    (count, k + 1, 3), normals (count, k + 1, 3) and wall indices (count, k + 1)."""
    rng = np.random.default_rng(seed)
    walls = _walls(sc)
    origin = np.array(sc.camera.origin, np.float64)
    P, N, W = [], [], []
    while len(P) < count:
        pts, nrm, idx = [origin], [np.zeros(3)], [-1]
        while len(pts) <= k:
            w = int(rng.integers(len(walls)))
            c, n, c0, c1 = walls[w]
            x = c + c0 * rng.uniform(-0.95, 0.95) + c1 * rng.uniform(-0.95, 0.95)
            if w == idx[-1]:
                continue
            ok = _cos(n, x, pts[-1]) >= 0.2
            if len(pts) > 1:
                ok = ok and _cos(nrm[-1], pts[-1], x) >= 0.2
            if ok:
                pts.append(x)
                nrm.append(n)
                idx.append(w)
        P.append(pts)
        N.append(nrm)
        W.append(idx)
    return np.array(P), np.array(N), np.array(W)


def _local(n, v):
    """v (m, 3) in the shading frame of the unit normals n (m, 3)."""
    s, t = blc._frame(n)
    return np.stack([(s * v).sum(1), (t * v).sum(1), (n * v).sum(1)], 1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _g(pa, pb, nb):
    """|cos at b| / d^2 for the segment a -> b."""
    d = pb - pa
    d2 = (d * d).sum(-1)
    return np.abs((nb * d).sum(-1)) / np.sqrt(d2) / d2


def _dir_pdf(pa, na, pb):
    """cos / pi of the direction a -> b about the normal at a."""
    return np.maximum((na * _unit(pb - pa)).sum(-1), 0.0) / np.pi


def _empty_store(n):
    st = {"len": np.zeros(n, np.int32)}
    for k, c, dt in blocks._PATH_PLANES:
        st[k] = np.zeros(blocks._path_shape(D, c, n), getattr(np, dt))
    st["material"] -= 1
    st["emitter"] -= 1
    return st


def build_stores(sc, P, N, W, s, t, material=0):
    """The camera store (z_j = x_j, j < t) and the light store (y_i = x_{k-i},
    i < s) of the polylines, from the closed forms in float64, rounded to fp32."""
    m, nv = P.shape[0], P.shape[1]
    k = nv - 1
    assert s + t == nv and t >= 2
    pdf_pos = float(sc.emitters[0].inv_area) / len(sc.emitters)
    cam, lit = _empty_store(m), _empty_store(m)
    cam["len"][:] = t
    lit["len"][:] = s
    for j in range(t):
        cam["p"][j] = P[:, j].T
        cam["beta"][j] = RHO ** max(j - 1, 0)
        if j == 0:
            continue
        cam["n"][j] = cam["sh_n"][j] = N[:, j].T
        cam["wi"][j] = _local(N[:, j], _unit(P[:, j - 1] - P[:, j])).T
        cam["material"][j] = material
        cam["emitter"][j] = W[:, j]
        if j >= 2:
            cam["pdf_fwd"][j] = _dir_pdf(P[:, j - 1], N[:, j - 1], P[:, j]) * _g(P[:, j - 1], P[:, j], N[:, j])
        if 1 <= j <= t - 2:
            cam["pdf_rev"][j] = _dir_pdf(P[:, j + 1], N[:, j + 1], P[:, j]) * _g(P[:, j + 1], P[:, j], N[:, j])
    for i in range(s):
        x = k - i
        lit["p"][i] = P[:, x].T
        lit["n"][i] = lit["sh_n"][i] = N[:, x].T
        lit["emitter"][i] = W[:, x]
        if i == 0:
            lit["beta"][i] = LE / pdf_pos
            lit["pdf_fwd"][i] = pdf_pos
        else:
            lit["beta"][i] = LE * np.pi / pdf_pos * RHO ** (i - 1)
            lit["material"][i] = material
            lit["wi"][i] = _local(N[:, x], _unit(P[:, x + 1] - P[:, x])).T
            lit["pdf_fwd"][i] = _dir_pdf(P[:, x + 1], N[:, x + 1], P[:, x]) * _g(P[:, x + 1], P[:, x], N[:, x])
        if i <= s - 2:
            lit["pdf_rev"][i] = _dir_pdf(P[:, x - 1], N[:, x - 1], P[:, x]) * _g(P[:, x - 1], P[:, x], N[:, x])
    return cam, lit


def contribution64(sc, P, N, s, t):
    """C_{s,t} of the polylines in float64 (one channel: the furnace is grey)."""
    k = P.shape[1] - 1
    pdf_pos = float(sc.emitters[0].inv_area) / len(sc.emitters)
    beta_z = RHO ** (t - 2)
    if s == 0:
        return np.full(len(P), beta_z * LE)
    z, y = t - 1, k - (s - 1)  # polyline indices of the two ends
    d = P[:, y] - P[:, z]
    d2 = (d * d).sum(1)
    cos_z = (N[:, z] * _unit(d)).sum(1)
    cos_y = -(N[:, y] * _unit(d)).sum(1)
    f_z = RHO / np.pi * cos_z
    if s == 1:
        return beta_z * f_z / d2 * LE * cos_y / pdf_pos
    return beta_z * f_z / d2 * (RHO / np.pi * cos_y) * (LE * np.pi / pdf_pos * RHO ** (s - 2))


def weights64(sc, P, N, delta=None):
    """Veach's power-heuristic weights (exponent 2) of every strategy s' =
    0 .. k - 1 (t' >= 2) of the polylines, from the definition: the path
    density of each strategy as the product of its vertices' densities. With
    `delta` = m (a vertex index counted from the light), v_m is a delta
    vertex: the two densities sampled at it count as 1 and the strategies m
    and m + 1, which would connect at it, are left out (weight nan)."""
    nv = P.shape[1]
    k = nv - 1
    pdf_pos = float(sc.emitters[0].inv_area) / len(sc.emitters)
    v = lambda i: k - i  # noqa: E731  vertex i from the light = polyline index k - i
    pl, pc = [], []
    for i in range(nv - 2):  # the last two vertices are the camera's in every strategy
        if i == 0:
            pl.append(np.full(len(P), pdf_pos))
        else:
            a, b = v(i - 1), v(i)
            pl.append(np.ones(len(P)) if delta == i - 1 else _dir_pdf(P[:, a], N[:, a], P[:, b]) * _g(P[:, a], P[:, b], N[:, b]))
        a, b = v(i + 1), v(i)
        pc.append(np.ones(len(P)) if delta == i + 1 else _dir_pdf(P[:, a], N[:, a], P[:, b]) * _g(P[:, a], P[:, b], N[:, b]))
    dens = []
    for sp in range(nv - 1):
        p = np.ones(len(P))
        for i in range(nv - 2):
            p = p * (pl[i] if i < sp else pc[i])
        if delta is not None and sp in (delta, delta + 1):
            p = np.zeros(len(P))
        dens.append(p * p)
    dens = np.array(dens)
    w = dens / dens.sum(0)
    if delta is not None:
        w[[delta, delta + 1]] = np.nan
    return w  # (strategies, polylines)


_POLY = {}


def _polylines(sc, k):
    if k not in _POLY:
        _POLY[k] = polylines(sc, k, 12, 50 + k)
    return _POLY[k]


# ------------------------------------------------------------------- tests --
def test_weights_and_contributions_equal_float64_restatement():
    """White furnace, 12 polylines for each k = 2 .. 6 (60 in all), every
    split (s, t), t >= 2. The float64 weights of a path sum to 1 (1e-12); the
    twin's weight and its unweighted L equal the restatement.

    Tolerance: the largest relative deviation of the twin from the
    restatement on these polylines, measured on the CPU, is 9.34e-7 for the
    weights and 3.56e-7 for the contributions (the stores are fp32 roundings
    of the float64 closed forms, and the walk multiplies up to five fp32
    ratios and squares them). The test asserts 4x the larger value,
    MEASURED_REL above, and that the bound stays below 1e-4: beyond that the
    walk would be wrong, not rounded."""
    sc = blc.scene("furnace")
    assert len(sc.materials) == 1 and len(sc.emitters) == 6
    worst_w = worst_c = 0.0
    for k in range(2, 7):
        P, N, W = _polylines(sc, k)
        w64 = weights64(sc, P, N)
        assert np.abs(w64.sum(0) - 1.0).max() < 1e-12
        for s in range(0, k):
            t = k + 1 - s
            cam, lit = build_stores(sc, P, N, W, s, t)
            L, w = blocks.bdpt_host(sc, cam, lit, 6, s, t, mis=True)
            Lu, w1 = blocks.bdpt_host(sc, cam, lit, 6, s, t, mis=False)
            assert np.all(w1 == 1.0)
            c64 = contribution64(sc, P, N, s, t)
            assert np.all(c64 > 0)
            worst_w = max(worst_w, float(np.abs(w / w64[s] - 1.0).max()))
            worst_c = max(worst_c, float(np.abs(Lu / c64[None] - 1.0).max()))
            # the weighted L is the product of the two, rounded once
            assert np.abs(L / (Lu * w[None]) - 1.0).max() <= 2.0 ** -23
    print("largest relative deviation: weights %.3g, contributions %.3g" % (worst_w, worst_c))
    assert BOUND < 1e-4
    assert worst_w <= BOUND, worst_w
    assert worst_c <= BOUND, worst_c


def test_sum_of_all_strategies_is_the_weighted_sum():
    """s = t = -1 adds every strategy the two stores hold (here t' = 2, 3 and
    s' = 0, 1, 2): the sum of the single-strategy calls; max_depth leaves out
    the strategies with more segments."""
    sc = blc.scene("furnace")
    P, N, W = _polylines(sc, 4)
    cam, lit = build_stores(sc, P, N, W, 2, 3)
    total = blocks.bdpt_host(sc, cam, lit, 6)
    acc = np.zeros_like(total, dtype=np.float64)
    for t in (2, 3):
        for s in (0, 1, 2):
            acc += blocks.bdpt_host(sc, cam, lit, 6, s, t)[0]
    assert np.abs(total / acc - 1.0).max() < 1e-6
    # max_depth cuts the strategies with more segments
    short = blocks.bdpt_host(sc, cam, lit, 2)
    acc = sum(blocks.bdpt_host(sc, cam, lit, 6, s, t)[0].astype(np.float64) for s, t in ((0, 2), (0, 3), (1, 2)))
    assert np.abs(short / acc - 1.0).max() < 1e-6


def _glass_material(sc):
    return [i for i, m in enumerate(sc.materials) if m.type == _abi.MTX_MAT_DIELECTRIC][0]


def test_non_connectable_vertex_gives_zero():
    """A connection end whose material has no smooth lobe (the smooth
    dielectric of glass_dict, or no material at all) returns L = 0 and weight
    0, on either side; s = 0 does not need a connectable end."""
    from mtx.mitsuba_dict import scene_from_dict

    fsc = blc.scene("furnace")
    P, N, W = _polylines(fsc, 5)
    sc = scene_from_dict(blc.glass_dict())
    glass = _glass_material(sc)
    grey = [i for i, m in enumerate(sc.materials) if m.type == _abi.MTX_MAT_DIFFUSE][0]
    W0 = np.zeros_like(W)  # the scene's one emitter
    for s, t in ((2, 4), (3, 3), (1, 5)):
        cam, lit = build_stores(fsc, P, N, W0, s, t, material=grey)
        L, w = blocks.bdpt_host(sc, cam, lit, 6, s, t)
        assert np.all(L > 0) and np.all(w > 0)
        for store, idx in ((cam, t - 1), (lit, s - 1)):
            if store is lit and s == 1:
                continue  # y_0 is an emitter point: no BSDF is evaluated there
            for bad in (glass, -1):
                keep = store["material"][idx].copy()
                store["material"][idx] = bad
                L, w = blocks.bdpt_host(sc, cam, lit, 6, s, t)
                assert not L.any() and not w.any(), (s, t, bad)
                store["material"][idx] = keep
    cam, lit = build_stores(fsc, P, N, W0, 0, 6, material=grey)
    cam["material"][5] = glass
    L, w = blocks.bdpt_host(sc, cam, lit, 6, 0, 6)
    assert np.all(L > 0) and np.all(w > 0)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_delta_vertex_removes_its_two_strategies(m):
    """k = 5 (strategies s' = 0 .. 4). Vertex v_m (counted from the light) is
    marked delta in whichever store holds it: the weights of the remaining
    strategies equal the restatement without the strategies m and m + 1 and
    with the two densities sampled at v_m counted as 1, and sum to 1 within
    the bound of the first test."""
    sc = blc.scene("furnace")
    k = 5
    P, N, W = _polylines(sc, k)
    w64 = weights64(sc, P, N, delta=m)
    total = np.zeros(len(P))
    for s in range(0, k):
        if s in (m, m + 1):
            continue
        t = k + 1 - s
        cam, lit = build_stores(sc, P, N, W, s, t)
        if m < s:
            lit["delta"][m] = 1
        else:
            cam["delta"][k - m] = 1
        _, w = blocks.bdpt_host(sc, cam, lit, 6, s, t)
        assert np.abs(w / w64[s] - 1.0).max() <= BOUND, (s, t)
        total += w
    assert np.abs(total - 1.0).max() <= 4 * BOUND  # up to four weights, each within the bound
    # without the flag the same strategies' weights sum to less than 1: the two others take their share
    full = weights64(sc, P, N)
    assert np.all(np.delete(full, [m, m + 1], 0).sum(0) < 1.0 - 1e-6)


def test_refusals():
    sc = blc.scene("furnace")
    P, N, W = _polylines(sc, 4)
    cam, lit = build_stores(sc, P, N, W, 2, 3)
    with pytest.raises(MtxError, match="weight requested with s = t = -1"):
        blocks.bdpt_host(sc, cam, lit, 6, want_weight=True)
    with pytest.raises(MtxError, match="MTX_BDPT_VISIBILITY"):
        blocks.bdpt_host(sc, cam, lit, 6, 2, 3, flags=_abi.MTX_BDPT_MIS | _abi.MTX_BDPT_VISIBILITY)
    for t in (0, 1):
        with pytest.raises(MtxError, match="t >= 2"):
            blocks.bdpt_host(sc, cam, lit, 6, 1, t)
    with pytest.raises(MtxError, match="max_depth = 0"):
        blocks.bdpt_host(sc, cam, lit, 0, 2, 3)
    with pytest.raises(MtxError, match="depth mismatch"):
        short = {k: (v if k == "len" else v[: D - 1]) for k, v in lit.items()}
        blocks.bdpt_host(sc, cam, short, 6, 2, 3)
    with pytest.raises(MtxError, match="outside the stores' depth"):
        blocks.bdpt_host(sc, cam, lit, 6, D + 1, 2)
    # s > len for every lane: zeros, not an error
    L, w = blocks.bdpt_host(sc, cam, lit, 6, 3, 3)
    assert not L.any() and not w.any()
    L, w = blocks.bdpt_host(sc, cam, lit, 6, 2, 4)
    assert not L.any() and not w.any()
    # an index outside the tables is no material / no emitter
    cam["material"][2] = 7
    L, w = blocks.bdpt_host(sc, cam, lit, 6, 2, 3)
    assert not L.any() and not w.any()


def test_abi_mirrors(tmp_path):
    """mtx_path_planes as the C compiler lays it out, the enum, version 8."""
    import shutil
    import subprocess

    from mtx import _lib

    assert _lib.lib().mtx_abi_version() == _abi.MTX_ABI_VERSION == 8
    assert (_abi.MTX_BDPT_MIS, _abi.MTX_BDPT_VISIBILITY) == (1, 2)
    assert C.sizeof(_abi.PathPlanes) == 104
    for name in ("mtx_blocks_bdpt_connect_dev", "mtx_blocks_bdpt_host"):
        assert name in _abi.EXPORTS and hasattr(_lib.lib(), name)
    if not shutil.which("gcc"):
        return
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtx.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mtx_path_planes));',
             '  printf("enum %d\\n", MTX_BDPT_MIS + 16 * MTX_BDPT_VISIBILITY);']
    for f, _ in _abi.PathPlanes._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(mtx_path_planes, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        field, val = line.split()
        if field == "size":
            assert C.sizeof(_abi.PathPlanes) == int(val)
        elif field == "enum":
            assert int(val) == 1 + 16 * 2
        else:
            assert getattr(_abi.PathPlanes, field).offset == int(val), field
