"""Connecting subpaths on the GPU: k_blk_bdpt_connect against its CPU twin
(mtx_blocks_bdpt_host) bit for bit on stores the real recorder wrote, its
shadow rays against scene.ray_test, and the bidirectional path tracer
("bdpt") held to the white furnace's closed form, strategy by strategy, and to
the fused path_test estimator of the same integral.

Statistics as in test_blocks_light_gpu.py: K = 16 independent renders per
estimator, block means, z = difference over the combined standard error from
the spread over the renders, |z| < 5.5."""
import numpy as np
import pytest

import blocks_light_cases as blc

pytestmark = pytest.mark.gpu

LANES = (1, 63, 64, 65, 257)
K = 16


@pytest.fixture(scope="module")
def lat(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lattice_bdpt_gpu"))


def _dict_scene(d, base_dir=None):
    from mtx.mitsuba_dict import scene_from_dict

    return scene_from_dict(d, base_dir=base_dir)


def _strategies(max_depth):
    return [(s, t) for t in range(2, max_depth + 2) for s in range(0, max_depth + 2 - t)]


def _record(sc, n, seed, max_depth=5):
    """(Scene, camera store, light store) of n lanes: the recorder of the
    "bdpt" integrator on rays through random film positions."""
    import torch

    from mtx import blocks

    integ = blocks.BidirectionalPathTracer({"max_depth": max_depth})
    sens = blocks.Sensor(sc)
    scn = blocks.Scene(sens.scene, sens.ctx.device)
    lanes = torch.arange(n, dtype=torch.int32, device="cuda")
    sampler = blocks.Sampler(seed, lanes)
    u = sampler.next_2d()
    pos = torch.stack([u[0] * sens.width, u[1] * sens.height])
    cam = blocks.PathVertices(pos.device, max_depth + 1, n)
    lit = blocks.PathVertices(pos.device, max_depth + 1, n)
    integ.record_camera(scn, sampler, sens.sample_ray(pos), cam)
    integ.record_light(scn, sampler, lit)
    return scn, cam, lit


def _mask(n):
    m = np.random.default_rng(n).random(n) < 0.6
    m[: min(n, 3)] = [True, False, True][: min(n, 3)]
    return m


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


SCENES = {
    "cornell": lambda lat: _dict_scene(blc.cornell_dict(16, 16)),
    "lattice": lambda lat: blc.scene("lattice", lat),
    "glass": lambda lat: _dict_scene(blc.glass_dict()),
}


# --------------------------------------------------- kernel against the twin --
@pytest.mark.parametrize("name", list(SCENES))
def test_kernel_equals_host_twin(name, lat):
    """Visibility off, max_depth 5, stores from the recorder: every single
    strategy (L and weight) and the sum of all equal the twin's bit patterns,
    with and without an `active` mask (a masked-off lane: zeros)."""
    import torch

    from mtx import blocks

    sc = SCENES[name](lat)
    M = 5
    some_l = some_w = 0
    for n in LANES:
        scn, cam, lit = _record(sc, n, 200 + n, M)
        hc, hl = cam.host(), lit.host()
        m = _mask(n)
        tm = torch.as_tensor(m, device="cuda")
        for s, t in _strategies(M) + [(None, None)]:
            for mis in (True, False):
                want = blocks.bdpt_host(sc, hc, hl, M, s, t, mis=mis)
                got = blocks.connect_subpaths(scn, cam, lit, M, s, t, mis=mis, test_visibility=False)
                got_m = blocks.connect_subpaths(scn, cam, lit, M, s, t, mis=mis, test_visibility=False, active=tm)
                if s is None:
                    want, got, got_m = (want,), (got,), (got_m,)
                for a, b, c in zip(want, got, got_m):
                    assert np.array_equal(_bits(b), a.view(np.uint32)), (name, n, s, t, mis)
                    masked = a.copy()
                    masked[..., ~m] = 0.0
                    assert np.array_equal(_bits(c), masked.view(np.uint32)), (name, n, s, t, mis, "active")
                some_l += int((want[0] != 0).sum())
                if s is not None and mis:
                    w = want[1]
                    assert np.all((w >= 0) & (w <= 1))
                    some_w += int(((w > 0) & (w < 1)).sum())
    assert some_l > 0  # the comparison is not one of zeros
    if name != "lattice":  # its sheets light nothing the camera sees: s = 0 alone contributes, with weight 1
        assert some_w > 0


@pytest.mark.parametrize("name", list(SCENES))
def test_visibility_zeroes_exactly_the_occluded_lanes(name, lat):
    """Visibility on: per single strategy, L is zero exactly on the lanes
    whose shadow ray spawn_ray_to(z.p, z.n, y.p) scene.ray_test reports
    occluded, among the lanes with a non-zero unoccluded L, and unchanged
    elsewhere (s = 0 has no connection edge). The Cornell box has both kinds."""
    from mtx import blocks

    sc = SCENES[name](lat)
    M = 5
    n_occ = n_vis = 0
    for n in LANES + (2048,):
        scn, cam, lit = _record(sc, n, 700 + n, M)
        for s, t in _strategies(M):
            free, w0 = blocks.connect_subpaths(scn, cam, lit, M, s, t, test_visibility=False)
            got, w1 = blocks.connect_subpaths(scn, cam, lit, M, s, t, test_visibility=True)
            assert np.array_equal(_bits(w0), _bits(w1))
            lit_up = (free != 0).any(0)
            expect = free.clone()
            if s >= 1:
                si = blocks.SurfaceInteraction(free.device, n)
                si.p, si.n = cam.p[t - 1].contiguous(), cam.n[t - 1].contiguous()
                o, d, maxt = si.spawn_ray_to(lit.p[s - 1].contiguous())
                occ = scn.ray_test(o, d, maxt, active=lit_up)
                expect[:, occ] = 0.0
                n_occ += int(occ.sum())
                n_vis += int((lit_up & ~occ).sum())
            assert np.array_equal(_bits(got), _bits(expect)), (name, n, s, t)
    if name != "lattice":  # its sheets light nothing the camera sees: no connection carries anything
        assert n_vis > 0
    if name == "cornell":
        assert n_occ > 0


# ------------------------------------------------------------ determinism --
def test_bdpt_is_deterministic():
    from mtx import load_dict

    sc = blc.scene("furnace")
    integ = load_dict({"type": "bdpt", "max_depth": 4})
    a = integ.render_film(sc, seed=3, spp=8, rfilter="box").cpu().numpy()
    b = integ.render_film(sc, seed=3, spp=8, rfilter="box").cpu().numpy()
    c = integ.render_film(sc, seed=3, spp=8, rfilter="box", max_lanes=5000).cpu().numpy()
    band = integ.render_film(sc, seed=3, spp=8, rfilter="box", y0=5, y1=13).cpu().numpy()
    other = integ.render_film(sc, seed=4, spp=8, rfilter="box").cpu().numpy()
    assert a.shape == (32, 32, 4) and np.isfinite(a).all() and a[..., :3].sum() > 0
    assert np.array_equal(a, b)
    assert np.array_equal(a, c)
    assert np.array_equal(band, a[5:13])
    assert not np.array_equal(a, other)


def test_load_dict_renders_the_cornell_box():
    from mtx import blocks, load_dict

    integ = load_dict({"type": "bdpt", "max_depth": 16, "rr_depth": 2})
    assert isinstance(integ, blocks.BidirectionalPathTracer) and integ.max_depth == 16
    img = integ.render(_dict_scene(blc.cornell_dict(32, 32)), spp=16).cpu().numpy()
    assert img.shape == (32, 32, 3) and np.isfinite(img).all() and img.mean() > 0.05


# ---------------------------------------------------------------- renders --
def _img(integ, scene, seed, spp):
    return integ.render(scene, seed=seed, spp=spp, rfilter="box").cpu().numpy().astype(np.float64)


def _single(s, t):
    from mtx import blocks

    class Single(blocks.BidirectionalPathTracer):
        def connect(self, scene, camera, light):
            return blocks.connect_subpaths(scene, camera, light, self.max_depth, s, t, mis=False)[0]

    return Single


FURNACE = dict(rho=0.5, Le=1.5, M=5, spp=256)
FURNACE_CASES = [None, (0, 3), (1, 2), (2, 2), (3, 2), (2, 3), (1, 4)]


@pytest.mark.parametrize("strategy", FURNACE_CASES, ids=lambda v: "sum" if v is None else "s%dt%d" % v)
def test_furnace_closed_form(strategy):
    """furnace_spec(0.5, 1.5, res=32), max_depth M = 5, K = 16 renders of 256
    samples per pixel. The weighted sum of all strategies is Le (1 - rho^M) /
    (1 - rho); a single strategy (s, t), rendered unweighted, is Le
    rho^(s+t-2): 8x8 block means and the image mean within 5.5 standard
    errors. A wrong density, or weights that do not sum to 1, is a bias here.

    The standard errors are those of test_ptracer_white_furnace_closed_form:
    the scene and the camera are symmetric under the square's eight
    symmetries, so the four corner blocks of the 4 x 4 grid are identically
    distributed, as are the eight edge and the four centre blocks, and each
    class pools its blocks' sample variances (60, 120 and 60 degrees of
    freedom instead of 15). That matters for the unweighted strategies whose
    connection can be short, (1, 4) and (2, 3): cos cos / d^2 is unbounded
    where both ends approach a common edge of the box, the estimator's
    variance is not finite, and a block that drew no such sample
    underestimates its own spread. With per-block variances and 64 samples
    per pixel the first GPU run of this test measured max |z| = 5.68 and a z
    of the mean of -3.59 for (1, 4) (mean 0.18411 against 0.1875), every
    other case below 4.6. (0, 3) has next to no variance: every camera path
    meets an emitting wall, so every sample is Le rho exactly.

    The weighted sum carries a bias this test can see: -2.2e-4 of its value
    (measured with 8 x 1024 samples per pixel: 2.905608 against 2.906250),
    from spawn_ray's offset of 1.8e-4, which the sampled densities contain
    and the connection geometry does not ("Connecting subpaths").
    With these 16 x 256 samples the z of the image mean is -4.64."""
    from mtx import blocks
    from test_gpu_convergence import _blocks

    f = FURNACE
    sc = blc.scene("furnace")
    props = {"max_depth": f["M"]}
    if strategy is None:
        integ = blocks.BidirectionalPathTracer(props)
        expect = f["Le"] * (1 - f["rho"] ** f["M"]) / (1 - f["rho"])
    else:
        integ = _single(*strategy)(props)
        expect = f["Le"] * f["rho"] ** (strategy[0] + strategy[1] - 2)
    imgs = np.stack([_img(integ, sc, 40 + k, f["spp"]) for k in range(K)])
    assert np.isfinite(imgs).all()
    x = np.stack([_blocks(i, 8) for i in imgs])
    m, var = x.mean(0), x.var(0, ddof=1)
    ring = np.minimum(np.arange(4), 3 - np.arange(4))
    cls = ring[:, None] + ring[None, :]  # 0 corner, 1 edge, 2 centre
    pooled = np.zeros_like(var)
    for c in range(3):
        pooled[cls == c] = var[cls == c].mean(0)
    z = (m - expect) / np.sqrt(pooled / K + 1e-24)
    means = imgs.mean(axis=(1, 2, 3))
    mean = means.mean()
    zm = (mean - expect) / (means.std(ddof=1) / np.sqrt(K) + 1e-12)
    print("furnace %s: expect %.5f mean %.5f z_mean %.2f max|z| %.2f" % (strategy, expect, mean, zm, np.abs(z).max()))
    assert np.abs(z).max() < 5.5, float(np.abs(z).max())
    assert abs(zm) < 5.5, (float(mean), expect, float(zm))


# scene, max_depth and block size of test_blocks_light_gpu.AGREE (restated; `sky` is a refusal here), bdpt spp
AGREE = {
    "cornell": (5, 8, 256),
    "lattice": (4, 4, 256),
    "glass": (5, 8, 256),
    "immersed": (4, 8, 256),
    "bumpy": (4, 8, 256),
    "bedroom": (4, 4, 128),
}


def _fused(name, lat):
    """The K path_test renders of the scene: those test_blocks_light_gpu
    compares its particle tracer with (same seeds, spp, rr_depth), rendered
    once per session whichever module asks first."""
    import test_blocks_light_gpu as tlg
    from mtx import load_dict

    build, M, _b, _spp_p, spp_f = tlg.AGREE[name]
    assert M == AGREE[name][0]
    sc = build(lat)
    if name not in tlg._FUSED:
        fused = load_dict({"type": "path_test", "max_depth": M, "rr_depth": 3})
        tlg._FUSED[name] = np.stack([tlg._fused_img(fused, sc, 900 + k, spp_f) for k in range(K)])
    return sc, tlg._FUSED[name]


def _agreement(name, lat, cls=None):
    from mtx import blocks
    from test_blocks_light_gpu import _block_stats
    from test_gpu_convergence import _z

    M, b, spp = AGREE[name]
    sc, f = _fused(name, lat)
    integ = (cls or blocks.BidirectionalPathTracer)({"max_depth": M})
    a = np.stack([_img(integ, sc, 500 + k, spp) for k in range(K)])
    assert np.isfinite(a).all() and np.isfinite(f).all()
    (bd, bd_mean), (pm, pm_mean) = _block_stats(a, b), _block_stats(f, b)
    z = _z(bd, pm)
    zm = (bd_mean[0] - pm_mean[0]) / np.sqrt(bd_mean[1] ** 2 + pm_mean[1] ** 2)
    print("%s: means %.5f %.5f z_mean %.2f max|z| %.2f" % (name, bd_mean[0], pm_mean[0], zm, np.abs(z).max()))
    return float(np.abs(z).max()), float(zm), float(bd_mean[0]), float(pm_mean[0])


@pytest.mark.parametrize("name", list(AGREE))
def test_bdpt_agrees_with_path_test(name, lat):
    """bdpt against the fused path_test at equal max_depth, box filter, K = 16
    renders each: every block |z| < 5.5 and the image means within 5.5
    combined standard errors. The scenes are those of
    test_blocks_light_gpu.test_ptracer_agrees_with_path_test, whose docstring
    says what each one pins (rectangles and cubes; mesh emitters; delta
    vertices that every contributing path crosses; a refraction that does not
    cancel; shading normals; textures, plastics and rough conductors)."""
    zmax, zm, mean_b, mean_f = _agreement(name, lat)
    assert mean_b > 0 and mean_f > 0
    assert zmax < 5.5, (name, zmax)
    assert abs(zm) < 5.5, (name, mean_b, mean_f, zm)


def test_weights_are_pinned(lat):
    """All weights 1, strategies summed: every path is counted once per
    strategy that can make it, many standard errors from path_test where the
    weighted sum agrees (the margin of test_adjoint_correction_is_pinned)."""
    from mtx import blocks

    class Unweighted(blocks.BidirectionalPathTracer):
        def connect(self, scene, camera, light):
            return blocks.connect_subpaths(scene, camera, light, self.max_depth, mis=False)

    zmax, _zm, _b, _f = _agreement("cornell", lat, Unweighted)
    assert zmax > 11.0, zmax


# ---------------------------------------------------------------- refusals --
def test_refusals():
    import torch

    from mtx import blocks, load_dict
    from mtx._lib import MtxError
    from test_blocks_light_gpu import _rough_glass_scene

    with pytest.raises(MtxError, match="environment"):
        load_dict({"type": "bdpt"}).render_film(blc.scene("sky"), spp=1)
    with pytest.raises(MtxError, match="roughdielectric"):
        load_dict({"type": "bdpt"}).render_film(_rough_glass_scene(), spp=1)
    with pytest.raises(MtxError, match="max_depth"):
        load_dict({"type": "bdpt", "max_depth": 0})
    with pytest.raises(MtxError, match="max_depth"):
        load_dict({"type": "bdpt", "max_depth": float("inf")})

    sc = blc.scene("furnace")
    scn, cam, lit = _record(sc, 64, 1, 4)
    keep = cam.beta
    cam.beta = keep.cpu()
    with pytest.raises(MtxError, match=r"camera\.beta: a host tensor"):
        blocks.connect_subpaths(scn, cam, lit, 4)
    cam.beta = keep[:, :2].contiguous()
    with pytest.raises(MtxError, match=r"camera\.beta: shape .* expected \(5, 3, 64\)"):
        blocks.connect_subpaths(scn, cam, lit, 4)
    cam.beta = keep
    lit.len = lit.len[:63].contiguous()
    with pytest.raises(MtxError, match=r"light\.len: shape"):
        blocks.connect_subpaths(scn, cam, lit, 4)
    other = blocks.PathVertices(cam.device, 4, 64)
    with pytest.raises(MtxError, match="depth mismatch"):
        blocks.connect_subpaths(scn, cam, other, 4)
    other = blocks.PathVertices(cam.device, 5, 32)
    with pytest.raises(MtxError, match="lanes"):
        blocks.connect_subpaths(scn, cam, other, 4)
    # a store on another device: a second GPU if there is one, else a store that says so
    other = blocks.PathVertices(cam.device, 5, 64)
    if torch.cuda.device_count() > 1:
        other = blocks.PathVertices(torch.device("cuda", 1), 5, 64)
    else:
        other.device = torch.device("cuda", cam.device.index + 1)
    with pytest.raises(MtxError, match=r"on cuda:\d"):
        blocks.connect_subpaths(scn, cam, other, 4)
    other = blocks.PathVertices(cam.device, 5, 64)
    with pytest.raises(MtxError, match="t >= 2"):
        blocks.connect_subpaths(scn, cam, other, 4, 1, 1)
    with pytest.raises(MtxError, match="give both"):
        blocks.connect_subpaths(scn, cam, other, 4, s=1)
    with pytest.raises(MtxError, match="max_depth"):
        blocks.connect_subpaths(scn, cam, other, 0)
    with pytest.raises(MtxError, match="lanes"):
        blocks.connect_subpaths(scn, cam, other, 4, active=torch.ones(63, dtype=torch.bool, device="cuda"))
    # an index past the scene's tables: reported, and handled as none
    other.material[1] = 99
    other.len[:] = 2
    with pytest.raises(MtxError, match="past the scene's tables"):
        blocks.connect_subpaths(scn, cam, other, 4)
