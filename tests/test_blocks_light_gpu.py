"""Light paths on the GPU: the kernels of scene.sample_emitter_ray and
sensor.sample_direction against their CPU twin (mtx_blocks_light_host) bit
for bit, the calls' refusals, and the particle tracer ("ptracer") held to the
white furnace's closed form and to the fused path_test estimator of the same
integral, which uses the emitter and sensor formulas the other way round.

Statistics as in test_gpu_convergence.py: K independent renders per
estimator, block means, z = difference over the combined standard error from
the spread over the renders, |z| < 5.5."""
import numpy as np
import pytest

import blocks_light_cases as blc

pytestmark = pytest.mark.gpu

LANES = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def lat(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lattice_light_gpu"))


def _dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else torch.as_tensor(
        np.ascontiguousarray(a), device="cuda").to(dtype)


def _emitter_ray_planes(ray, w, es):
    import torch

    em = es.emitter.view(torch.float32)[None]
    return torch.cat([ray.o, ray.d, ray.maxt[None], w, es.p, es.n, em]).cpu().numpy()


def _mask(n):
    m = np.random.default_rng(n).random(n) < 0.6
    m[: min(n, 3)] = [True, False, True][: min(n, 3)]
    return m


# ------------------------------------------------ kernels against the probe --
@pytest.mark.parametrize("kind", blc.KINDS)
def test_sample_emitter_ray_equals_host_probe(kind, lat):
    from mtx import _abi, blocks

    sc = blc.scene(kind, lat)
    scn = blocks.Scene(sc)
    for n in LANES:
        u = blc.samples(n, 100 + n)
        want = blocks.light_host(sc, _abi.MTX_LIGHT_EMITTER_RAY, u)
        got = _emitter_ray_planes(*scn.sample_emitter_ray(_dev(u[:2]), _dev(u[2:])))
        assert np.array_equal(got, want), (kind, n)
        assert np.array_equal(got[16].view(np.int32), want[16].view(np.int32))
    n = 257
    u, m = blc.samples(n, 7), _mask(n)
    want = blocks.light_host(sc, _abi.MTX_LIGHT_EMITTER_RAY, u)
    want[:16, ~m] = 0.0
    want[16, ~m] = np.array(-1, np.int32).view(np.float32)
    got = _emitter_ray_planes(*scn.sample_emitter_ray(_dev(u[:2]), _dev(u[2:]), _dev(m)))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), kind


def _sensor_planes(sd):
    import torch

    return torch.cat([sd.pos, sd.d, sd.dist[None], sd.weight[None]]).cpu().numpy(), sd.valid.cpu().numpy()


def _connection_points(sc, n, seed):
    """n points with normals: emitter samples (points of the scene's lights,
    which the scene's own geometry may hide from the camera) interleaved with
    the grid / outside / random points of the CPU test, their normal the
    direction to the camera."""
    from mtx import _abi, blocks

    es = blocks.light_host(sc, _abi.MTX_LIGHT_EMITTER_RAY, blc.samples(n, seed))
    pts, _, _ = blc.sensor_points(sc)
    pick = np.random.default_rng(seed).permutation(pts.shape[1])[:n]
    p, nrm = es[10:13].copy(), es[13:16].copy()
    to_cam = np.array(sc.camera.origin, np.float32)[:, None] - pts[:, pick]
    p[:, 1::2], nrm[:, 1::2] = pts[:, pick][:, 1::2], to_cam[:, 1::2]
    return np.ascontiguousarray(p), np.ascontiguousarray(nrm)


@pytest.mark.parametrize("kind", blc.KINDS)
def test_sensor_direction_equals_host_probe(kind, lat):
    """Without test_visibility every plane equals the probe's. With it the
    weight of exactly the lanes that scene.ray_test reports occluded on
    spawn_ray_to(p, n, origin) is zero and nothing else changes."""
    from mtx import _abi, blocks

    sc = blc.scene(kind, lat)
    scn, sens = blocks.Scene(sc), blocks.Sensor(sc)
    origin = np.array(sc.camera.origin, np.float32)
    n_occ = n_vis = 0
    for n in LANES + (2048,):
        p, nrm = _connection_points(sc, n, 300 + n)
        want = blocks.light_host(sc, _abi.MTX_LIGHT_SENSOR_DIRECTION, p)
        wv = want[7].view(np.uint32) != 0
        tp, tn = _dev(p), _dev(nrm)
        got, valid = _sensor_planes(sens.sample_direction(tp, tn, test_visibility=False))
        assert np.array_equal(got, want[:7]) and np.array_equal(valid, wv), (kind, n)
        si = blocks.SurfaceInteraction(tp.device, n)
        si.p, si.n = tp, tn
        o, d, maxt = si.spawn_ray_to(_dev(np.repeat(origin[:, None], n, 1)))
        occ = scn.ray_test(o, d, maxt, active=_dev(wv)).cpu().numpy()
        got_v, valid_v = _sensor_planes(sens.sample_direction(tp, tn, test_visibility=True))
        expect = want[:7].copy()
        expect[6, occ] = 0.0
        assert np.array_equal(got_v, expect) and np.array_equal(valid_v, wv), (kind, n)
        n_occ += int(occ.sum())
        n_vis += int((wv & ~occ).sum())
    assert n_vis > 0
    if kind != "furnace":  # the furnace's camera sees every wall point
        assert n_occ > 0
    n = 257
    p, nrm = _connection_points(sc, n, 9)
    m = _mask(n)
    want = blocks.light_host(sc, _abi.MTX_LIGHT_SENSOR_DIRECTION, p)
    want[:, ~m] = 0.0
    got, valid = _sensor_planes(sens.sample_direction(_dev(p), _dev(nrm), False, _dev(m)))
    assert np.array_equal(got.view(np.uint32), want[:7].view(np.uint32))
    assert np.array_equal(valid, want[7].view(np.uint32) != 0)


# ---------------------------------------------------------------- refusals --
def _rough_glass_scene():
    from mtx.mitsuba_dict import scene_from_dict

    d = blc.cornell_dict(16, 16)
    d["frosted"] = {"type": "roughdielectric", "alpha": 0.2, "int_ior": 1.5, "ext_ior": 1.0}
    d["small-box"] = dict(d["small-box"], bsdf={"type": "ref", "id": "frosted"})
    return scene_from_dict(d)


def test_refusals():
    import torch

    from mtx import blocks, load_dict
    from mtx._lib import MtxError

    sc = blc.scene("furnace")
    scn, sens = blocks.Scene(sc), blocks.Sensor(sc)
    u2 = torch.rand((2, 8), device="cuda")
    p3 = torch.rand((3, 8), device="cuda")
    with pytest.raises(MtxError, match="host tensor"):
        scn.sample_emitter_ray(u2.cpu(), u2)
    with pytest.raises(MtxError, match="host tensor"):
        sens.sample_direction(p3, p3.cpu())
    with pytest.raises(MtxError, match=r"expected \(2, N\)"):
        scn.sample_emitter_ray(p3, u2)
    with pytest.raises(MtxError, match=r"expected \(3, N\)"):
        sens.sample_direction(u2, p3)
    with pytest.raises(MtxError, match="lanes"):
        scn.sample_emitter_ray(u2, u2, torch.ones(7, dtype=torch.bool, device="cuda"))
    with pytest.raises(MtxError, match="lanes"):
        sens.sample_direction(p3, p3, True, torch.ones(9, dtype=torch.bool, device="cuda"))
    with pytest.raises(MtxError, match="roughdielectric"):
        load_dict({"type": "ptracer"}).render_film(_rough_glass_scene(), spp=1)
    with pytest.raises(MtxError, match="gaussian"):
        load_dict({"type": "ptracer"}).render_film(sc, spp=1, rfilter="gaussian")


# ------------------------------------------------------------- the renders --
def _ptracer_img(integ, scene, seed, spp):
    return integ.render(scene, seed=seed, spp=spp, rfilter="box").cpu().numpy().astype(np.float64)


def _fused_img(integ, scene, seed, spp):
    from mtx import develop

    return develop(integ.render_film(scene, seed=seed, spp=spp, rfilter="box"), 0).astype(np.float64)


def _block_stats(imgs, b):
    """(block means, their standard errors), (image mean, its standard error) over the K renders `imgs`."""
    from test_gpu_convergence import _blocks

    K = len(imgs)
    x = np.stack([_blocks(i, b) for i in imgs])
    means = x.reshape(K, -1).mean(1)
    return (x.mean(0), x.std(0, ddof=1) / np.sqrt(K)), (means.mean(), means.std(ddof=1) / np.sqrt(K))


def test_ptracer_is_deterministic():
    from mtx import load_dict

    sc = blc.scene("furnace")
    integ = load_dict({"type": "ptracer", "max_depth": 4, "rr_depth": 2, "samples_per_pass": 5000})
    a = integ.render_film(sc, seed=3, spp=8).cpu().numpy()
    b = integ.render_film(sc, seed=3, spp=8).cpu().numpy()
    c = integ.render_film(sc, seed=4, spp=8).cpu().numpy()
    assert a.shape == (32, 32, 4) and np.isfinite(a).all() and a[..., :3].sum() > 0
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    assert np.all(a[..., 3] == 1.0)


FURNACE = dict(rho=0.5, Le=1.5, M=6, spp=4096, K=4)


@pytest.mark.parametrize("hide", [False, True])
def test_ptracer_white_furnace_closed_form(hide):
    """furnace_spec(0.5, 1.5, res=32), M = 6, rr_depth 2: every pixel is
    Le (1 - rho^M) / (1 - rho), minus Le with hide_emitters. K = 4 renders of
    4096 particles per pixel: 8x8 blocks within 5.5 standard errors of the
    closed form, and the image mean within 5.5 of its own standard error.

    A render of 4096 particles per pixel is four passes of 2^20 particles.
    Each pass is rendered here with a seed of its own (16 renders of 1024
    particles per pixel) and a render is the mean of four of them, so the
    passes themselves are 16 independent samples of the image mean: its
    standard error has 15 degrees of freedom, and a Student t of 15 passes
    5.5 with probability 6e-5 for a correct estimator (from the four renders
    alone it would be a t of 3: 1.2 %).

    A block's standard error comes from the spread over the K = 4 renders.
    The scene and the camera are symmetric under the square's eight
    symmetries about the view axis, so the four corner blocks of the 4 x 4
    grid are identically distributed, as are the eight edge blocks and the
    four centre blocks: each class pools its blocks' sample variances (12, 24
    and 12 degrees of freedom), and z is normal enough for the threshold to
    mean what it says."""
    from mtx import load_dict

    f = FURNACE
    sc = blc.scene("furnace")
    integ = load_dict({"type": "ptracer", "max_depth": f["M"], "rr_depth": 2, "hide_emitters": hide})
    expect = f["Le"] * (1 - f["rho"] ** f["M"]) / (1 - f["rho"]) - (f["Le"] if hide else 0.0)
    from test_gpu_convergence import _blocks

    passes = np.stack([_ptracer_img(integ, sc, 40 + k, f["spp"] // 4) for k in range(4 * f["K"])])
    imgs = passes.reshape((f["K"], 4) + passes.shape[1:]).mean(1)
    x = np.stack([_blocks(i, 8) for i in imgs])
    m, var = x.mean(0), x.var(0, ddof=1)
    ring = np.minimum(np.arange(4), 3 - np.arange(4))
    cls = ring[:, None] + ring[None, :]  # 0 corner, 1 edge, 2 centre
    pooled = np.zeros_like(var)
    for c in range(3):
        pooled[cls == c] = var[cls == c].mean(0)
    z = (m - expect) / np.sqrt(pooled / f["K"] + 1e-24)
    means = passes.mean(axis=(1, 2, 3))
    zm = (means.mean() - expect) / (means.std(ddof=1) / np.sqrt(len(means)))
    print("furnace hide=%s: expect %.5f mean %.5f z_mean %.2f max|z| %.2f" % (hide, expect, means.mean(), zm,
                                                                              np.abs(z).max()))
    assert np.abs(z).max() < 5.5, float(np.abs(z).max())
    assert abs(zm) < 5.5, (float(means.mean()), expect, float(zm))


def _dict_scene(d, base_dir=None):
    from mtx.mitsuba_dict import scene_from_dict

    return scene_from_dict(d, base_dir=base_dir)


def _bedroom(face_normals=True):
    from mtx.scene import Scene

    return Scene.bedroom(width=64, height=36, scale=0.02, tex_res=64,
                         spec=blc.connectable_bedroom_spec(face_normals))


AGREE = {
    # scene builder, max_depth, block, ptracer spp, path_test spp
    "cornell": (lambda lat: _dict_scene(blc.cornell_dict(32, 32)), 5, 8, 1024, 1024),
    "lattice": (lambda lat: blc.scene("lattice", lat), 4, 4, 1024, 256),
    "sky": (lambda lat: blc.scene("sky"), 4, 8, 1024, 1024),
    "glass": (lambda lat: _dict_scene(blc.glass_dict()), 5, 8, 1024, 1024),
    "immersed": (lambda lat: _dict_scene(blc.immersed_dict()), 4, 8, 1024, 1024),
    "bumpy": (lambda lat: _dict_scene(blc.bumpy_dict(lat), lat), 4, 8, 1024, 1024),
    "bedroom": (lambda lat: _bedroom(), 4, 4, 512, 512),
}


_FUSED = {}


def _agreement(name, lat, ptracer_cls=None):
    """(max block |z|, z of the means, the two means) of ptracer against path_test on AGREE[name]."""
    from mtx import load_dict
    from test_gpu_convergence import _z

    build, M, b, spp_p, spp_f = AGREE[name]
    sc = build(lat)
    K = 16
    props = {"max_depth": M, "rr_depth": 3}
    ptracer = load_dict(dict(props, type="ptracer")) if ptracer_cls is None else ptracer_cls(props)
    fused = load_dict(dict(props, type="path_test"))
    a = np.stack([_ptracer_img(ptracer, sc, 500 + k, spp_p) for k in range(K)])
    if name not in _FUSED:  # the reference: rendered once per scene
        _FUSED[name] = np.stack([_fused_img(fused, sc, 900 + k, spp_f) for k in range(K)])
    f = _FUSED[name]
    assert np.isfinite(a).all() and np.isfinite(f).all()
    (pt, pt_mean), (pm, pm_mean) = _block_stats(a, b), _block_stats(f, b)
    z = _z(pt, pm)
    zm = (pt_mean[0] - pm_mean[0]) / np.sqrt(pt_mean[1] ** 2 + pm_mean[1] ** 2)
    print("%s: means %.5f %.5f z_mean %.2f max|z| %.2f" % (name, pt_mean[0], pm_mean[0], zm, np.abs(z).max()))
    return float(np.abs(z).max()), float(zm), float(pt_mean[0]), float(pm_mean[0])


@pytest.mark.parametrize("name", list(AGREE))
def test_ptracer_agrees_with_path_test(name, lat):
    """ptracer against the fused path_test at equal max_depth (rr_depth 3 on
    both), box filter: every block |z| < 5.5 and the image means within 5.5
    combined standard errors. cornell: rectangles and cubes, diffuse; lattice:
    18 mesh emitters (the camera sees the front of one sheet, which nothing
    lights: a pin of the directly visible mesh emitters); sky: the environment
    alone; glass: a smooth dielectric cube that every contributing path
    enters and leaves; immersed: camera and floor inside the glass, one
    interface on every contributing path, so the transmission correction does
    not cancel; bumpy: vertex normals that differ from the geometric one at
    every hit, the shading-normal correction of the adjoint BSDF; bedroom: the
    64 x 36 proxy at 2 % of its triangles (textures, both plastics, rough
    conductors), its delta, null and rough-dielectric lobes replaced
    (blocks_light_cases.connectable_bedroom_spec says why) and its meshes
    shaded with face normals. With the proxy's vertex normals the two
    estimators differ by a known term and are not compared here: the particle
    tracer's light-leak mask (Mitsuba's) removes light that path_test keeps,
    2.4 % of the image mean on these coarse meshes (DESIGN.md 3.1 has the
    figures); the correction itself is pinned on the bumpy scene, where that
    term is empty.

    K = 16 renders each. The standard errors come from the spread over the
    renders, so z is a Student t with K - 1 degrees of freedom: at K = 4 it
    passes 5.5 with probability 1.2 % per comparison, at K = 16 with 6e-5."""
    zmax, zm, mean_p, mean_f = _agreement(name, lat)
    assert mean_p > 0 and mean_f > 0
    assert zmax < 5.5, (name, zmax)
    assert abs(zm) < 5.5, (name, mean_p, mean_f, zm)


def test_adjoint_correction_is_pinned(lat):
    """The bumpy scene tells the shading-normal correction from its
    neighbours: a particle tracer with the inverse ratio, or with none, is
    many standard errors from path_test where the real one agrees."""
    import torch

    from mtx import blocks

    class Inverse(blocks.ParticleTracer):
        @staticmethod
        def _adjoint(si, wi_g, wo_local, wo_world):
            ok, corr = blocks.ParticleTracer._adjoint(si, wi_g, wo_local, wo_world)
            some = corr > 0
            return ok & some, blocks.rcp(torch.where(some, corr, torch.ones_like(corr)))

    class Uncorrected(blocks.ParticleTracer):
        @staticmethod
        def _adjoint(si, wi_g, wo_local, wo_world):
            ok, corr = blocks.ParticleTracer._adjoint(si, wi_g, wo_local, wo_world)
            return ok, torch.ones_like(corr)

    for cls in (Inverse, Uncorrected):
        zmax, _zm, _p, _f = _agreement("bumpy", lat, cls)
        assert zmax > 11.0, (cls.__name__, zmax)  # twice the threshold: not a near miss
