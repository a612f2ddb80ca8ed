"""blocks.Sensor, blocks.Film and blocks.SamplingIntegrator on the GPU: sensor
rays against the oracle's camera_ray probe, Film.put / raw against the
oracle's film (box and gaussian: tests/test_rfilter_gpu.py's restatement) on
both source paths, splits, permutations and masks against the ragged numpy
restatement (tests/blocks_film_cases.py, anchored by tests/test_blocks_film.py),
and two integrators written on the blocks, registered and rendered, against
the fused integrators' raw films. Every comparison is bit for bit."""
import blocks_film_cases as fc
import numpy as np
import pytest
from test_blocks_gpu import dev, host, same
from test_environment import with_sky
from test_mitsuba_dict import cornell_box
from test_rfilter_gpu import NAMES, REACH, TENT, _restated

pytestmark = pytest.mark.gpu

F32 = np.float32
LANES = (1, 63, 64, 65, 257, 4096)
NMAX = 4096
_POS = {}


@pytest.fixture(scope="module")
def scenes(small_scene):
    from mtx.mitsuba_dict import scene_from_dict

    d = cornell_box(32, 24)
    d["sensor"]["fov_axis"] = "y"  # the bedroom's sensor keeps the fov along x
    return {"small": small_scene, "cornell_y": scene_from_dict(d),
            "sky": scene_from_dict(with_sky(cornell_box(32, 32), [0.4, 0.5, 0.6]))}


def planes_of(film):
    return film.planes.cpu().numpy()


def put_both(blocks, sc, rfilter, L, pos, spp, **kw):
    """One put on the general path and one on the pixel-major path; returns both films."""
    g = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    p = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    assert g.put(dev(pos), dev(L), **kw) == 0
    assert p.put(dev(pos), dev(L), pixel_major_spp=spp, **kw) == 0
    return g, p


# ------------------------------------------------------------ sensor rays --
def positions(sc):
    """Film positions, once per scene: integer pixel corners, the film's edges,
    positions outside the film, and jittered ones inside."""
    key = id(sc)
    if key not in _POS:
        W, H = sc.width, sc.height
        rng = np.random.default_rng(31)
        pos = (rng.random((NMAX, 2)) * [W, H]).astype(F32)
        k = NMAX // 4
        pos[1:k:4] = np.floor(pos[1:k:4])  # corners (lane 0 stays a plain position)
        pos[2:k:4, 0] = rng.choice(F32([0, W]), len(pos[2:k:4]))  # left / right edge
        pos[3:k:4, 1] = rng.choice(F32([0, H]), len(pos[3:k:4]))  # top / bottom edge
        out = (rng.random((k, 2)) * [3 * W, 3 * H] - [W, H]).astype(F32)
        pos[k: 2 * k] = out  # a third of them inside, the rest around the film
        pos[63], pos[64] = F32([W, H]), F32([-0.5, H + 2.25])
        _POS[key] = (pos, (pos / F32([W, H])).astype(F32))
        assert _POS[key][1].dtype == F32
    return _POS[key]


@pytest.mark.parametrize("kind", ["small", "cornell_y"])
@pytest.mark.parametrize("n", LANES)
def test_sensor_rays(scenes, oracle, kind, n):
    from mtx import blocks

    sc = scenes[kind]
    pos, adj = positions(sc)
    want = oracle.probe(sc, "camera_ray", adj[:n])
    sens = blocks.Sensor(sc)
    assert (sens.width, sens.height) == (sc.width, sc.height)
    ray = sens.sample_ray(dev(pos[:n]))
    same(host(ray.o), want[:, 0:3], f"{kind} o")
    same(host(ray.d), want[:, 3:6], f"{kind} d")
    same(host(ray.maxt), want[:, 6], f"{kind} maxt")
    if n == NMAX:
        inside = (pos[:, 0] >= 0) & (pos[:, 0] < sc.width) & (pos[:, 1] >= 0) & (pos[:, 1] < sc.height)
        assert inside.any() and (~inside).any() and (pos == np.floor(pos)).all(1).any()
        assert len(np.unique(want[:, 3:6], axis=0)) > NMAX // 2
    act = (np.arange(n) % 7) != 3
    ray = sens.sample_ray(dev(pos[:n]), dev(act))
    same(host(ray.o), np.where(act[:, None], want[:, 0:3], F32(0)), "masked o")
    same(host(ray.d), np.where(act[:, None], want[:, 3:6], F32(0)), "masked d")


def test_sensor_argument_forms(scenes, oracle):
    """`sensor` as scene_with_sensor takes it: another camera of the same film size."""
    from mtx import blocks

    sc, other = scenes["sky"], scenes["sky"].with_film(32, 32)
    cam = type(sc.camera).from_buffer_copy(bytes(sc.camera))
    cam.origin[0] += 0.25
    pos, adj = positions(sc)
    want = oracle.probe(other.with_camera(cam), "camera_ray", adj[:257])
    ray = blocks.Sensor(sc, cam).sample_ray(dev(pos[:257]))
    same(host(ray.o), want[:, 0:3], "o through another camera")
    same(host(ray.d), want[:, 3:6], "d through another camera")
    back = blocks.Sensor(sc).sample_ray(dev(pos[:257]))  # the scene's own camera again
    same(host(back.o), oracle.probe(sc, "camera_ray", adj[:257])[:, 0:3], "o through the scene's camera")


# ----------------------------------------------------- put against the oracle --
@pytest.mark.parametrize("rfilter", ["tent", "box", "gaussian"])
@pytest.mark.parametrize("spp", fc.SPPS)
def test_put_equals_the_oracle_film(small_scene, oracle, spp, rfilter):
    from mtx import blocks

    sc = small_scene
    a, L, pos, _ = fc.band_samples(sc, oracle, spp)
    fid = NAMES[rfilter]
    want = oracle.film(sc.width, fc.Y0, fc.Y1, spp, L, pos) if fid == TENT else _restated(oracle, fid, sc, a, L, pos)
    g, p = put_both(blocks, sc, rfilter, L, pos, spp)
    b = REACH[fid]
    assert tuple(g.planes.shape) == (8, (2 * b + 1) ** 2, (fc.Y1 - fc.Y0) * sc.width, 4)
    same(planes_of(p), planes_of(g), "pixel-major planes vs general planes")
    for film, what in ((g, "general"), (p, "pixel-major")):
        raw = film.raw()
        assert tuple(raw.shape) == (fc.Y1 - fc.Y0 + 2 * b, sc.width + 2 * b, 4)
        same(raw.cpu().numpy(), want, f"{what} raw film, spp {spp}, {rfilter}")
    assert want[..., :3].sum() > 0 and want[..., 3].sum() > 0
    # spp_total given = the count every pixel has
    g2, p2 = put_both(blocks, sc, rfilter, L, pos, spp, spp_total=spp)
    same(planes_of(g2), planes_of(g), "general, spp_total given")
    same(planes_of(p2), planes_of(g), "pixel-major, spp_total given")
    # develop: the border cropped, rgb / w
    inner = want[b: want.shape[0] - b, b: want.shape[1] - b]
    w = inner[..., 3:4]
    img = np.where(w != 0, inner[..., :3] / np.where(w != 0, w, 1), 0).astype(F32)
    same(g.develop().cpu().numpy(), img, "develop")


# ------------------------------------------------------------------ splits --
@pytest.mark.parametrize("rfilter", ["tent", "gaussian"])
def test_splits(small_scene, oracle, rfilter):
    from mtx import blocks

    sc, spp = small_scene, 9
    _, L, pos, _ = fc.band_samples(sc, oracle, spp)
    one, _ = put_both(blocks, sc, rfilter, L, pos, spp)
    want = planes_of(one)
    px0 = fc.Y0 * sc.width
    # whole-pixel passes of 100, 1 and 283 pixels
    g = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    p = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    lo = 0
    for npx in (100, 1, 283):
        sl = slice(lo * spp, (lo + npx) * spp)
        assert g.put(dev(pos[sl]), dev(L[sl])) == 0
        assert p.put(dev(pos[sl]), dev(L[sl]), pixel_major_spp=spp, px0=px0 + lo) == 0
        lo += npx
    assert lo * spp == len(L)
    same(planes_of(g), want, "general, whole-pixel passes")
    same(planes_of(p), want, "pixel-major, whole-pixel passes")
    # sample passes 4 + 5 of spp 9
    g = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    p = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    Ls, ps = L.reshape(-1, spp, 3), pos.reshape(-1, spp, 2)
    for s0, s1 in ((0, 4), (4, 9)):
        Lp, pp = Ls[:, s0:s1].reshape(-1, 3), ps[:, s0:s1].reshape(-1, 2)
        assert g.put(dev(pp), dev(Lp), spp_total=9, sample_offset=s0) == 0
        assert p.put(dev(pp), dev(Lp), spp_total=9, sample_offset=s0, pixel_major_spp=s1 - s0) == 0
    same(planes_of(g), want, "general, sample passes")
    same(planes_of(p), want, "pixel-major, sample passes")


def test_sample_shard_equals_the_oracle_shard(small_scene, oracle):
    from mtx import blocks

    sc = small_scene
    _, L, pos, _ = fc.band_samples(sc, oracle, 4, spp_total=8, sample_offset=4)
    want = oracle.film(sc.width, fc.Y0, fc.Y1, 4, L, pos, spp_total=8, sample_offset=4)
    g, p = put_both(blocks, sc, "tent", L, pos, 4, spp_total=8, sample_offset=4)
    same(g.raw().cpu().numpy(), want, "general shard")
    same(p.raw().cpu().numpy(), want, "pixel-major shard")


# --------------------------------------------------------- order and masks --
@pytest.mark.parametrize("rfilter", ["tent", "gaussian"])
def test_permuted_lanes(small_scene, oracle, rfilter):
    """Lanes in any order: a pixel's samples rank by lane index."""
    from mtx import blocks

    sc, spp = small_scene, 9
    _, L, pos, pix = fc.band_samples(sc, oracle, spp)
    perm = np.random.default_rng(41).permutation(len(L))
    fid = NAMES[rfilter]
    ref = fc.planes_np(oracle, fid, sc.width, fc.Y0, fc.Y1, pix[perm], L[perm], pos[perm])
    film = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    assert film.put(dev(pos[perm]), dev(L[perm])) == 0
    same(planes_of(film), fc.device_layout(ref), "planes of permuted lanes")
    same(film.raw().cpu().numpy(), fc.raw_np(ref), "raw film of permuted lanes")
    # the order matters to the bits: the restatement in (pixel, sample) order differs somewhere
    assert (fc.planes_np(oracle, fid, sc.width, fc.Y0, fc.Y1, pix, L, pos) != ref).any()


@pytest.mark.parametrize("spp_total", [None, 9])
@pytest.mark.parametrize("rfilter", ["tent", "gaussian"])
def test_masks_and_dropped_samples(small_scene, oracle, rfilter, spp_total):
    from mtx import blocks

    sc, spp = small_scene, 9
    _, L, pos, pix = fc.band_samples(sc, oracle, spp)
    n = len(L)
    act = (np.arange(n) % 7) != 3
    for q in (5, 77, 300):  # pixels left with no sample at all
        act[q * spp: (q + 1) * spp] = False
    pos = pos.copy()
    bad = np.zeros(n, bool)
    pos[10::97, 1] = F32(fc.Y1) + F32(0.5)   # a row below the band
    pos[20::97, 1] = F32(fc.Y0) - F32(0.25)  # a row above it
    pos[30::97, 0] = F32(-0.5)
    pos[40::97, 0] = F32(sc.width)           # the right edge is outside
    pos[50::97, 0] = np.nan
    pos[60::97, 1] = np.inf
    for k in (10, 20, 30, 40, 50, 60):
        bad[k::97] = True
    keep = act & ~bad
    assert (bad & act).sum() > 20 and (bad & ~act).any()
    fid = NAMES[rfilter]
    ref = fc.planes_np(oracle, fid, sc.width, fc.Y0, fc.Y1, pix[keep], L[keep], pos[keep], spp_total=spp_total)
    film = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    dropped = film.put(dev(pos), dev(L), dev(act), spp_total=spp_total)
    assert dropped == int((bad & act).sum())
    same(planes_of(film), fc.device_layout(ref), "planes under masks")
    same(film.raw().cpu().numpy(), fc.raw_np(ref), "raw film under masks")
    assert not planes_of(film)[:, :, [5, 77, 300]].any()
    counts = np.bincount(pix[keep], minlength=sc.width * (fc.Y1 - fc.Y0))
    assert len(set(counts.tolist())) >= 4  # ragged: several different counts per pixel
    # the pixel-major path where it applies: masked lanes and non-finite positions, none outside its pixel
    pm = pos.copy()
    inside = np.isfinite(pm).all(1)
    restore = bad & inside
    pm[restore] = fc.band_samples(sc, oracle, spp)[2][restore]
    keep = act & inside
    ref = fc.planes_np(oracle, fid, sc.width, fc.Y0, fc.Y1, pix[keep], L[keep], pm[keep], spp_total=spp_total)
    p = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    g = blocks.Film(sc.width, fc.Y0, fc.Y1, rfilter)
    assert p.put(dev(pm), dev(L), dev(act), spp_total=spp_total, pixel_major_spp=spp) == int((~inside & act).sum())
    assert g.put(dev(pm), dev(L), dev(act), spp_total=spp_total) == int((~inside & act).sum())
    same(planes_of(p), fc.device_layout(ref), "pixel-major planes under masks")
    same(planes_of(g), planes_of(p), "general planes vs pixel-major planes under masks")


# -------------------------------------------------------------- end to end --
def _integrators():
    """bi.simple and bi.path_mis as blocks.SamplingIntegrator subclasses, registered once."""
    import blocks_integrators as bi
    from mtx import blocks, register_integrator

    def make(loop):
        class OnBlocks(blocks.SamplingIntegrator):
            def __init__(self, props=None):
                super().__init__(props)
                self.max_depth = self.props.get("max_depth", 8)
                self.rr_depth = self.props.get("rr_depth", 2)

            def sample(self, scene, sampler, ray, medium=None, active=None):
                L, valid = loop(scene, sampler, ray.o, ray.d, self.max_depth, self.rr_depth)
                return L, valid, []

        return OnBlocks

    register_integrator("blocks_simple", make(bi.simple))
    register_integrator("blocks_path_mis", make(bi.path_mis))
    return {"blocks_simple": "integrator", "blocks_path_mis": "path_test"}


# scene, rows, spp, filter, extra arguments, max_lanes (at least 3 passes, the last one ragged)
RENDERS = {
    "small_whole_tent": ("small", None, 3, "tent", {}, 3000),             # 1000 + 1000 + 304 pixels
    "small_band_gaussian": ("small", (fc.Y0, fc.Y1), 3, "gaussian", {}, 500),  # 166 + 166 + 52
    "sky_box": ("sky", None, 9, "box", {}, 4000),                          # 444 + 444 + 136
    "sky_declared_filter": ("sky", None, 9, "scene", {}, None),            # the Cornell box declares the gaussian
    "small_band_shard": ("small", (fc.Y0, fc.Y1), 4, "tent", {"spp_total": 8, "sample_offset": 4}, 700),
}


@pytest.mark.parametrize("name", ["blocks_simple", "blocks_path_mis"])
@pytest.mark.parametrize("case", sorted(RENDERS))
def test_render_film_equals_the_fused_film(scenes, case, name):
    from mtx import blocks, load_dict

    fused_name = _integrators()[name]
    kind, rows, spp, rfilter, extra, max_lanes = RENDERS[case]
    sc = scenes[kind]
    kw = dict(extra)
    if rows:
        kw["y0"], kw["y1"] = rows
    props = {"max_depth": 8, "rr_depth": 2}
    want = load_dict({"type": fused_name, **props}).render_film(sc, seed=7, spp=spp, rfilter=rfilter, **kw)
    integ = load_dict({"type": name, **props})
    assert isinstance(integ, blocks.SamplingIntegrator)
    got = integ.render_film(sc, seed=7, spp=spp, rfilter=rfilter, max_lanes=max_lanes, **kw)
    assert got.is_cuda and tuple(got.shape) == want.shape
    same(got.cpu().numpy(), want, f"{name} {case}")
    assert want[..., :3].sum() > 0
    if max_lanes:  # the passes do not show: one pass gives the same film
        n_px = ((rows[1] - rows[0]) if rows else sc.height) * sc.width
        per = max_lanes // spp
        assert -(-n_px // per) >= 3 and n_px % per
    if case == "sky_declared_filter":
        assert want.shape == (sc.height + 4, sc.width + 4, 4)
        prop = load_dict({"type": name, "rfilter": "scene", **props})  # the property instead of the argument
        same(prop.render_film(sc, seed=7, spp=spp).cpu().numpy(), want, "rfilter property")


def test_render_develops_the_film(scenes):
    from mtx import develop, load_dict

    _integrators()
    sc = scenes["small"]
    film = load_dict({"type": "integrator", "max_depth": 8, "rr_depth": 2}).render_film(sc, seed=2, spp=3)
    integ = load_dict({"type": "blocks_simple", "max_depth": 8, "rr_depth": 2})
    img = integ.render(sc, seed=2, spp=3)
    assert img.is_cuda and tuple(img.shape) == (sc.height, sc.width, 3)
    same(img.cpu().numpy(), develop(film, 1), "render() vs develop of the fused film")
    same(integ.render(sc, seed=2, spp=3, develop=False).cpu().numpy(), film, "render(develop=False)")


# ---------------------------------------------------------------- refusals --
def test_refusals(scenes, oracle):
    import torch
    from mtx import MtxError, blocks, load_dict
    from mtx.mitsuba_dict import scene_from_dict

    sc, spp = scenes["small"], 3
    _, L, pos, _ = fc.band_samples(sc, oracle, spp)
    n = len(L)
    P, Lt = dev(pos), dev(L)
    film = blocks.Film(sc.width, fc.Y0, fc.Y1, "tent")
    assert film.put(P, Lt, pixel_major_spp=spp) == 0
    before = planes_of(film).copy()
    assert before.any()

    def unchanged_and_usable():
        same(planes_of(film), before, "planes after a refused put")
        again = blocks.Film(sc.width, fc.Y0, fc.Y1, "tent")
        assert again.put(P, Lt) == 0
        same(planes_of(again), before, "context still usable")

    with pytest.raises(MtxError, match=r"put: pos.*host"):
        film.put(P.cpu(), Lt)
    with pytest.raises(MtxError, match=r"put: L.*host"):
        film.put(P, Lt.cpu())
    with pytest.raises(MtxError, match=r"put: pos.*float64"):
        film.put(P.double(), Lt)
    with pytest.raises(MtxError, match=r"put: L.*shape"):
        film.put(P, Lt[:2].contiguous())
    with pytest.raises(MtxError, match=rf"put: L.*N = {n}"):
        film.put(P, Lt[:, :-1].contiguous())
    with pytest.raises(MtxError, match=r"put: active"):
        film.put(P, Lt, torch.ones(n, device="cuda"))
    with pytest.raises(MtxError, match=r"put: pos.*contiguous"):
        film.put(dev(np.tile(pos, (1, 2)))[::2], Lt)
    sens = blocks.Sensor(sc)
    with pytest.raises(MtxError, match=r"sample_ray: pos.*host"):
        sens.sample_ray(P.cpu())
    with pytest.raises(MtxError, match=r"sample_ray: pos.*shape"):
        sens.sample_ray(Lt)
    with pytest.raises(MtxError, match=r"sample_ray: active.*N = "):
        sens.sample_ray(P, torch.ones(n - 1, dtype=torch.bool, device="cuda"))
    unchanged_and_usable()
    # a false pixel-major claim: 5 lanes in another pixel, one of them only by its row
    wrong = pos.copy()
    for k in (0, 100, 101, 700):
        wrong[k, 0] += F32(1)
    wrong[n - 1, 1] -= F32(1)
    with pytest.raises(MtxError, match=r"\b5 lanes whose position lies outside the pixel"):
        film.put(dev(wrong), Lt, pixel_major_spp=spp)
    unchanged_and_usable()
    with pytest.raises(MtxError, match=r"pixel-major layout"):  # not a multiple of the samples per pixel
        film.put(dev(pos[:-1]), dev(L[:-1]), pixel_major_spp=spp)
    with pytest.raises(MtxError, match=r"pixel-major layout"):  # pixels past the band's end
        film.put(P, Lt, pixel_major_spp=spp, px0=fc.Y0 * sc.width + 1)
    unchanged_and_usable()
    assert film.put(dev(pos[:0]), dev(L[:0])) == 0  # N = 0: nothing
    # the scene's declared filter must be one of the three
    with pytest.raises(MtxError, match=r"unknown reconstruction filter"):
        blocks.Film(8, 0, 4, "mitchell")
    d = cornell_box(16, 16)
    d["sensor"]["film"]["rfilter"] = {"type": "mitchell"}
    _integrators()
    with pytest.raises(MtxError, match=r"mitchell"):
        load_dict({"type": "blocks_simple"}).render_film(scene_from_dict(d), spp=1, rfilter="scene")
    with pytest.raises(MtxError, match=r"mitchell"):
        load_dict({"type": "blocks_simple", "rfilter": "scene"}).render(scene_from_dict(d), spp=1)
