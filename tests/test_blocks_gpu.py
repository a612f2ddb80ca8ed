"""The device-tensor building blocks (mtx.blocks) on the GPU, each block
bit for bit against the item-by-item probe the oracle has for the same
per-lane function, then composed: two integrators written in Python on the
blocks (tests/blocks_integrators.py) against the oracle's loops and the fused
sample().

Lane counts: one lane, both sides of the wave edge, past a block edge, a few
blocks. The references are computed once for 4096 items per scene; a test at
n lanes feeds the first n items and compares with the first n rows."""
import mesh_emitter_cases as mc
import numpy as np
import pytest
from test_environment import with_sky
from test_mesh_emitters_gpu import _rays
from test_mitsuba_dict import cornell_box

pytestmark = pytest.mark.gpu

LANES = (1, 63, 64, 65, 257, 4096)
NMAX = 4096
SCENES = ("small", "full", "sky")
_REF = {}


@pytest.fixture(scope="module")
def scenes(small_scene, tmp_path_factory):
    from mtx.mitsuba_dict import scene_from_dict

    d = str(tmp_path_factory.mktemp("blocks_gpu"))
    mc.write_meshes(d)
    return {"small": small_scene, "full": mc.build(d, "full", 32, 18),
            "sky": scene_from_dict(with_sky(cornell_box(32, 32), [0.4, 0.5, 0.6]))}


def dev(a):
    """(N, C) or (N,) numpy -> the blocks' (C, N) / (N,) CUDA tensor."""
    import torch

    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda()


def host(t):
    a = t.cpu().numpy()
    return np.ascontiguousarray(a.T)


def same(got, want, what=""):
    """Bit-for-bit equality of float32 / int32 arrays (a NaN equals a NaN)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype.kind == "f":
        gb, wb = got.view(np.uint32), np.asarray(want, np.float32).view(np.uint32)
        bad = (gb != wb) & ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got.astype(np.int64) != np.asarray(want).astype(np.int64)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def rays_of(sc):
    """The _rays recipe, with every 16th ray (from the 16th on) leaving the scene: sure misses."""
    o, d = _rays(sc, NMAX, seed=3)
    o[15::16] = np.float32([50.0, 60.0, 70.0])
    d[15::16] = np.float32([0.6, 0.0, 0.8])
    return o, d


def active_of(n):
    return (np.arange(n) % 7) != 3


def ref(scenes, oracle, kind):
    """Rays and the oracle's hit records / interactions of a scene, once."""
    if kind in _REF:
        return _REF[kind]
    sc = scenes[kind]
    o, d = rays_of(sc)
    n = len(o)
    big = np.float32(3.40282346638528859812e+38)
    r8 = np.zeros((n, 8), np.float32)
    r8[:, :3], r8[:, 3], r8[:, 4:7] = o, big, d
    hits, _ = oracle.trace(sc, r8)
    hits = hits.reshape(n, 4)
    t, prim = hits[:, 0].view(np.float32), hits[:, 1]
    bu, bv = hits[:, 2].view(np.float32), hits[:, 3].view(np.float32)
    hit = prim != 0xffffffff
    # the hit triangle's vertices, normals, uvs and shape fields, gathered from the scene arrays
    shp = np.frombuffer(bytes(sc.shapes), np.uint32).reshape(-1, 4)
    pr = np.where(hit, prim, 0).astype(np.int64)
    vi = np.asarray(sc.tri_vidx, np.uint32).reshape(-1, 3)[pr].astype(np.int64)
    sh = shp[np.asarray(sc.tri_shape)[pr]]
    vpos = np.asarray(sc.vpos, np.float32).reshape(-1, 3)
    vn = np.asarray(sc.vnormal, np.float32).reshape(-1, 3)
    vuv = np.asarray(sc.vuv, np.float32).reshape(-1, 2)
    use_n = ((sh[:, 2] & 1) == 0) & (len(vn) > 0)
    use_uv = ((sh[:, 2] & 2) != 0) & (len(vuv) > 0)
    item = np.zeros((n, 40), np.float32)
    item[:, 0], item[:, 1], item[:, 2], item[:, 3:6] = t, bu, bv, d
    item[:, 6:15] = vpos[vi].reshape(n, 9)
    item[:, 15] = use_n
    if len(vn):
        item[:, 16:25] = np.where(use_n[:, None], vn[vi].reshape(n, 9), 0)
    item[:, 25] = use_uv
    if len(vuv):
        item[:, 26:32] = np.where(use_uv[:, None], vuv[vi].reshape(n, 6), 0)
    q = oracle.si_probe(item)
    si = {"p": q[:, 0:3], "n": q[:, 3:6], "sh_n": q[:, 12:15], "uv": q[:, 15:17], "wi": q[:, 17:20]}
    miss = {"p": np.zeros(3), "n": [0, 0, 1], "sh_n": [0, 0, 1], "uv": np.zeros(2)}
    for k, v in miss.items():
        si[k] = np.where(hit[:, None], si[k], np.float32(v)).astype(np.float32)
    si["wi"] = np.where(hit[:, None], si["wi"], -d).astype(np.float32)
    env = len(sc.emitters) if sc.env_radiance is not None else -1
    si["t"] = t
    si["prim"] = prim.view(np.int32)
    si["material"] = np.where(hit, sh[:, 0].view(np.int32), -1).astype(np.int32)
    si["emitter"] = np.where(hit, sh[:, 1].view(np.int32), env).astype(np.int32)
    si["bary"] = np.stack([bu, bv], 1)
    _REF[kind] = {"o": o, "d": d, "hit": hit, "si": si, "r8": r8}
    return _REF[kind]


def si_on_device(r, n):
    """A blocks.SurfaceInteraction holding the first n reference rows."""
    from mtx import blocks

    si = blocks.SurfaceInteraction(dev(r["o"][:n]).device, n)
    for k, v in r["si"].items():
        getattr(si, k).copy_(dev(v[:n]))
    return si._done()


# ------------------------------------------------------------- 1. sampler --
@pytest.mark.parametrize("skip", [0, 2])
@pytest.mark.parametrize("n", LANES)
def test_sampler(oracle, n, skip):
    from mtx import blocks

    lanes = np.arange(n, dtype=np.uint32) * 5 + 2
    want = oracle.rng_stream(11, 2, 5 * (n - 1) + 1, 7 + skip)[::5, skip:]
    for order in ((1, 1, 2, 2, 1), (2, 1, 2, 1, 1)):  # 7 draws: 1d 1d 2d ..., 2d 1d 2d 1d ...
        s = blocks.Sampler(11, lanes, skip=skip)
        got = []
        for dims in order:
            x = s.next_1d() if dims == 1 else s.next_2d()
            assert tuple(x.shape) == ((n,) if dims == 1 else (2, n))
            got.append(host(x).reshape(n, dims))
        same(np.concatenate(got, 1), want, f"sampler order {order}")


# ------------------------------------------- 2. ray_intersect / ray_test --
@pytest.mark.parametrize("kind", SCENES)
@pytest.mark.parametrize("n", LANES)
def test_ray_intersect(scenes, oracle, kind, n):
    from mtx import blocks

    r = ref(scenes, oracle, kind)
    scn = blocks.Scene(scenes[kind])
    assert scn.has_environment == (kind == "sky")
    o, d = dev(r["o"][:n]), dev(r["d"][:n])
    si = scn.ray_intersect(o, d)
    for k, v in r["si"].items():  # t, prim, barycentrics: oracle.trace; p .. wi: oracle.si_probe; the shape table
        same(host(getattr(si, k)), v[:n], f"{kind} si.{k}")
    same(host(si.valid), r["hit"][:n], "valid")
    if n == NMAX:
        miss = ~r["hit"]
        assert miss.any() and r["hit"].any()
        assert (r["si"]["emitter"][miss] == (len(scenes[kind].emitters) if kind == "sky" else -1)).all()
    # masked-off lanes: invalid, emitter -1, whatever the ray; the others unchanged
    act = active_of(n)
    sm = scn.ray_intersect(o, d, None, dev(act))
    off = ~act
    for k, v in r["si"].items():
        same(host(getattr(sm, k))[act], v[:n][act], f"{kind} masked si.{k}")
    assert not host(sm.valid)[off].any()
    assert (host(sm.emitter)[off] == -1).all() and (host(sm.material)[off] == -1).all()
    assert np.isinf(host(sm.t)[off]).all() and (host(sm.prim)[off] == -1).all()
    same(host(sm.wi)[off], -r["d"][:n][off], "masked wi")
    # the same interactions from hit records the caller holds
    s2 = scn.interact(d, si.t, si.prim, si.bary[0].contiguous(), si.bary[1].contiguous())
    for k, v in r["si"].items():
        same(host(getattr(s2, k)), v[:n], f"{kind} interact si.{k}")
    # a finite maxt and the any-hit tree
    r8 = r["r8"][:n].copy()
    r8[:, 3] = np.float32(1.5)
    hits, _ = oracle.trace(scenes[kind], r8)
    hits = hits.reshape(n, 4)
    s3 = scn.ray_intersect(o, d, dev(r8[:, 3]))
    same(host(s3.t), hits[:, 0].view(np.float32), "t under maxt")
    same(host(s3.prim), hits[:, 1].view(np.int32), "prim under maxt")
    occ, _ = oracle.trace(scenes[kind], r8, any_hit=True)
    same(host(scn.ray_test(o, d, dev(r8[:, 3]))), occ.astype(bool), "ray_test")
    got = host(scn.ray_test(o, d, dev(r8[:, 3]), dev(act)))
    same(got, occ.astype(bool) & act, "masked ray_test")


# --------------------------------------------------------------- 3. spawn --
@pytest.mark.parametrize("kind", SCENES)
@pytest.mark.parametrize("n", LANES)
def test_spawn(scenes, oracle, kind, n):
    r = ref(scenes, oracle, kind)
    si = si_on_device(r, n)
    rng = np.random.default_rng(5)
    p, nrm = r["si"]["p"][:n], r["si"]["n"][:n]
    v = rng.normal(size=(n, 3)).astype(np.float32)
    o, d, maxt = si.spawn_ray(dev(v))
    want = oracle.probe(scenes[kind], "spawn_ray", np.concatenate([p, nrm, v], 1))
    same(host(o), want[:, 0:3], "spawn_ray o")
    same(host(d), want[:, 3:6], "spawn_ray d")
    same(host(maxt), want[:, 6], "spawn_ray maxt")
    tgt = (p + rng.normal(size=(n, 3)) * 2).astype(np.float32)
    far = np.arange(n) % 2 == 0  # targets on the far side of the normal
    tgt[far] = (p - nrm * rng.uniform(0.1, 2.0, (n, 1)) + rng.normal(size=(n, 3)) * 0.05).astype(np.float32)[far]
    o, d, maxt = si.spawn_ray_to(dev(tgt))
    want = oracle.probe(scenes[kind], "spawn_ray_to", np.concatenate([p, nrm, tgt], 1))
    same(host(o), want[:, 0:3], "spawn_ray_to o")
    same(host(d), want[:, 3:6], "spawn_ray_to d")
    same(host(maxt), want[:, 6], "spawn_ray_to maxt")


# ---------------------------------------------------- 4. emitter sampling --
@pytest.mark.parametrize("kind", SCENES)
@pytest.mark.parametrize("n", LANES)
def test_sample_emitter(scenes, oracle, kind, n):
    from mtx import blocks

    sc = scenes[kind]
    r = ref(scenes, oracle, kind)
    scn = blocks.Scene(sc)
    si = si_on_device(r, n)
    u = np.random.default_rng(9).random((n, 2)).astype(np.float32)
    p, nrm = r["si"]["p"][:n], r["si"]["n"][:n]
    want = oracle.probe(sc, "sample_emitter", np.concatenate([p, u], 1))

    def check_ds(ds, rows, what):
        same(host(ds.p)[rows], want[rows, 3:6], what + " ds.p")
        same(host(ds.n)[rows], want[rows, 6:9], what + " ds.n")
        same(host(ds.d)[rows], want[rows, 9:12], what + " ds.d")
        same(host(ds.dist)[rows], want[rows, 12], what + " ds.dist")
        same(host(ds.pdf)[rows], want[rows, 13], what + " ds.pdf")
        same(host(ds.emitter)[rows], want[rows, 14].astype(np.int32), what + " ds.emitter")

    every = np.ones(n, bool)
    ds, w = scn.sample_emitter_direction(si, dev(u), test_visibility=False)
    same(host(w), want[:, 0:3], "weight")
    check_ds(ds, every, "unoccluded")
    if n == NMAX:  # every kind of emitter of the scene is picked
        assert set(want[:, 14].astype(int)) == set(range(len(sc.emitters) + (kind == "sky")))
    # with visibility: the oracle's weight, zeroed where its shadow ray is occluded
    sr = oracle.probe(sc, "spawn_ray_to", np.concatenate([p, nrm, want[:, 3:6]], 1))
    r8 = np.zeros((n, 8), np.float32)
    r8[:, :3], r8[:, 3], r8[:, 4:7] = sr[:, 0:3], sr[:, 6], sr[:, 3:6]
    occ = oracle.trace(sc, r8, any_hit=True)[0].astype(bool)
    wv = np.where(occ[:, None], np.float32(0), want[:, 0:3])
    ds, w = scn.sample_emitter_direction(si, dev(u))
    same(host(w), wv, "visible weight")
    check_ds(ds, every, "visible")
    if n == NMAX:
        lit = (want[:, 0:3] != 0).any(1)
        assert (occ & lit).any() and (~occ & lit).any()
    act = active_of(n)
    ds, w = scn.sample_emitter_direction(si, dev(u), True, dev(act))
    same(host(w), np.where(act[:, None], wv, np.float32(0)), "masked weight")
    check_ds(ds, act, "masked")
    assert (host(ds.pdf)[~act] == 0).all() and (host(ds.d)[~act] == 0).all() and (host(ds.emitter)[~act] == -1).all()


# ------------------------------------------------------------ 5. pdf / eval --
@pytest.mark.parametrize("kind", SCENES)
@pytest.mark.parametrize("n", LANES)
def test_emitter_pdf_eval(scenes, oracle, kind, n):
    from mtx import blocks

    sc = scenes[kind]
    scn = blocks.Scene(sc)
    count = len(sc.emitters) + (kind == "sky")
    rng = np.random.default_rng(13)
    em = ((np.arange(n) + 1) % (count + 1) - 1).astype(np.int32)  # every index, the environment's and -1

    def unit(k):
        v = rng.normal(size=(k, 3))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    d, nrm, wi = unit(n), unit(n), unit(n)  # d on both sides of n, wi in both hemispheres
    dist = rng.uniform(0.5, 3.0, n).astype(np.float32)
    want = oracle.probe(sc, "pdf_emitter", np.concatenate([em[:, None].astype(np.float32), d, dist[:, None], nrm, wi], 1))
    e = dev(em)
    same(host(scn.pdf_emitter(e, dev(d), dev(dist), dev(nrm))), want[:, 0], "pdf")
    si = blocks.SurfaceInteraction(e.device, n)
    si.emitter.copy_(e)
    si.wi.copy_(dev(wi))
    same(host(scn.emitter_eval(si)), want[:, 1:4], "eval")
    if n == NMAX:
        dn = (d * nrm).sum(1)
        assert (dn > 0).any() and (dn < 0).any() and (want[:, 0] > 0).any() and (want[:, 1:4] > 0).any()
    act = active_of(n)
    same(host(scn.emitter_eval(si, dev(act))), np.where(act[:, None], want[:, 1:4], np.float32(0)), "masked eval")


def test_pdf_emitter_direction(scenes, oracle):
    """The facade's DirectionSample of a hit (ds.d, ds.dist from the exact ops; the
    environment branch for a miss) against the probe fed with the same numbers."""
    from mtx import blocks

    kind, n = "sky", NMAX
    sc, r = scenes[kind], ref(scenes, oracle, kind)
    scn = blocks.Scene(sc)
    si = si_on_device(r, n)
    prev = np.random.default_rng(2).uniform(-1, 1, (n, 3)).astype(np.float32)
    got = host(scn.pdf_emitter_direction(dev(prev), si))
    dist = host(blocks.norm(si.p - dev(prev)))
    dd = np.where(r["hit"][:, None], host(blocks.div(si.p - dev(prev), dev(dist))), -host(si.to_world(si.wi)))
    em = r["si"]["emitter"].astype(np.float32)
    want = oracle.probe(sc, "pdf_emitter", np.concatenate([em[:, None], dd, dist[:, None], r["si"]["sh_n"]], 1))
    same(got, want[:, 0], "pdf_emitter_direction")
    assert (~r["hit"]).any() and (got[~r["hit"]] > 0).all()
    # a miss sees the environment along the ray: -to_world(wi) is the ray direction
    np.testing.assert_allclose(dd[~r["hit"]], r["d"][~r["hit"]], atol=2e-6)


# ---------------------------------------------------------------- 6. BSDF --
def _flags(m):
    f = {1: 0x02, 2: 0x08 | 0x02, 3: 0x20, 4: 0x08, 5: 0x20 | 0x40, 6: 0x08 | 0x10}.get(int(m.type), 0)
    return f | (0x01 if m.flags & 2 else 0)


@pytest.mark.parametrize("n", LANES)
def test_bsdf(small_scene, oracle, n):
    """One call whose lanes cycle through all materials (and -1): a wave holds
    every BSDF type, both distributions, twosided and mask."""
    from mtx import blocks

    sc = small_scene
    scn = blocks.Scene(sc)
    nm = len(sc.materials)
    assert {int(m.type) for m in sc.materials} == {1, 2, 3, 4, 5, 6}
    assert {bool(m.flags & 4) for m in sc.materials if m.type in (2, 4, 6)} == {False, True}
    assert any(m.flags & 1 for m in sc.materials) and any(m.flags & 2 for m in sc.materials)
    rng = np.random.default_rng(17)
    mat = ((np.arange(n) + 1) % (nm + 1) - 1).astype(np.int32)

    def unit(k):
        v = rng.normal(size=(k, 3))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    wi, wo = unit(n), unit(n)
    uv, u = rng.random((n, 2)).astype(np.float32), rng.random((n, 3)).astype(np.float32)
    want = np.zeros((n, 16), np.float32)
    flags = np.zeros(n, np.int32)
    for m in range(nm):
        idx = np.nonzero(mat == m)[0]
        if len(idx):
            want[idx] = oracle.bsdf_probe(sc, m, wi[idx], wo[idx], uv[idx], u[idx])[0]
            flags[idx] = _flags(sc.materials[m])
    si = blocks.SurfaceInteraction(dev(mat).device, n)
    si.material.copy_(dev(mat))
    si.uv.copy_(dev(uv))
    si.wi.copy_(dev(wi))

    def check(out, rows, what):
        val, pdf, bs, w = out
        same(host(val)[rows], want[rows, 0:3], what + " value")
        same(host(pdf)[rows], want[rows, 3], what + " pdf")
        same(host(bs.wo)[rows], want[rows, 4:7], what + " sample wo")
        same(host(bs.pdf)[rows], want[rows, 7], what + " sample pdf")
        same(host(bs.eta)[rows], want[rows, 8], what + " sample eta")
        same(host(bs.sampled_type)[rows], want[rows, 9].view(np.int32), what + " sample type")
        same(host(w)[rows], want[rows, 10:13], what + " weight")

    args = (dev(wo), dev(u[:, 0]), dev(u[:, 1:3]))
    check(scn.bsdf_eval_pdf_sample(si, *args), np.ones(n, bool), "bsdf")
    same(host(scn.bsdf_flags(si)), flags, "flags")
    if n == NMAX:
        assert (wi[:, 2] > 0).any() and (wi[:, 2] < 0).any()
        assert (want[mat >= 0][:, 0:3] != 0).any() and not want[mat < 0].any()
    act = active_of(n)
    out = scn.bsdf_eval_pdf_sample(si, *args, dev(act))
    check(out, act, "masked bsdf")
    for t in (out[0], out[1], out[2].wo, out[2].pdf, out[2].eta, out[2].sampled_type, out[3]):
        assert not host(t)[~act].any()


# ---------------------------------------------------------- 7. exact math --
def _f64(x):
    return np.asarray(x, np.float64)


def _f32(x):
    return _f64(x).astype(np.float32)


def _fma64(a, b, c):
    """fmaf through float64: exact when a * b + c fits 53 bits (the inputs below), then one rounding."""
    return _f32(_f64(a) * _f64(b) + _f64(c))


def _dot64(a, b):
    return _fma64(a[:, 2], b[:, 2], _fma64(a[:, 1], b[:, 1], _f32(_f64(a[:, 0]) * _f64(b[:, 0]))))


@pytest.mark.parametrize("n", LANES)
def test_math_float64(n):
    """No probe reaches these ops alone: numpy float64 rounded once. Inputs are
    full 24-bit floats in [1, 2): a product is exact in double (48 bits), and a
    product plus a float below 8 fits 53 bits, so every fmaf is exact before
    its single rounding. Division and square root through double are correctly
    rounded for float32 (53 >= 2 * 24 + 2: double rounding is innocuous)."""
    import torch
    from mtx import blocks

    rng = np.random.default_rng(23)
    a, b, c = (rng.uniform(1, 2, (n, 3)).astype(np.float32) for _ in range(3))
    A, B, Cc = dev(a), dev(b), dev(c)
    got = host(blocks.fma(A, B, Cc))
    same(got, _fma64(a, b, c), "fma")
    same(host(blocks.fma(A, B[0].contiguous(), Cc)), _fma64(a, b[:, :1], c), "fma, (N,) against (3, N)")
    if n >= 63:  # the op does what a * b + c does not
        assert (got != host(A * B + Cc)).any()
    same(host(blocks.div(A, B)), _f32(_f64(a) / _f64(b)), "div")
    same(host(blocks.rcp(A)), _f32(1.0 / _f64(a)), "rcp")
    same(host(blocks.sqrt(A)), _f32(np.sqrt(_f64(a))), "sqrt")
    same(host(blocks.dot(A, B)), _dot64(a, b), "dot")
    sq = _dot64(a, a)
    same(host(blocks.norm(A)), _f32(np.sqrt(_f64(sq))), "norm")
    inv = _f32(1.0 / _f64(_f32(np.sqrt(_f64(sq)))))
    same(host(blocks.normalize(A)), _f32(_f64(a) * _f64(inv)[:, None]), "normalize")
    pa, pb = a[:, 0].copy(), b[:, 0].copy()
    pa[::5] = 0  # pdf_a = 0: variant b selects 0; with pb = 0 too variant a divides 0 by 0
    pb[::10] = 0
    a2, b2 = _f32(_f64(pa) ** 2), _f32(_f64(pb) ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        wb = np.where(pa > 0, _f32(_f64(a2) / _f64(_fma64(pb, pb, a2))), np.float32(0))
        wa = _f32(_f64(a2) / _f64(_f32(_f64(a2) + _f64(b2))))
    wa = np.where(np.isfinite(wa), wa, np.float32(0))
    same(host(blocks.mis_weight(dev(pa), dev(pb), "b")), wb, "mis_weight b")
    same(host(blocks.mis_weight(dev(pa), dev(pb), "a")), wa, "mis_weight a")
    # to_world: dyadic inputs with sign(n.z) + n.z a power of two, so frame_from_normal
    # and the transform are exact in float32 and float64 alike (the formula's structure)
    nz = rng.choice(np.float32([1, 3, 7, -1, -3, -7]), n)
    nn = np.stack([rng.integers(-8, 9, n) / 8, rng.integers(-8, 9, n) / 8, nz], 1).astype(np.float32)
    v = (rng.integers(-16, 17, (n, 3)) / 4).astype(np.float32)
    x, y, z = (nn[:, k].astype(np.float64) for k in range(3))
    sg = np.where(np.signbit(z), -1.0, 1.0)
    q = -1.0 / (sg + z)
    bb = x * y * q
    s = np.stack([np.copysign(1, z) * x * x * q + 1.0, np.copysign(1, z) * bb, -np.copysign(1, z) * x], 1)
    t = np.stack([bb, y * y * q + sg, -y], 1)
    wv = nn.astype(np.float64) * v[:, 2:3] + t * v[:, 1:2] + s * v[:, 0:1]
    np.testing.assert_array_equal(host(blocks.to_world(dev(nn), dev(v))), wv.astype(np.float32))
    wl = np.stack([(v * s).sum(1), (v * t).sum(1), (v * nn).sum(1)], 1)
    np.testing.assert_array_equal(host(blocks.to_local(dev(nn), dev(v))), wl.astype(np.float32))
    assert torch.equal(blocks.mis_weight(dev(pa), dev(pb)), blocks.mis_weight(dev(pa), dev(pb), "b"))


@pytest.mark.parametrize("kind", SCENES)
def test_math_to_local_through_si_probe(scenes, oracle, kind):
    """to_local reached through the oracle: si_probe's wi is to_local(frame(sh_n), -ray_d)."""
    from mtx import blocks

    r = ref(scenes, oracle, kind)
    h = r["hit"]
    got = host(blocks.to_local(dev(r["si"]["sh_n"]), dev(-r["d"])))
    same(got[h], r["si"]["wi"][h], "to_local")
    back = host(blocks.to_world(dev(r["si"]["sh_n"]), dev(got)))  # an orthonormal frame: back to -d up to rounding
    np.testing.assert_allclose(back[h], -r["d"][h], atol=2e-6)


# ---------------------------------------------------------- 8. end to end --
@pytest.mark.parametrize("kind", SCENES)
@pytest.mark.parametrize("name", ["integrator", "path_test"])
@pytest.mark.parametrize("n", [NMAX, 65])
def test_integrators_on_blocks(scenes, oracle, kind, name, n):
    """Frames, spawn offsets, draw order, masks and the MIS arithmetic in
    composition: the loop written on the blocks equals the oracle's and the
    fused kernel's, bit for bit."""
    import blocks_integrators as bi
    from mtx import IndependentSampler, blocks, load_dict

    sc = scenes[kind]
    r = ref(scenes, oracle, kind)
    o, d = r["o"][:n], r["d"][:n]
    lanes = np.arange(n, dtype=np.uint32) * 5 + 2
    integ = load_dict({"type": name, "max_depth": 8, "rr_depth": 2})
    Lc, vc = oracle.sample_rays(sc, integ.render_args(sc, 7, 1), np.concatenate([o, d], 1), lanes, 2)
    loop = bi.simple if name == "integrator" else bi.path_mis
    L, valid = loop(blocks.Scene(sc), blocks.Sampler(7, lanes, skip=2), dev(o), dev(d), 8, 2)
    same(host(valid), vc.astype(bool), "valid vs oracle")
    same(host(L), Lc, "L vs oracle")
    Lf, vf, _ = integ.sample(sc, IndependentSampler(7, lanes, skip=2), (o, d))
    same(host(valid), np.asarray(vf, bool), "valid vs sample()")
    same(host(L), Lf, "L vs sample()")
    if n == NMAX:
        assert (Lc > 0).any() and np.isfinite(Lc).all()


# ----------------------------------------------------------- 9. refusals --
def test_refusals(scenes, oracle):
    import torch
    from mtx import MtxError, blocks

    sc = scenes["small"]
    r = ref(scenes, oracle, "small")
    scn = blocks.Scene(sc)
    n = 65
    o, d = dev(r["o"][:n]), dev(r["d"][:n])

    def usable():
        same(host(scn.ray_intersect(o, d).prim), r["si"]["prim"][:n], "context still usable")

    with pytest.raises(MtxError, match=r"ray_intersect: o.*host"):
        scn.ray_intersect(o.cpu(), d)
    with pytest.raises(MtxError, match=r"ray_intersect: d.*contiguous"):
        scn.ray_intersect(o, dev(np.tile(r["d"][:n], (1, 2)))[::2])
    with pytest.raises(MtxError, match=r"ray_intersect: o.*float64"):
        scn.ray_intersect(o.double(), d)
    with pytest.raises(MtxError, match=r"ray_intersect: d.*N = 65"):
        scn.ray_intersect(o, dev(r["d"][:64]))
    with pytest.raises(MtxError, match=r"ray_intersect: active"):
        scn.ray_intersect(o, d, None, torch.ones(n, device="cuda"))
    with pytest.raises(MtxError, match=r"fma: argument b.*contiguous"):
        blocks.fma(o, d.T.contiguous().T, o)
    with pytest.raises(MtxError, match=r"dot: argument b.*host"):
        blocks.dot(o, d.cpu())
    with pytest.raises(MtxError, match=r"lanes.*int64"):
        blocks.Sampler(1, torch.arange(4, device="cuda"))
    usable()
    # N = 0: empties, no launch
    e3 = torch.empty((3, 0), device="cuda")
    si = scn.ray_intersect(e3, e3)
    assert tuple(si.p.shape) == (3, 0) and tuple(si.valid.shape) == (0,)
    assert tuple(scn.ray_test(e3, e3, torch.empty(0, device="cuda")).shape) == (0,)
    assert tuple(blocks.fma(e3, e3, e3).shape) == (3, 0)
    assert tuple(blocks.Sampler(1, np.zeros(0, np.uint32)).next_2d().shape) == (2, 0)
    ds, w = scn.sample_emitter_direction(si, torch.empty((2, 0), device="cuda"))
    assert tuple(w.shape) == (3, 0) and tuple(ds.pdf.shape) == (0,)
    assert tuple(scn.bsdf_flags(si).shape) == (0,)
    # the first index past each table: counted on the device, handled as invalid, reported
    si = si_on_device(r, n)
    zero3 = torch.zeros((3, n), device="cuda")
    u1, u2 = torch.rand(n, device="cuda"), torch.rand((2, n), device="cuda")
    si.material[3] = len(sc.materials)
    si.material[40] = len(sc.materials)
    with pytest.raises(MtxError, match=r"2 lanes with a material index"):
        scn.bsdf_eval_pdf_sample(si, zero3, u1, u2)
    with pytest.raises(MtxError, match=r"2 lanes with a material index"):
        scn.bsdf_flags(si)
    usable()
    si.emitter[7] = len(sc.emitters)  # no environment: emitter_count = the area emitters
    with pytest.raises(MtxError, match=r"1 lanes with an emitter index"):
        scn.emitter_eval(si)
    with pytest.raises(MtxError, match=r"1 lanes with an emitter index"):
        scn.pdf_emitter(si.emitter, zero3, u1, zero3)
    usable()
    prim = si.prim.clone()
    prim[5] = sc.n_tris
    with pytest.raises(MtxError, match=r"1 lanes with a prim"):
        scn.interact(d, si.t, prim, u1, u1)
    usable()
    sky = blocks.Scene(scenes["sky"])
    e = torch.full((n,), len(scenes["sky"].emitters) + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(MtxError, match=rf"{n} lanes with an emitter index"):
        sky.emitter_eval(si_with_emitter(e, n))
    e.fill_(len(scenes["sky"].emitters))  # the environment's own index is in range
    assert (host(sky.emitter_eval(si_with_emitter(e, n))) == np.float32([0.4, 0.5, 0.6])).all()


def si_with_emitter(e, n):
    from mtx import blocks

    si = blocks.SurfaceInteraction(e.device, n)
    si.emitter.copy_(e)
    si.wi.zero_()
    return si
