"""Film renders without a stored raygen, bit for bit against the CPU oracle.

mtx_render's chunks of path_test, mypath, nrc and integrator launch no
k_raygen_camera (ChunkParams::cam0, wavefront.h): the bounce-0 closest hit
(k_trace_camera), the bounce-0 shade (k_shade_cam) and the film source
kernels each derive the camera sample of a path from its index, the chunk's
parameters and the camera. The cases are what the derivation can get wrong:
the path index of a chunk that does not start at pixel 0 or ends short, the
sampler lane of a sample shard and a row band, the second wavefront's
buffers, a camera that changed, the initial flags under an environment, a
scene whose emitter takes a large share of the hits at every depth (the
emission MIS against the previous vertex), and the integrators that keep the
stored raygen.
"""
import numpy as np
import pytest
from test_environment import furnace
from test_mitsuba_dict import T, cornell_box

pytestmark = pytest.mark.gpu

FILM = ["path_test", "mypath", "nrc", "integrator"]


def _integ(name, **kw):
    from mtx import load_dict

    if name == "nrc":
        kw.pop("max_depth", None)
    return load_dict({"type": name, **kw})


@pytest.mark.parametrize("name", FILM)
def test_film_parity_odd_chunks(small_scene, oracle, name):
    """spp 3, chunks of 333 pixels = 999 paths: every chunk but the first has
    px0 != 0, no boundary is a multiple of 64 paths, the seventh chunk is
    short (306 pixels)."""
    integ = _integ(name, max_depth=5)
    film = integ.render_film(small_scene, seed=13, spp=3, chunk_paths=1000)
    ref = oracle.render(small_scene, integ.render_args(small_scene, 13, 3))
    np.testing.assert_array_equal(film, ref)
    assert film[..., 3].sum() > 0 and np.isfinite(film).all()


@pytest.mark.parametrize("spp,offset", [(3, 5), (4, 4)])
@pytest.mark.parametrize("band", [(0, None), (7, 20)])
def test_rank_shard_and_row_band(small_scene, oracle, spp, offset, band):
    """The sampler lane pix * spp_total + sample_offset + smp and the band's
    first row, in the trace, the shade and both film source kernels (spp 3:
    k_film_src, spp 4: k_film_src_staged)."""
    integ = _integ("path_test", max_depth=4)
    y0, y1 = band
    kw = dict(y0=y0, y1=y1, spp_total=8, sample_offset=offset)
    film = integ.render_film(small_scene, seed=6, spp=spp, chunk_paths=1500, **kw)
    ref = oracle.render(small_scene, integ.render_args(small_scene, 6, spp, **kw))
    np.testing.assert_array_equal(film, ref)
    assert film[..., 3].sum() > 0


def test_two_streams(small_scene, oracle):
    """73,728 paths: the default split alternates two wavefronts on two
    streams, so the camera source runs on the second one's buffers."""
    integ = _integ("path_test", max_depth=4)
    spp = 32
    assert small_scene.width * small_scene.height * spp >= 1 << 16
    film, st = integ.render_film(small_scene, seed=7, spp=spp, stats=True)
    assert st["streams"] == 2
    ref = oracle.render(small_scene, integ.render_args(small_scene, 7, spp))
    np.testing.assert_array_equal(film, ref)


def test_camera_change(small_scene, oracle):
    """Same geometry, another camera: trace, shade and film all read the
    current DevScene::camera."""
    from mtx import _abi

    integ = _integ("mypath", max_depth=4)
    first = integ.render_film(small_scene, seed=2, spp=3)
    cam = _abi.Camera.from_buffer_copy(bytes(small_scene.camera))
    cam.origin[0] += 0.25
    cam.origin[1] += 0.1
    cam.tan_x *= 0.8
    cam.tan_y *= 0.8
    moved = small_scene.with_camera(cam)
    film = integ.render_film(moved, seed=2, spp=3)
    ref = oracle.render(moved, integ.render_args(moved, 2, 3))
    np.testing.assert_array_equal(film, ref)
    assert not np.array_equal(film, first)
    # and back
    np.testing.assert_array_equal(integ.render_film(small_scene, seed=2, spp=3), first)


@pytest.mark.parametrize("name", ["path_test", "mypath"])
def test_environment(oracle, name):
    """A constant environment: PF_VALID_RAY in the derived initial flags
    (path_test's alpha on a primary miss) and the emitter index of a miss."""
    from mtx.mitsuba_dict import scene_from_dict

    sc = scene_from_dict(furnace(32, 32, albedo=0.8))
    integ = _integ(name, max_depth=6)
    film = integ.render_film(sc, seed=11, spp=3, chunk_paths=1000)
    ref = oracle.render(sc, integ.render_args(sc, 11, 3))
    np.testing.assert_array_equal(film, ref)
    assert film[1, 1, 3] > 0  # a corner pixel sees only the sky, and counts


def _lit_box(radiance, width=32, height=32):
    """The Cornell box closed by a front wall, seen from inside, its light
    grown to most of the ceiling: a large share of every bounce's hits are
    emitter hits."""
    d = cornell_box(width, height)
    d["sensor"] = dict(d["sensor"], fov=90.0, to_world=T.look_at(origin=[0, 0, 0.95], target=[0, 0, 0], up=[0, 1, 0]))
    d["front"] = {"type": "rectangle", "to_world": T().translate([0.0, 0.0, 1.0]).rotate([0, 1, 0], 180),
                  "bsdf": {"type": "ref", "id": "white"}}
    d["light"] = dict(d["light"], to_world=T().translate([0.0, 0.99, 0.0]).rotate([1, 0, 0], 90).scale(0.9),
                      emitter={"type": "area", "radiance": {"type": "rgb", "value": radiance}})
    return d


@pytest.mark.parametrize("name", ["path_test", "mypath"])
def test_emitter_hits_at_every_depth(oracle, name):
    """Emitter hits at every bounce: the emission MIS of each reads the
    previous vertex, the first of which follows the derived camera ray."""
    from mtx.mitsuba_dict import scene_from_dict

    sc = scene_from_dict(_lit_box([4.0, 3.0, 2.0]))
    dark = scene_from_dict(_lit_box([0.0, 0.0, 0.0]))
    integ = _integ(name, max_depth=6, rr_depth=3)
    ref = oracle.render(sc, integ.render_args(sc, 5, 4))
    ref_dark = oracle.render(dark, integ.render_args(dark, 5, 4))
    # the emitter term is exercised: most pixels change when its radiance is zeroed
    assert (np.abs(ref[..., :3] - ref_dark[..., :3]).sum(-1) > 0).mean() > 0.9
    film = integ.render_film(sc, seed=5, spp=4, chunk_paths=1500)
    np.testing.assert_array_equal(film, ref)


def test_restir_keeps_the_stored_raygen(small_scene, oracle):
    """ReSTIR GI reads the bounce-0 planes (k_rs_begin): cam0 clear, three
    frames bit-exact."""
    from mtx import load_dict
    from test_restir import CONFIGS, _oracle_frames

    sc = small_scene.with_film(40, 24)
    ref, _ = _oracle_frames(oracle, sc, CONFIGS["unbiased"], 3)
    integ = load_dict({"type": "restirgi", **CONFIGS["unbiased"]})
    for fr in range(3):
        np.testing.assert_array_equal(integ.render_film(sc, seed=fr, spp=1), ref[fr], err_msg=f"frame {fr}")


def test_pssmlt_path_keeps_the_stored_rays(small_scene, oracle):
    """pssmltpath's chains start from k_mlt_begin's stored rays: cam0 clear."""
    integ = _integ("pssmlt", iterations=45)
    sc = small_scene.with_film(32, 18)
    film = integ.render_film(sc, seed=2, spp=2, chunk_paths=700)
    ref = oracle.pssmlt_render(sc, integ.render_args(sc, 2, 2), 45)
    np.testing.assert_array_equal(film, ref)
    assert film[..., 3].sum() > 0


def test_bounce0_visit_counters(small_scene, oracle):
    """max_depth 1: the chunk's only closest-hit launch is the camera source's
    STATS twin. Its ray, node and triangle counts equal the oracle's traversal
    of the same camera rays (the oracle's film positions through its
    camera_ray)."""
    integ = _integ("path_test", max_depth=1)
    spp = 3
    film, st = integ.render_film(small_scene, seed=9, spp=spp, stats=True, counters=True)
    a = integ.render_args(small_scene, 9, spp)
    np.testing.assert_array_equal(film, oracle.render(small_scene, a))
    _, pos = oracle.render_samples(small_scene, a)
    adj = pos / np.array([small_scene.width, small_scene.height], np.float32)
    cr = oracle.probe(small_scene, "camera_ray", adj.astype(np.float32))
    rays = np.zeros((len(pos), 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = cr[:, 0:3], cr[:, 6], cr[:, 3:6]
    _, visits = oracle.trace(small_scene, rays, False)
    assert st["trace_launches"] == 1
    assert st["rays_closest"] == len(pos)
    assert st["nodes_closest"] == int(visits[:, 0].astype(np.uint64).sum())
    assert st["tris_closest"] == int(visits[:, 1].astype(np.uint64).sum())
