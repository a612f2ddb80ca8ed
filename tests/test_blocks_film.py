"""The numpy restatement of blocks.Film (tests/blocks_film_cases.py) against
the oracle, on the CPU: with uniform sample counts it is the oracle's film
bit for bit, and tests/test_rfilter_gpu.py's restatement for the box and the
gaussian. That anchors it before tests/test_blocks_film_gpu.py uses it as the
reference for masked, shuffled and ragged puts."""
import blocks_film_cases as fc
import numpy as np
import pytest
from test_rfilter_gpu import BOX, GAUSSIAN, NAMES, TENT, _film_slot, _restated

F32 = np.float32


@pytest.mark.parametrize("spp", fc.SPPS)
def test_uniform_counts_equal_the_oracle_film(small_scene, oracle, spp):
    sc = small_scene
    a, L, pos, pix = fc.band_samples(sc, oracle, spp)
    got = fc.raw_np(fc.planes_np(oracle, TENT, sc.width, fc.Y0, fc.Y1, pix, L, pos))
    np.testing.assert_array_equal(got, oracle.film(sc.width, fc.Y0, fc.Y1, spp, L, pos))
    np.testing.assert_array_equal(got, oracle.render(sc, a))
    assert got[..., :3].sum() > 0
    # T given equals T counted when every pixel has spp samples
    np.testing.assert_array_equal(
        got, fc.raw_np(fc.planes_np(oracle, TENT, sc.width, fc.Y0, fc.Y1, pix, L, pos, spp_total=spp)))


def test_sample_shard_equals_the_oracle_film(small_scene, oracle):
    sc = small_scene
    a, L, pos, pix = fc.band_samples(sc, oracle, 4, spp_total=8, sample_offset=4)
    got = fc.raw_np(fc.planes_np(oracle, TENT, sc.width, fc.Y0, fc.Y1, pix, L, pos, spp_total=8, sample_offset=4))
    np.testing.assert_array_equal(got, oracle.film(sc.width, fc.Y0, fc.Y1, 4, L, pos, spp_total=8, sample_offset=4))
    np.testing.assert_array_equal(got, oracle.render(sc, a))


@pytest.mark.parametrize("rfilter", ["box", "gaussian"])
@pytest.mark.parametrize("spp", fc.SPPS)
def test_box_and_gaussian_equal_the_uniform_restatement(small_scene, oracle, spp, rfilter):
    sc = small_scene
    a, L, pos, pix = fc.band_samples(sc, oracle, spp)
    fid = NAMES[rfilter]
    assert fid in (BOX, GAUSSIAN)
    got = fc.raw_np(fc.planes_np(oracle, fid, sc.width, fc.Y0, fc.Y1, pix, L, pos))
    np.testing.assert_array_equal(got, _restated(oracle, fid, sc, a, L, pos))


def test_slots_of_ragged_counts():
    """film_slots is film_slot per element, for every count a pixel of the tests can have."""
    for T in range(1, 20):
        g = np.arange(T + 3)
        assert fc.film_slots(g, np.full(len(g), T)).tolist() == [_film_slot(int(x), T) for x in g]


def test_passes_continue_from_the_planes(small_scene, oracle):
    """Whole-pixel passes and sample passes with spp_total / sample_offset rebuild the single put's planes."""
    sc = small_scene
    _, L, pos, pix = fc.band_samples(sc, oracle, 9)
    one = fc.planes_np(oracle, TENT, sc.width, fc.Y0, fc.Y1, pix, L, pos)
    cut = 100 * 9
    two = fc.planes_np(oracle, TENT, sc.width, fc.Y0, fc.Y1, pix[:cut], L[:cut], pos[:cut])
    two = fc.planes_np(oracle, TENT, sc.width, fc.Y0, fc.Y1, pix[cut:], L[cut:], pos[cut:], planes=two)
    np.testing.assert_array_equal(one, two)
    first = (np.arange(len(pix)) % 9) < 4
    two = fc.planes_np(oracle, TENT, sc.width, fc.Y0, fc.Y1, pix[first], L[first], pos[first], spp_total=9)
    two = fc.planes_np(oracle, TENT, sc.width, fc.Y0, fc.Y1, pix[~first], L[~first], pos[~first], spp_total=9,
                       sample_offset=4, planes=two)
    np.testing.assert_array_equal(one, two)
