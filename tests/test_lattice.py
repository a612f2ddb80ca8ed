"""The CPU oracle's traversal (BVH and brute force) on the exact lattice scenes
of lattice_cases.py: closest hit and any hit equal an independent float64
reference bit for bit at the places generic rays never reach -- origins on a
surface, hits on edges, diagonals and shared vertices, coincident sheets,
rays inside a sheet's plane, zero and negative-zero direction components,
maxt equal to t and one ulp below, scaled directions, a translated scene, a
host refit -- and within a derived rounding bound on a rotated copy. The
kernels' twin is test_lattice_gpu.py. (No GPU.)"""
import numpy as np
import pytest

import lattice_cases as lc


@pytest.fixture(scope="module")
def lat(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lattice"))


def _oracle_traces(oracle):
    return {"bvh": lambda s, r, m: oracle.trace(s, r, m)[0],
            "brute": lambda s, r, m: (oracle.trace(s, r, brute=True)[0] if m == 0 else
                                      (oracle.trace(s, r, brute=True)[0].reshape(-1, 4)[:, 1] != lc.MISS))}


def _check_both(oracle, scene, rays, words, occluded, label):
    for name, trace in _oracle_traces(oracle).items():
        lc.check_trace(trace, scene, rays, words, occluded, (label, name))


def test_reference_forms_agree(lat):
    """The matrix-product form of the reference equals textbook
    Moeller-Trumbore pair by pair, bounded rays included."""
    s = lc.build(lat, "plain")
    rays = lc.rays_a()[::29].copy()
    rays[::3, 3] = 1.0
    rays[1::3, 3] = 0.25
    a, b = lc.lattice_reference(s.tri_geom, rays), lc.direct_reference(s.tri_geom, rays)
    for k in lc._FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert 0 < a.any.sum() < len(rays)


def test_class_a_lattice_rays(lat, oracle):
    s = lc.build(lat, "plain")
    rays = lc.rays_a()
    ref, occ = lc.refs("a", s, rays)
    counts = lc.assert_class_a_not_hollow(s.tri_geom, ref)
    print(len(rays), counts)
    assert np.array_equal(ref.any, occ.any)  # the occlusion records are a permutation
    _check_both(oracle, s, rays, ref.words(), occ.any, "a")


def test_class_b_bounded_rays(lat, oracle):
    """maxt = t keeps the hit; one ulp below it is gone and the reference
    decides what replaces it (a farther sheet, or nothing)."""
    s = lc.build(lat, "plain")
    rays = lc.rays_a()
    ra, _ = lc.refs("a", s, rays)
    at, below = lc.rays_b(rays, ra)
    rat, oat = lc.refs("b-at", s, at)
    assert np.array_equal(rat.words(), ra.words()[ra.prim != lc.MISS]) and oat.any.all()
    rbe, obe = lc.refs("b-below", s, below)
    assert (rbe.prim == lc.MISS).all() and not obe.any.any()  # nothing lies nearer than the closest hit
    _check_both(oracle, s, at, rat.words(), oat.any, "b-at")
    _check_both(oracle, s, below, rbe.words(), obe.any, "b-below")
    # a bound between the first and the second sheet: the reference decides
    mid = rays[::3].copy()
    mid[:, 3] = 0.75
    rm, om = lc.refs("b-mid", s, mid)
    assert 0.05 < om.any.mean() < 0.95  # both answers occur
    _check_both(oracle, s, mid, rm.words(), om.any, "b-mid")


@pytest.mark.parametrize("k", [-40, -30, 30, 60])
def test_class_c_direction_scale(lat, oracle, k):
    """mtx_trace's stated range for the direction (include/mtx.h): the largest
    component magnitude within [2^-40, 2^60]. prim, u, v are unchanged and t
    scales by 2^-k exactly; a subset is recomputed by the reference itself."""
    s = lc.build(lat, "plain")
    rays = lc.rays_a()
    ref, occ = lc.refs("a", s, rays)
    r2 = lc.scaled(rays, k)
    words = lc.scaled_words(ref, k)
    sub = lc.lattice_reference(s.tri_geom, r2[::11])
    assert np.array_equal(sub.words(), words[::11])
    _check_both(oracle, s, r2, words, occ.any, ("c", k))


def test_class_d_translated_scene(lat, oracle):
    s = lc.build(lat, "plain", translated=True)
    rays = lc.rays_a(lc.OFFSET)
    ref, occ = lc.refs("d", s, rays)
    base, _ = lc.refs("a", lc.build(lat, "plain"), lc.rays_a())
    assert np.array_equal(ref.t, base.t) and np.array_equal(ref.any, base.any)
    _check_both(oracle, s, rays, ref.words(), occ.any, "d")


def test_class_e_degenerate_directions(lat, oracle):
    """d = 0 misses in both modes; NaN and inf rays terminate and miss (host
    only: none of those is sent to a device)."""
    s = lc.build(lat, "plain")
    rays = lc.rays_zero()
    miss = np.tile(np.array([np.float32(np.inf).view(np.uint32), lc.MISS, 0, 0], np.uint32), (len(rays), 1))
    _check_both(oracle, s, rays, miss, np.zeros(len(rays), bool), "e")
    odd = lc.rays_a()[:37 * 40].copy()
    for j, (col, val) in enumerate([(0, np.nan), (4, np.nan), (5, np.inf), (6, -np.inf), (1, np.inf), (3, np.nan)]):
        odd[j::6, col] = val
    odd[5::6, 4:7] = np.nan  # NaN maxt and direction
    miss = np.tile(miss[:1], (len(odd), 1))
    _check_both(oracle, s, odd, miss, np.zeros(len(odd), bool), "e-nonfinite")


def test_class_f_off_lattice(lat, oracle):
    """The accuracy of tri_intersect itself, on the rotated scene: clear rays
    (lattice_cases.offlattice_classes; the bound TAU_C 2^-24 sum|terms| / |det|
    is derived there) agree with the float64 reference in prim exactly and in
    t, u, v within the bound. At most a quarter of the class is borderline and
    every aim kind keeps 200 clear rays."""
    s = lc.build(lat, "rot")
    rays, kinds = lc.rays_f(s.tri_geom)
    ref, clear, bt, bu, bv = lc.cached("f", lambda: lc.offlattice_classes(s.tri_geom, rays))
    assert (~clear).mean() <= 0.25, (~clear).mean()
    for ki, (kind, _) in enumerate(lc.AIM_KINDS):
        assert (clear & (kinds == ki)).sum() >= 200, (kind, (clear & (kinds == ki)).sum())
    brute = oracle.trace(s, rays, brute=True)[0].reshape(-1, 4)
    assert np.array_equal(oracle.trace(s, rays)[0].reshape(-1, 4), brute)
    lc.check_off_lattice(brute, ref, clear, bt, bu, bv)


def test_emitting_side_radiance(lat, oracle):
    """CPU twin of the production closest-hit check: the ``integrator``
    estimator at max_depth 1 on the ``emit`` scene returns the hit sheet's
    radiance on its emitting side and 0 elsewhere; valid = hit. Exact."""
    from mtx import load_dict

    s = lc.build(lat, "emit")
    assert len(s.emitters) == 3 * len(lc.PLANES)
    rays = lc.rays_a()
    ref, _ = lc.refs("a-emit", s, rays)
    L, valid = lc.expected_radiance(s, s.tri_geom, rays, ref)
    lit = (L != 0).any(1)
    assert 0.2 < lit.mean() < 0.8 and len(np.unique(L[lit], axis=0)) >= 15  # of 18: a twin sheet may hide its twin
    integ = load_dict({"type": "integrator", "max_depth": 1})
    Lc, vc = oracle.sample_rays(s, integ.render_args(s, 1, 1), np.concatenate([rays[:, 0:3], rays[:, 4:7]], 1),
                                np.arange(len(rays), dtype=np.uint32), 2)
    assert np.array_equal(vc.astype(bool), valid) and np.array_equal(Lc, L)


def test_after_host_refit(lat, oracle):
    """The z stack moved by a lattice vector (Scene.with_vertices: both trees
    refit, not rebuilt): class (a) against the reference recomputed from the
    moved records."""
    s = lc.build(lat, "plain")
    t = lc.cached("moved", lambda: s.with_vertices(lc.moved_vertices(s)))
    rays = lc.rays_a()
    ref, occ = lc.refs("a-moved", t, rays)
    base, _ = lc.refs("a", s, rays)
    assert (ref.words() != base.words()).any(1).mean() > 0.1
    _check_both(oracle, t, rays, ref.words(), occ.any, "refit")
