"""The query's walk, restated in numpy (hashgrid_query_cases.walk), against
brute force on every case of the GPU test: a conservative cell box plus the
own-cell filter finds exactly the brute-force neighbours in the brute-force
order, and the box of the plain q -+ r does not on group (b). No GPU."""
import numpy as np
import pytest

import hashgrid_query_cases as hq


def _check(case, widen=True):
    ref = hq.brute_force(case["p"], case["q"], case["r"], case["res"])
    got = hq.walk(case["p"], case["q"], case["r"], case["res"], case["n_cells"], widen)
    assert not isinstance(got, int), (case["name"], "queries over the cap", got)
    return hq.same(got, ref)


@pytest.mark.parametrize("n", hq.NS)
def test_walk_equals_brute_force_on_random_points(n):
    for case in hq.cases_random(n):
        assert _check(case), case["name"]


@pytest.mark.parametrize("group", ["lattice", "outside", "degenerate"])
def test_walk_equals_brute_force(group):
    for case in getattr(hq, "cases_" + group)():
        assert _check(case), case["name"]


def test_reference_meets_the_cases_it_is_for():
    """The lattice cases hold neighbours exactly at d2 = r^2 and duplicates;
    r = 0 finds the coincident pair; far queries find nothing."""
    by = {c["name"]: c for c in hq.cases_lattice() + hq.cases_outside()}
    c = by["b-exact-res12-c2"]
    count, _off, qi, si = hq.brute_force(c["p"], c["q"], c["r"], c["res"])
    d = c["p"][:, si].astype(np.float64) - c["q"][:, qi].astype(np.float64)
    assert ((d * d).sum(0) == 1.5625).sum() >= 30 * 3  # (1.25, 0, 0) and (0.75, 1, 0) families around inner queries
    n = c["p"].shape[1]
    dup = si[(qi == 0)]
    assert 0 in dup and n - 4 in dup and list(dup).index(0) < list(dup).index(n - 4)
    count, *_ = hq.brute_force(by["c-r0-res7"]["p"], by["c-r0-res7"]["q"], 0.0, 7)
    assert list(count) == [2, 1, 2]
    count, *_ = hq.brute_force(by["c-far-res7"]["p"], by["c-far-res7"]["q"], 0.1, 7)
    assert not count.any()


def test_unwidened_box_is_too_tight_on_the_lattice_group():
    """Group (b) tells a conservative box from the box of q -+ r: every `ulp`
    case loses its one-float-beyond sample without the widening."""
    lost = [c["name"] for c in hq.cases_lattice() if not _check(c, widen=False)]
    assert sorted(lost) == sorted(c["name"] for c in hq.cases_lattice() if "ulp" in c["name"]), lost


def test_cap():
    ok, over = hq.cases_cap()
    assert _check(ok)
    assert hq.walk(over["p"], over["q"], over["r"], over["res"], over["n_cells"]) == 1
    lo, hi = hq.cell_box(ok["q"][:, 0], ok["r"], 0.0, 1.0, 64)
    assert list(hi - lo + 1) == [16, 16, 16]
    lo, hi = hq.cell_box(over["q"][:, 0], over["r"], 0.0, 1.0, 64)
    assert list(hi - lo + 1) == [17, 17, 17]
