"""Chi-square goodness of fit of sampled directions and warps against the
density they claim: the shared harness (numpy / scipy, float64) and the case
tables of tests/test_sampling_chi2.py and tests/test_sampling_chi2_gpu.py.

The histogram is a grid of cells in two coordinates ((theta, phi) on the
sphere, with the horizon on a cell edge). The expected count of a cell is
n_total times the integral of the density over it, by Gauss-Legendre
quadrature with q x q points per cell. Every cell is integrated at two
densities, q and 2 q points per axis; a cell whose two integrals differ by
more than a small fraction of its own statistical spread is doubled again.
The statistic is evaluated against both sets of expected counts and the
harness asserts that the two differ by less than 0.1 sqrt(2 dof): the
quadrature proves its own convergence, case by case.

Cells are pooled as Mitsuba's ChiSquareTest does: sorted by expected count,
the lowest go into one pooled cell until it holds at least 5."""
import copy
import math

import numpy as np
from scipy import special, stats

N_SAMPLES = 1_000_000
SIGNIFICANCE = 0.01
Z_THRESHOLD = 5.5  # the project's z bound (tests/test_gpu_convergence.py)

# BSDFFlags bits (mtx_core/bsdf.h)
BF_NULL, BF_DELTA_REFLECTION = 0x01, 0x20


def sidak(n_cases, level=SIGNIFICANCE):
    """Mitsuba's rule: with K cases in a module each passes at p > 1 - (1 - level)^(1/K)."""
    return 1.0 - (1.0 - level) ** (1.0 / n_cases)


# --------------------------------------------------------------- harness --
class Chi2Result(dict):
    __getattr__ = dict.__getitem__


def _integrate(density, a_edges, b_edges, cells, q, chunk=1 << 20):
    """Integral of density(a, b) over each of `cells` (flat index ia * nb + ib), q x q Gauss-Legendre points."""
    nb = len(b_edges) - 1
    x, w = np.polynomial.legendre.leggauss(q)
    out = np.empty(len(cells))
    step = max(1, chunk // (q * q))
    for s in range(0, len(cells), step):
        c = cells[s: s + step]
        ia, ib = np.divmod(c, nb)
        a0, a1, b0, b1 = a_edges[ia], a_edges[ia + 1], b_edges[ib], b_edges[ib + 1]
        a = (0.5 * (a0 + a1))[:, None] + (0.5 * (a1 - a0))[:, None] * x  # (C, q)
        b = (0.5 * (b0 + b1))[:, None] + (0.5 * (b1 - b0))[:, None] * x
        A = np.broadcast_to(a[:, :, None], (len(c), q, q)).reshape(-1)
        B = np.broadcast_to(b[:, None, :], (len(c), q, q)).reshape(-1)
        f = np.asarray(density(A, B), np.float64).reshape(len(c), q, q)
        wa = (0.5 * (a1 - a0))[:, None] * w
        wb = (0.5 * (b1 - b0))[:, None] * w
        out[s: s + step] = np.einsum("cij,ci,cj->c", f, wa, wb)
    return out


def _pooled_statistic(observed, expected, pooled, extra_observed):
    e, o = expected[~pooled], observed[~pooled]
    stat = float((((o - e) ** 2) / e).sum())
    pe, po = float(expected[pooled].sum()), float(observed[pooled].sum()) + extra_observed
    if pooled.any() or extra_observed:
        stat += (po - pe) ** 2 / pe if pe > 0 else (np.inf if po > 0 else 0.0)
    return stat


def grid_chi2(counts, density, a_edges, b_edges, n_total, outside=0, q=4, q_max=256, min_expected=5.0):
    """Chi-square test of a 2-D histogram. `counts[ia, ib]` are the observed
    cell counts, `outside` the samples that fell off the grid (they join the
    pooled cell, whose expected count has nothing for them), `density(a, b)`
    the claimed density in the grid's own coordinates (Jacobian included),
    `n_total` the number of samples drawn, valid or not.

    Returns statistic, dof, p, integral (of the density over the grid),
    quad_term (difference of the two integrals), stat_coarse, conv (the
    asserted |statistic - stat_coarse| / sqrt(2 dof)), q (most points per
    axis any cell needed, at the coarser of its two densities) and points."""
    a_edges, b_edges = np.asarray(a_edges, np.float64), np.asarray(b_edges, np.float64)
    observed = np.asarray(counts, np.float64).reshape(-1)
    ncell = (len(a_edges) - 1) * (len(b_edges) - 1)
    assert observed.shape == (ncell,)
    cells = np.arange(ncell)
    coarse = n_total * _integrate(density, a_edges, b_edges, cells, q)
    fine = n_total * _integrate(density, a_edges, b_edges, cells, 2 * q)
    points = ncell * 5 * q * q
    q_of = np.full(ncell, q)
    while True:
        # a cell is settled once doubling moves it by under 0.2 % of its Poisson spread
        todo = cells[np.abs(fine - coarse) > 2e-3 * np.sqrt(np.maximum(fine, 1e-2))]
        todo = todo[q_of[todo] * 4 <= q_max]
        if not len(todo):
            break
        for qq in np.unique(q_of[todo]):
            c = todo[q_of[todo] == qq]
            coarse[c] = fine[c]
            fine[c] = n_total * _integrate(density, a_edges, b_edges, c, 4 * qq)
            q_of[c] = 2 * qq
            points += len(c) * 16 * qq * qq
    # pooling (by the finer counts; the same cells for both statistics)
    order = np.argsort(fine, kind="stable")
    csum = np.cumsum(fine[order])
    n_pool = int((fine < min_expected).sum())  # every cell below the minimum, then more until the pool holds it
    while 0 < n_pool < ncell and csum[n_pool - 1] < min_expected:
        n_pool += 1
    pooled = np.zeros(ncell, bool)
    pooled[order[:n_pool]] = True
    dof = int((~pooled).sum()) + (1 if (n_pool or outside) else 0) - 1
    assert dof >= 1, "the grid leaves no degree of freedom"
    stat = _pooled_statistic(observed, fine, pooled, outside)
    stat_c = _pooled_statistic(observed, coarse, pooled, outside)
    conv = abs(stat - stat_c) / math.sqrt(2.0 * dof)
    r = Chi2Result(statistic=stat, dof=dof, p=float(stats.chi2.sf(stat, dof)), integral=float(fine.sum() / n_total),
                   quad_term=float(abs(fine.sum() - coarse.sum()) / n_total), stat_coarse=stat_c, conv=conv,
                   q=int(q_of.max()), points=int(points), n_pooled=n_pool)
    assert conv < 0.1, f"quadrature not converged: statistic {stat_c:.3f} -> {stat:.3f} at dof {dof} (q {r.q})"
    return r


class SphereGrid:
    """(theta, phi) cells over the whole sphere, uniform in both angles; an
    even number of theta cells puts the horizon on an edge."""

    def __init__(self, n_theta=32, n_phi=32):
        assert n_theta % 2 == 0
        self.n_theta, self.n_phi = n_theta, n_phi
        self.theta_edges = np.linspace(0.0, math.pi, n_theta + 1)
        self.theta_edges[n_theta // 2] = 0.5 * math.pi
        self.phi_edges = np.linspace(0.0, 2.0 * math.pi, n_phi + 1)

    def histogram(self, d):
        d = np.asarray(d, np.float64)
        theta = np.arccos(np.clip(d[:, 2] / np.linalg.norm(d, axis=1), -1.0, 1.0))
        phi = np.mod(np.arctan2(d[:, 1], d[:, 0]), 2.0 * math.pi)
        it = np.minimum((theta * (self.n_theta / math.pi)).astype(np.int64), self.n_theta - 1)
        # a direction on the horizon belongs to the side its z has
        it = np.where((d[:, 2] > 0) & (it >= self.n_theta // 2), self.n_theta // 2 - 1, it)
        it = np.where((d[:, 2] < 0) & (it < self.n_theta // 2), self.n_theta // 2, it)
        ip = np.minimum((phi * (self.n_phi / (2.0 * math.pi))).astype(np.int64), self.n_phi - 1)
        return np.bincount(it * self.n_phi + ip, minlength=self.n_theta * self.n_phi).reshape(self.n_theta, self.n_phi)


def directions(theta, phi):
    st = np.sin(theta)
    return np.stack([st * np.cos(phi), st * np.sin(phi), np.cos(theta)], 1)


def sphere_chi2(sample_dirs, pdf_fn, n_total, grid=None, counts=None, **kw):
    """Directions `sample_dirs` (the valid samples only; or their histogram
    `counts` on `grid`) against `pdf_fn(dirs (M, 3) float64) -> (M,)`, a
    density per solid angle. `n_total` is the number of samples drawn."""
    grid = grid or SphereGrid()
    if counts is None:
        counts = grid.histogram(sample_dirs)

    def density(theta, phi):
        return np.asarray(pdf_fn(directions(theta, phi)), np.float64) * np.sin(theta)

    return grid_chi2(counts, density, grid.theta_edges, grid.phi_edges, n_total, **kw)


def plane_chi2(a, b, density, a_edges, b_edges, n_total, **kw):
    """The 2-D variant: samples in coordinates (a, b) of the caller's choice
    against the density in those coordinates."""
    a_edges, b_edges = np.asarray(a_edges, np.float64), np.asarray(b_edges, np.float64)
    ia = np.searchsorted(a_edges, a, side="right") - 1
    ib = np.searchsorted(b_edges, b, side="right") - 1
    na, nb = len(a_edges) - 1, len(b_edges) - 1
    ia = np.where(a == a_edges[-1], na - 1, ia)
    ib = np.where(b == b_edges[-1], nb - 1, ib)
    inside = (ia >= 0) & (ia < na) & (ib >= 0) & (ib < nb)
    counts = np.bincount(ia[inside] * nb + ib[inside], minlength=na * nb).reshape(na, nb)
    return grid_chi2(counts, density, a_edges, b_edges, n_total, outside=int((~inside).sum()), **kw)


def z_binomial(k, n, p):
    """z of k successes in n draws of probability p (0 when p is 0 or 1 and k agrees)."""
    var = n * p * (1.0 - p)
    if var <= 0:
        return 0.0 if k == round(n * p) else math.inf
    return (k - n * p) / math.sqrt(var)


# The pdf is evaluated in float32 at float32 directions: a handful of roundings
# of 2^-24 each, which the integral inherits (it matters where the binomial
# spread is zero: the diffuse lobe's valid share is exactly 1).
F32_TERM = 8 * 2.0 ** -24


def classify(sample_pdf, pdf_at_sample, weight):
    """(valid, delta, zero) masks of drawn samples: zero-weight samples and
    delta samples (a sampled pdf > 0 where the evaluated pdf is 0 and the
    weight is not: the mask's pass-through) stay out of the histogram."""
    nonzero = (weight != 0).any(1)
    return (pdf_at_sample > 0) & nonzero, (sample_pdf > 0) & (pdf_at_sample == 0) & nonzero, ~nonzero


def check_bsdf_case(r, material, what, p_min):
    """The assertions of one BSDF case: r is sphere_chi2's result with the
    counts n (drawn), valid, delta and zero added.

    Mass balance: |valid share - integral of the pdf| <= 5.5 sigma + the
    quadrature term (+ the float32 term). sigma is the binomial spread at the
    observed share s or at the hypothesised mass I = min(integral, 1),
    whichever is larger: at s alone (the Wald form) it is 0 whenever all n
    samples are valid, which a true mass of 1 - 1e-6 produces almost surely at
    n = 1e4, and the test would then hold the quadrature to 1e-7 instead of
    the sampler to 5.5 sigma. The spread at I is the score form of the same
    z-test; where s is not 0 or 1 the two differ by a negligible amount."""
    n = r.n
    share = r.valid / n
    mass = min(r.integral, 1.0)
    sigma = math.sqrt(max(share * (1 - share), mass * (1 - mass)) / n)
    tol = Z_THRESHOLD * sigma + r.quad_term + F32_TERM
    print(f"{what}: chi2 {r.statistic:.1f} dof {r.dof} p {r.p:.4f} | int pdf {r.integral:.6f} valid {share:.6f} "
          f"(tol {tol:.1e}, quad {r.quad_term:.1e}) | delta {r.delta / n:.5f} | q {r.q} pts {r.points} "
          f"conv {r.conv:.4f}")
    assert r.p > p_min, f"{what}: chi2 {r.statistic:.1f} at {r.dof} dof, p = {r.p:.3g} <= {p_min:.3g}"
    assert abs(share - r.integral) <= tol, (what, share, r.integral, tol)
    assert r.valid + r.delta + r.zero == n
    if material.flags & MF_MASK:
        assert abs(z_binomial(r.delta, n, 1.0 - float(material.opacity))) <= Z_THRESHOLD, (what, r.delta / n)
    else:
        assert r.delta == 0, (what, r.delta)


# --------------------------------------------- Beckmann: the Smith G1 fit --
def g1_exact(a):
    """Smith G1 of the Beckmann distribution, a = 1 / (alpha tan theta)."""
    a = np.asarray(a, np.float64)
    return 2.0 / (1.0 + special.erf(a) + np.exp(-a * a) / (a * math.sqrt(math.pi)))


def g1_fit(a):
    """The rational fit Microfacet::smith_g1 uses (Walter et al. 2007), float64."""
    a = np.asarray(a, np.float64)
    return np.where(a >= 1.6, 1.0, (3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a))


def g1_ratio(alpha, wi):
    """G1_exact(wi) / G1_fit(wi): what the density of Beckmann visible-normal
    samples is, over what Microfacet::pdf reports, at every direction."""
    wi = np.asarray(wi, np.float64)
    s = math.hypot(wi[0], wi[1])
    if s == 0.0:
        return 1.0
    a = abs(wi[2]) / (alpha * s)
    return float(g1_exact(a) / g1_fit(a))


# ------------------------------------------------------------- the cases --
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# normal, two oblique, grazing (cos theta = 0.05), and one below the surface
WI = {
    "normal": _unit([0.0, 0.0, 1.0]),
    "oblique": _unit([0.3, 0.1, 0.9]),
    "steep": _unit([0.95, 0.0, 0.3]),
    "grazing": np.array([math.sqrt(1 - 0.05 ** 2) * math.cos(2.0), math.sqrt(1 - 0.05 ** 2) * math.sin(2.0), 0.05]),
    "below": _unit([0.2, -0.5, -0.7]),
}
UV = {"uv0": (0.3, 0.3), "uv1": (0.81, 0.07)}
ALPHAS = (None, 0.3, 0.5)  # None: the scene's own

_TYPE = {1: "diffuse", 2: "roughplastic", 3: "conductor", 4: "roughconductor", 5: "dielectric", 6: "roughdielectric"}
MF_MASK, MF_BECKMANN = 2, 4
# the material keys small_scene has, by the first material of each: (name, rough, second uv)
KEYS = (
    ("roughconductor_ggx", True, False),
    ("diffuse", False, True),
    ("diffuse_mask", False, True),
    ("roughdielectric_beckmann", True, False),
    ("roughconductor_beckmann", True, False),
    ("roughplastic_ggx", True, True),
    ("roughplastic_beckmann", True, True),
)


def key_name(m):
    t = _TYPE[int(m.type)]
    if int(m.type) in (2, 4, 6):
        t += "_beckmann" if m.flags & MF_BECKMANN else "_ggx"
    return t + ("_mask" if m.flags & MF_MASK else "")


def material_ids(scene):
    """{key name: first material id that has it} (the keys of tests/test_core_math.py)."""
    out = {}
    for i, m in enumerate(scene.materials):
        out.setdefault(key_name(m), i)
    return out


def bsdf_cases():
    """(id, key, alpha or None, wi name, uv name) of every chi-square BSDF case; the list index seeds it."""
    cases = []
    for key, rough, uv2 in KEYS:
        for alpha in ALPHAS if rough else (None,):
            for uv in ("uv0", "uv1") if (uv2 and alpha is None) else ("uv0",):
                for wi in WI:
                    a = "" if alpha is None else f"-a{alpha}"
                    cases.append((f"{key}{a}-{wi}-{uv}", key, alpha, wi, uv))
    return cases


def seed_of(index):
    return 7919 * index + 13


def scene_with_alpha(alpha, **kw):
    """The bedroom proxy with every rough BSDF's alpha replaced, through the
    loader (the roughplastic tables are rebuilt for the new alpha)."""
    from mtx import scene

    spec = copy.deepcopy(scene.load_bedroom_spec())

    def walk(b):
        if isinstance(b, dict):
            if b.get("type") in ("roughconductor", "roughdielectric", "roughplastic"):
                b["alpha"] = alpha
            for v in b.values():
                walk(v)

    walk(spec["bsdfs"])
    return scene.Scene.bedroom(spec=spec, **kw)


def true_pdf_scale(scene, mid, wi, pdf, cos_o):
    """The evaluated pdf corrected to the density the sampler really has.
    Beckmann only: Microfacet::pdf multiplies by the rational fit of G1(wi),
    sample_visible_11 inverts the exact distribution, so the microfacet lobe
    is G1_exact / G1_fit times what pdf reports (upstream has the same). The
    roughplastic diffuse lobe (prob_diffuse cos / pi) is left alone."""
    m = scene.materials[mid]
    if not (m.flags & MF_BECKMANN) or int(m.type) not in (2, 4, 6):
        return pdf
    ratio = g1_ratio(float(m.alpha), wi)
    if int(m.type) != 2:
        return pdf * ratio
    tab = np.asarray(scene.tables[m.table: m.table + 64], np.float64)
    x = abs(float(np.float32(wi[2]))) * 63.0
    i = min(int(x), 62)
    t_i = tab[i] + (tab[i + 1] - tab[i]) * (x - i)
    ps, pd = (1.0 - t_i) * m.spec_weight, t_i * (1.0 - m.spec_weight)
    pd = pd / (ps + pd)
    diffuse = pd * np.maximum(cos_o, 0.0) / math.pi * (pdf > 0)
    return (pdf - diffuse) * ratio + diffuse
