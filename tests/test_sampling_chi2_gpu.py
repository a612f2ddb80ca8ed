"""The chi-square loop closed on device outputs alone: one
Scene.bsdf_eval_pdf_sample call of 2^21 lanes (every wave holds every
material, an active mask, u from blocks.Sampler), the histogram of each
(material, wi) by torch.bincount, and expected counts from the kernel's own
pdf at the quadrature directions. The same lanes bit for bit against the
oracle's probe, 512 times the lane count tests/test_blocks_gpu.py::test_bsdf
feeds, and once more with a ragged last wave."""
import chi2_cases as cc
import numpy as np
import pytest
from test_blocks_gpu import active_of, dev, host, same

pytestmark = pytest.mark.gpu

N0 = 1 << 21
SIZES = (N0, N0 + 65)
WI_NAMES = tuple(cc.WI)
CASES = [(key, wi) for key, _, _ in cc.KEYS for wi in WI_NAMES]
P_MIN = cc.sidak(len(CASES))
GRID = cc.SphereGrid(16, 16)  # about 10 600 active lanes per (material, wi)
SEED = 29
_REF = {}


def lanes_of(sc, n):
    """Per lane: material (all of them and -1 in every wave), wi (one of the case directions), uv, active."""
    nm = len(sc.materials)
    lane = np.arange(n)
    mat = ((lane + 1) % (nm + 1) - 1).astype(np.int32)
    wi_idx = (lane // (nm + 1)) % len(WI_NAMES)
    wi = np.float32([cc.WI[k] for k in WI_NAMES])[wi_idx]
    uv = np.float32(list(cc.UV.values()))[(lane // ((nm + 1) * len(WI_NAMES))) % len(cc.UV)]
    return mat, wi_idx, wi, uv, active_of(n)


def reference(oracle, sc, u):
    """oracle.bsdf_probe of the first len(u) lanes, once for the largest size (the lanes of a
    smaller one are its first)."""
    n = len(u)
    if "want" not in _REF or len(_REF["u"]) < n:
        mat, _, wi, uv, _ = lanes_of(sc, n)
        want = np.zeros((n, 16), np.float32)
        for m in range(len(sc.materials)):
            idx = np.nonzero(mat == m)[0]
            want[idx] = oracle.bsdf_probe(sc, m, wi[idx], np.zeros((len(idx), 3), np.float32), uv[idx], u[idx])[0]
        _REF["want"], _REF["u"] = want, u
    same(u, _REF["u"][:n], "the sampler's draws do not depend on the lane count")
    return _REF["want"][:n]


def cell_index(wo):
    """GRID's cell of each column of wo (3, N), on the device, as cc.SphereGrid.histogram does it."""
    import torch

    w = wo.double()
    z = w[2] / torch.linalg.vector_norm(w, dim=0).clamp_min(1e-300)
    theta = torch.acos(z.clamp(-1.0, 1.0))
    phi = torch.remainder(torch.atan2(w[1], w[0]), 2.0 * np.pi)
    nt, nph = GRID.n_theta, GRID.n_phi
    it = (theta * (nt / np.pi)).long().clamp_max(nt - 1)
    it = torch.where((w[2] > 0) & (it >= nt // 2), nt // 2 - 1, it)
    it = torch.where((w[2] < 0) & (it < nt // 2), nt // 2, it)
    ip = (phi * (nph / (2.0 * np.pi))).long().clamp_max(nph - 1)
    return it * nph + ip


@pytest.mark.parametrize("n", sorted(SIZES, reverse=True))
def test_bsdf_chi2_on_device(small_scene, oracle, n):
    import torch
    from mtx import blocks

    sc = small_scene
    scn = blocks.Scene(sc)
    ids = cc.material_ids(sc)
    mat, wi_idx, wi, uv, act = lanes_of(sc, n)
    si = blocks.SurfaceInteraction(dev(mat).device, n)
    si.material.copy_(dev(mat))
    si.uv.copy_(dev(uv))
    si.wi.copy_(dev(wi))
    sampler = blocks.Sampler(SEED, np.arange(n, dtype=np.uint32))
    u1, u2 = sampler.next_1d(), sampler.next_2d()
    active = dev(act)
    val, pdf, bs, weight = scn.bsdf_eval_pdf_sample(si, torch.zeros((3, n), device=u1.device), u1, u2, active)

    # ---- every lane against the oracle's probe, bit for bit
    u = np.concatenate([host(u1)[:, None], host(u2)], 1)
    assert u.min() >= 0 and u.max() < 1
    want = reference(oracle, sc, u)
    got_wo, got_pdf, got_w = host(bs.wo), host(bs.pdf), host(weight)
    same(got_wo[act], want[act, 4:7], "sample wo")
    same(got_pdf[act], want[act, 7], "sample pdf")
    same(host(bs.eta)[act], want[act, 8], "sample eta")
    same(host(bs.sampled_type)[act], want[act, 9].view(np.int32), "sample type")
    same(got_w[act], want[act, 10:13], "weight")
    for t in (val, pdf, bs.wo, bs.pdf, bs.eta, bs.sampled_type, weight):
        assert not host(t)[~act].any()

    # ---- the histograms of all (material, wi) in one bincount
    _, pdf_at, _, _ = scn.bsdf_eval_pdf_sample(si, bs.wo, u1, u2, active)
    nonzero = (weight != 0).any(0)
    drawn = active & dev(mat >= 0)  # the lanes that drew a sample of a material
    valid = (pdf_at > 0) & nonzero & drawn
    delta = (bs.pdf > 0) & (pdf_at == 0) & nonzero & drawn
    zero = ~nonzero & drawn
    ncell = GRID.n_theta * GRID.n_phi
    nm = len(sc.materials)
    group = (torch.as_tensor(mat, device=u1.device).long().clamp_min(0) * len(WI_NAMES)
             + torch.as_tensor(wi_idx, device=u1.device))
    counts = torch.bincount((group * ncell + cell_index(bs.wo))[valid], minlength=nm * len(WI_NAMES) * ncell)
    counts = counts.reshape(nm, len(WI_NAMES), ncell).cpu().numpy()

    def tally(mask):
        return torch.bincount(group[mask], minlength=nm * len(WI_NAMES)).reshape(nm, len(WI_NAMES)).cpu().numpy()

    n_valid, n_delta, n_zero, n_drawn = tally(valid), tally(delta), tally(zero), tally(drawn)

    # ---- expected counts from the kernel's own pdf at the quadrature directions
    def device_pdf(mid, w, tex):
        def pdf_fn(d):
            m = len(d)
            q = blocks.SurfaceInteraction(u1.device, m)
            q.material.fill_(mid)
            q.uv.copy_(dev(np.broadcast_to(np.float32(tex), (m, 2))))
            q.wi.copy_(dev(np.broadcast_to(np.float32(w), (m, 3))))
            z1, z2 = torch.zeros(m, device=u1.device), torch.zeros((2, m), device=u1.device)
            p = scn.bsdf_eval_pdf_sample(q, dev(d.astype(np.float32)), z1, z2)[1]
            return cc.true_pdf_scale(sc, mid, w, p.double().cpu().numpy(), d[:, 2] * np.sign(w[2]))
        return pdf_fn

    # (the lanes alternate between the two uv; the pdf is taken at the first: it may not depend on uv)
    for key, name in CASES:
        mid, k = ids[key], WI_NAMES.index(name)
        w = cc.WI[name]
        r = cc.sphere_chi2(None, device_pdf(mid, w, cc.UV["uv0"]), int(n_drawn[mid, k]), grid=GRID,
                           counts=counts[mid, k].reshape(GRID.n_theta, GRID.n_phi))
        r.update(n=int(n_drawn[mid, k]), valid=int(n_valid[mid, k]), delta=int(n_delta[mid, k]),
                 zero=int(n_zero[mid, k]))
        assert r.n > 10000
        cc.check_bsdf_case(r, sc.materials[mid], f"{key}-{name} n={n}", P_MIN)
