"""Two integrators written in Python on mtx.blocks: the BSDF-only estimator
("integrator") and NEE + MIS variant B ("path_test"), restated from this
repository's own loops (oracle/oracle.cpp orc_simple, orc_path_mis) in the
blocks' vocabulary. tests/test_blocks_gpu.py holds them to the oracle and to
the fused sample() bit for bit; tools/blocks_probe.py times them.

A lane of the oracle that has stopped executes nothing. Here every lane runs
every block, so each update of a path's state that can reach its result is
masked with the mask the oracle's control flow implies; a stopped lane's
interaction is invalid (masked-off ray_intersect) and its later draws are
never read. Plain * and comparisons are torch operations (single IEEE
operations); fmaxf / fminf are torch.fmax / torch.fmin.
"""
import torch
from mtx import blocks


def _hmax(v):
    return torch.fmax(torch.fmax(v[0], v[1]), v[2])


def _roulette(f, eta, depth, rr_depth, sampler):
    """The stopping criterion both loops share: returns (f, keep_going)."""
    fmax = _hmax(f)
    rr_prob = torch.fmin(fmax * (eta * eta), fmax.new_tensor(0.95))
    rr_active = depth >= rr_depth
    rr_continue = sampler.next_1d() < rr_prob
    f = torch.where(rr_active, f * blocks.rcp(rr_prob), f)
    return f, (~rr_active | rr_continue) & (fmax != 0)


def simple(scn, sampler, o, d, max_depth=8, rr_depth=2):
    """BSDF sampling only, no emitter sampling: (L (3, N), valid (N,))."""
    n, dev = o.shape[1], o.device
    f = torch.ones((3, n), device=dev)
    L = torch.zeros((3, n), device=dev)
    eta = torch.ones(n, device=dev)
    depth = torch.zeros(n, dtype=torch.int32, device=dev)
    prev_bsdf_pdf = torch.ones(n, device=dev)
    active = torch.ones(n, dtype=torch.bool, device=dev)
    zero3 = torch.zeros((3, n), device=dev)
    maxt = None
    while bool(active.any()):
        si = scn.ray_intersect(o, d, maxt, active)
        le = torch.where(prev_bsdf_pdf > 0, scn.emitter_eval(si), zero3)
        L = torch.where(active, blocks.fma(f, le, L), L)
        active_next = active & (depth + 1 < max_depth) & si.valid
        s1, s2 = sampler.next_1d(), sampler.next_2d()
        _, _, bs, bsdf_weight = scn.bsdf_eval_pdf_sample(si, zero3, s1, s2, active_next)
        o, d, maxt = si.spawn_ray(si.to_world(bs.wo))
        f = f * bsdf_weight
        eta = eta * bs.eta
        prev_bsdf_pdf = bs.pdf
        depth = depth + si.valid.to(torch.int32)
        f, go = _roulette(f, eta, depth, rr_depth, sampler)
        active = active_next & go
    return L, depth != 0


def path_mis(scn, sampler, o, d, max_depth=8, rr_depth=2):
    """Emitter sampling + BSDF sampling with the power heuristic (variant B)."""
    n, dev = o.shape[1], o.device
    throughput = torch.ones((3, n), device=dev)
    result = torch.zeros((3, n), device=dev)
    eta = torch.ones(n, device=dev)
    depth = torch.zeros(n, dtype=torch.int32, device=dev)
    valid_ray = torch.full((n,), scn.has_environment, dtype=torch.bool, device=dev)
    prev_p = torch.zeros((3, n), device=dev)
    prev_bsdf_pdf = torch.ones(n, device=dev)
    prev_bsdf_delta = torch.ones(n, dtype=torch.bool, device=dev)
    active = torch.ones(n, dtype=torch.bool, device=dev)
    zero1, zero3 = torch.zeros(n, device=dev), torch.zeros((3, n), device=dev)
    maxt = None
    while bool(active.any()):
        si = scn.ray_intersect(o, d, maxt, active)
        # direct emission, weighted against the emitter-sampling pdf of the same direction
        em_pdf = torch.where(prev_bsdf_delta, zero1, scn.pdf_emitter_direction(prev_p, si))
        mis_bsdf = blocks.mis_weight(prev_bsdf_pdf, em_pdf, "b")
        le = torch.where(prev_bsdf_pdf > 0, scn.emitter_eval(si), zero3)
        result = torch.where(active, blocks.fma(throughput, le * mis_bsdf, result), result)
        active_next = active & (depth + 1 < max_depth) & si.valid
        # emitter sampling, visibility included
        active_em = active_next & ((scn.bsdf_flags(si) & blocks.BF_SMOOTH) != 0)
        ds, em_weight = scn.sample_emitter_direction(si, sampler.next_2d(), True, active_em)
        wo = si.to_local(ds.d)
        s1, s2 = sampler.next_1d(), sampler.next_2d()
        bsdf_val, bsdf_pdf, bs, bsdf_weight = scn.bsdf_eval_pdf_sample(si, wo, s1, s2)
        mi_em = blocks.mis_weight(ds.pdf, bsdf_pdf, "b")
        result = torch.where(active_em, blocks.fma(throughput, bsdf_val * em_weight * mi_em, result), result)
        # BSDF sampling
        o, d, maxt = si.spawn_ray(si.to_world(bs.wo))
        throughput = throughput * bsdf_weight
        eta = eta * bs.eta
        valid_ray = valid_ray | (active & si.valid & ((bs.sampled_type & blocks.BF_NULL) == 0))
        prev_p, prev_bsdf_pdf = si.p, bs.pdf
        prev_bsdf_delta = (bs.sampled_type & blocks.BF_DELTA) != 0
        depth = depth + si.valid.to(torch.int32)
        throughput, go = _roulette(throughput, eta, depth, rr_depth, sampler)
        active = active_next & go
    return torch.where(valid_ray, result, zero3), valid_ray
