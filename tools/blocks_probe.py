"""Building-blocks probe (not a bench.py workload, not a test): one JSON document with

* per block at N lanes (default 2^22) on the small bedroom proxy and on the
  full bedroom: the median wall time of one call of the facade (the call is
  complete on return: it synchronises torch's stream, launches on the
  context's stream and drains it), the bytes the call must move by its plane
  layout (inputs read once, outputs written once; scene data not counted) and
  the resulting share of the HBM peak. The streaming blocks (sampler, spawn,
  math) stand beside torch's own elementwise kernels on the same tensors,
  timed the same way in the same run;
* the NEE + MIS loop composed in Python on the blocks
  (tests/blocks_integrators.py path_mis) against the fused sample() on the
  same rays, in Mpaths/s: the price of one launch per block and of state
  that passes through HBM between blocks.

With ``--only film`` the document (profiles/blocks_film_probe.json) holds
instead: ``sensor.sample_ray``, ``Film.put`` on the pixel-major and on the
general path and ``Film.raw`` at N lanes beside torch's ``copy_`` of the same
contribution planes, and a whole ``render_film`` composed on the blocks
against the fused integrator's on the same frame.

With ``--only light`` (profiles/blocks_light_probe.json): the two light-path
calls, ``scene.sample_emitter_ray`` and ``sensor.sample_direction`` with and
without its visibility test, at N lanes beside torch's ``copy_`` of the same
planes, and a whole ``ptracer`` frame beside the composed ``path_test`` frame
of the same film and sample count. The frame's scene is the Cornell box of
tests/blocks_light_cases.py: the bedroom proxy holds a roughdielectric, which
the particle tracer refuses.

With ``--only bdpt`` (profiles/blocks_bdpt_probe.json; ``--scenes`` is not
read): for the 32 x 32 and the 256 x 256 Cornell box, one pass of the ``bdpt``
integrator split into recording the two subpaths and the connect kernel, the
kernel's strategies per second, and the RMSE of ``bdpt`` and of ``path_test``
against a long ``path_test`` render at equal wall time on a Cornell variant
whose light faces the ceiling (all of the room is lit indirectly).

Usage: python tools/blocks_probe.py [--only blocks|film|light|bdpt] [--log2n 22] [--reps 5] [--scenes small,full] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mitsuba3-experiments_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # as bench.py: 8.0 TB/s spec


def camera_rays(scene, n, seed):
    """Camera rays through random film positions, (3, n) origin and direction planes."""
    rng = np.random.default_rng(seed)
    cam = scene.camera
    pos = rng.random((n, 2)).astype(np.float32)
    dl = np.stack([(1 - 2 * pos[:, 0]) * np.float32(cam.tan_x), (1 - 2 * pos[:, 1]) * np.float32(cam.tan_y),
                   np.ones(n, np.float32)], 1)
    dl /= np.linalg.norm(dl, axis=1, keepdims=True)
    M = np.stack([np.array(cam.axis_x), np.array(cam.axis_y), np.array(cam.axis_z)], 1).astype(np.float32)
    d = (dl @ M.T).astype(np.float32)
    o = np.tile(np.array(cam.origin, np.float32), (n, 1))
    return np.ascontiguousarray(o.T), np.ascontiguousarray(d.T)


def timed(fn, reps, warmup=2):
    import torch

    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def row(name, t, n, bytes_per_lane):
    gbs = bytes_per_lane * n / (t["median_ms"] * 1e-3) / 1e9
    return {"block": name, **t, "bytes_per_lane": bytes_per_lane, "GBps": round(gbs, 1),
            "hbm_share": round(gbs / HBM_PEAK_GBS, 4)}


def probe_scene(label, sc, n, reps):
    import blocks_integrators as bi
    import torch
    from mtx import IndependentSampler, blocks, load_dict

    scn = blocks.Scene(sc)
    o, d = (torch.from_numpy(a).cuda() for a in camera_rays(sc, n, 1))
    lanes = torch.arange(n, dtype=torch.int32, device="cuda")
    smp = blocks.Sampler(3, lanes, skip=2)
    si = scn.ray_intersect(o, d)
    u2, u1 = smp.next_2d(), smp.next_1d()
    ds, _ = scn.sample_emitter_direction(si, u2)
    wo = si.to_local(ds.d)
    a3, b3, c3 = si.p, si.wi, si.n
    out3 = torch.empty_like(a3)
    rows = [
        row("torch copy (3, N)", timed(lambda: out3.copy_(a3), reps), n, 24),
        row("torch add (3, N)", timed(lambda: torch.add(a3, b3, out=out3), reps), n, 36),
        row("torch a * b + c (3, N), two kernels", timed(lambda: a3 * b3 + c3, reps), n, 72),
        row("sampler.next_1d", timed(smp.next_1d, reps), n, 36),
        row("sampler.next_2d", timed(smp.next_2d, reps), n, 40),
        row("si.spawn_ray", timed(lambda: si.spawn_ray(b3), reps), n, 64),
        row("blocks.fma (3, N)", timed(lambda: blocks.fma(a3, b3, c3), reps), n, 48),
        row("blocks.dot", timed(lambda: blocks.dot(a3, b3), reps), n, 28),
        row("si.to_local", timed(lambda: si.to_local(b3), reps), n, 36),
        row("blocks.mis_weight", timed(lambda: blocks.mis_weight(u1, si.t), reps), n, 12),
        row("scene.ray_intersect", timed(lambda: scn.ray_intersect(o, d), reps), n, 104),
        row("scene.ray_test", timed(lambda: scn.ray_test(o, d, si.t), reps), n, 29),
        row("scene.sample_emitter_direction (visibility)", timed(lambda: scn.sample_emitter_direction(si, u2), reps),
            n, 92),
        row("scene.sample_emitter_direction (no visibility)",
            timed(lambda: scn.sample_emitter_direction(si, u2, False), reps), n, 80),
        row("scene.pdf_emitter_direction (4 launches + 3 torch ops)",
            timed(lambda: scn.pdf_emitter_direction(a3, si), reps), n, 0),
        row("scene.emitter_eval", timed(lambda: scn.emitter_eval(si), reps), n, 28),
        row("scene.bsdf_eval_pdf_sample", timed(lambda: scn.bsdf_eval_pdf_sample(si, wo, u1, u2), reps), n, 100),
        row("scene.bsdf_flags", timed(lambda: scn.bsdf_flags(si), reps), n, 8),
    ]
    integ = load_dict({"type": "path_test", "max_depth": 8, "rr_depth": 2})
    hl = np.arange(n, dtype=np.uint32)
    fused = timed(lambda: integ.sample(sc, IndependentSampler(3, hl, skip=2), (o, d)), max(3, reps // 2), 1)
    comp = timed(lambda: bi.path_mis(scn, blocks.Sampler(3, lanes, skip=2), o, d, 8, 2), max(3, reps // 2), 1)
    L, v = bi.path_mis(scn, blocks.Sampler(3, lanes, skip=2), o, d, 8, 2)
    Lf, vf, _ = integ.sample(sc, IndependentSampler(3, hl, skip=2), (o, d))
    same = bool(torch.equal(L.T.contiguous(), Lf) and torch.equal(v, vf))
    mp = lambda t: round(n / (t["median_ms"] * 1e-3) / 1e6, 2)  # noqa: E731
    return {"scene": label, "n_tris": int(sc.n_tris), "lanes": n, "blocks": rows,
            "path_mis": {"fused_sample": {**fused, "Mpaths_per_s": mp(fused)},
                         "composed_on_blocks": {**comp, "Mpaths_per_s": mp(comp)},
                         "fused_over_composed": round(comp["median_ms"] / fused["median_ms"], 2),
                         "results_bit_identical": same}}


FILM_SPP = 8  # samples per pixel of the film probe: one per slot, every slot's planes move


def probe_film(label, sc, n, reps):
    """Sensor rays, Film.put on both source paths and Film.raw at n lanes (a
    film of n / FILM_SPP pixels, pixel-major jittered positions) beside torch's
    copy_ of the same contribution planes, and a whole render_film composed on
    the blocks against the fused integrator's on the same frame."""
    import blocks_integrators as bi
    import torch
    from mtx import blocks, load_dict

    n_px = n // FILM_SPP
    W = 1 << ((n_px.bit_length() - 1 + 1) // 2)
    H = n_px // W
    scf = sc.with_film(W, H)
    sens = blocks.Sensor(scf)
    pix = torch.arange(n_px, device="cuda").repeat_interleave(FILM_SPP)
    g = torch.Generator(device="cuda").manual_seed(5)
    u = torch.rand((2, n), device="cuda", generator=g) * 0.999
    pos = torch.stack([(pix % W).float() + u[0], (pix // W).float() + u[1]])
    L = torch.rand((3, n), device="cuda", generator=g)
    rows = [row("sensor.sample_ray", timed(lambda: sens.sample_ray(pos), reps), n, 36)]
    same_planes = True
    for rf in ("tent", "gaussian"):
        film = blocks.Film(W, 0, H, rf)
        other = torch.empty_like(film.planes)
        plane_bytes = film.planes.numel() * 4
        per_lane = 2 * plane_bytes // n  # every slot's accumulators are loaded and stored once
        rows += [
            row(f"torch copy_ of the planes ({rf})", timed(lambda: other.copy_(film.planes), reps), n, per_lane),
            row(f"film.put pixel-major ({rf}; claim pass + staged put)",
                timed(lambda: film.put(pos, L, pixel_major_spp=FILM_SPP), reps), n, per_lane + 28),
            row(f"film.put general ({rf}; keys + group-by + put)", timed(lambda: film.put(pos, L), reps), n,
                per_lane + 28),
            row(f"film.raw ({rf})", timed(film.raw, reps), n,
                (plane_bytes + 16 * (W + 2 * film.border) * (H + 2 * film.border)) // n),
        ]
        a, b = blocks.Film(W, 0, H, rf), blocks.Film(W, 0, H, rf)
        a.put(pos, L)
        b.put(pos, L, pixel_major_spp=FILM_SPP)
        same_planes = same_planes and bool(torch.equal(a.planes, b.planes))
        del film, other, a, b

    class PathMis(blocks.SamplingIntegrator):
        def sample(self, scene, sampler, ray, medium=None, active=None):
            Lr, valid = bi.path_mis(scene, sampler, ray.o, ray.d, 8, 2)
            return Lr, valid, []

    fused_i = load_dict({"type": "path_test", "max_depth": 8, "rr_depth": 2})
    out = torch.empty((H + 2, W + 2, 4), device="cuda")
    k = max(3, reps // 2)
    fused = timed(lambda: fused_i.render_film(scf, seed=1, spp=FILM_SPP, out=out), k, 1)
    comp = timed(lambda: PathMis().render_film(scf, seed=1, spp=FILM_SPP), k, 1)
    same = bool(torch.equal(PathMis().render_film(scf, seed=1, spp=FILM_SPP),
                            fused_i.render_film(scf, seed=1, spp=FILM_SPP, out=out)))
    return {"scene": label, "n_tris": int(sc.n_tris), "lanes": n, "film": [W, H], "spp": FILM_SPP, "blocks": rows,
            "both_paths_same_planes": same_planes,
            "render_film": {"fused": fused, "composed_on_blocks": comp,
                            "fused_over_composed": round(comp["median_ms"] / fused["median_ms"], 2),
                            "films_bit_identical": same}}


def probe_light(label, sc, n, reps):
    """The two light-path calls at n lanes on `sc`, and a ptracer frame beside
    the composed path_test frame on the Cornell box."""
    import blocks_integrators as bi
    import torch
    from mtx import blocks, load_dict
    from mtx.mitsuba_dict import scene_from_dict
    from blocks_light_cases import cornell_dict

    scn, sens = blocks.Scene(sc), blocks.Sensor(sc)
    g = torch.Generator(device="cuda").manual_seed(7)
    u_pos, u_dir = torch.rand((2, n), device="cuda", generator=g), torch.rand((2, n), device="cuda", generator=g)
    ray, _, _ = scn.sample_emitter_ray(u_pos, u_dir)
    si = scn.ray_intersect(ray.o, ray.d, ray.maxt)  # first vertices of light paths: the points a connection starts at
    planes17, other17 = torch.empty((17, n), device="cuda"), torch.empty((17, n), device="cuda")
    planes7, other7 = torch.empty((7, n), device="cuda"), torch.empty((7, n), device="cuda")
    rows = [
        row("torch copy_ of 17 planes", timed(lambda: other17.copy_(planes17), reps), n, 136),
        row("scene.sample_emitter_ray", timed(lambda: scn.sample_emitter_ray(u_pos, u_dir), reps), n, 16 + 68),
        row("torch copy_ of 7 planes", timed(lambda: other7.copy_(planes7), reps), n, 56),
        row("sensor.sample_direction (no visibility)", timed(lambda: sens.sample_direction(si.p, si.n, False), reps),
            n, 12 + 29),
        row("sensor.sample_direction (visibility)", timed(lambda: sens.sample_direction(si.p, si.n, True), reps), n,
            24 + 29),
    ]
    side = 1 << ((n // FILM_SPP).bit_length() - 1) // 2
    box = scene_from_dict(cornell_dict(side, side))

    class PathMis(blocks.SamplingIntegrator):
        def sample(self, scene, sampler, ray, medium=None, active=None):
            Lr, valid = bi.path_mis(scene, sampler, ray.o, ray.d, 8, 2)
            return Lr, valid, []

    k = max(3, reps // 2)
    pt = load_dict({"type": "ptracer", "max_depth": 8, "rr_depth": 2})
    ptracer = timed(lambda: pt.render_film(box, seed=1, spp=FILM_SPP), k, 1)
    comp = timed(lambda: PathMis().render_film(box, seed=1, spp=FILM_SPP, rfilter="box"), k, 1)
    fused_i = load_dict({"type": "path_test", "max_depth": 8, "rr_depth": 2})
    fused = timed(lambda: fused_i.render_film(box, seed=1, spp=FILM_SPP, rfilter="box"), k, 1)
    paths = side * side * FILM_SPP
    mp = lambda t: round(paths / (t["median_ms"] * 1e-3) / 1e6, 2)  # noqa: E731
    return {"scene": label, "n_tris": int(sc.n_tris), "lanes": n, "blocks": rows,
            "frame": {"scene": "cornell_box", "film": [side, side], "spp": FILM_SPP, "max_depth": 8, "rr_depth": 2,
                      "ptracer": {**ptracer, "Mpaths_per_s": mp(ptracer)},
                      "path_test_composed_on_blocks": {**comp, "Mpaths_per_s": mp(comp)},
                      "path_test_fused": {**fused, "Mpaths_per_s": mp(fused)},
                      "ptracer_over_composed": round(ptracer["median_ms"] / comp["median_ms"], 2)}}


def probe_bdpt(side, reps, max_depth=8, spp=FILM_SPP):
    """One bdpt pass on the side x side Cornell box, split; and bdpt against
    path_test at equal wall time on the variant whose light faces the ceiling."""
    import copy

    import blocks_light_cases as blc
    import torch
    from mtx import blocks, develop, load_dict
    from mtx.mitsuba_dict import scene_from_dict

    box = scene_from_dict(blc.cornell_dict(side, side))
    integ = load_dict({"type": "bdpt", "max_depth": max_depth})
    sens = blocks.Sensor(box)
    scn = blocks.Scene(sens.scene, sens.ctx.device)
    n = side * side * spp
    lanes = torch.arange(n, dtype=torch.int32, device="cuda")
    pix = torch.arange(side * side, device="cuda").repeat_interleave(spp)
    state = {}

    def record():
        sampler = blocks.Sampler(1, lanes)
        u = sampler.next_2d()
        pos = torch.stack([(pix % side).float() + u[0], (pix // side).float() + u[1]])
        cam = blocks.PathVertices(pos.device, max_depth + 1, n)
        lit = blocks.PathVertices(pos.device, max_depth + 1, n)
        integ.record_camera(scn, sampler, sens.sample_ray(pos), cam)
        integ.record_light(scn, sampler, lit)
        state["stores"] = (cam, lit)

    k = max(3, reps // 2)
    rec = timed(record, k, 1)
    cam, lit = state["stores"]
    con = timed(lambda: blocks.connect_subpaths(scn, cam, lit, max_depth), reps)
    con_free = timed(lambda: blocks.connect_subpaths(scn, cam, lit, max_depth, test_visibility=False), reps)
    whole = timed(lambda: integ.render_film(box, seed=1, spp=spp, rfilter="box"), k, 1)
    lz, ly = cam.len.long(), lit.len.long()
    strategies = 0
    for t in range(2, max_depth + 2):
        strategies += int(((lz >= t) * (torch.clamp(ly, max=max_depth + 1 - t) + 1)).sum())
    # equal wall time, on the variant whose light faces the ceiling
    d = copy.deepcopy(blc.cornell_dict(side, side))
    d["light"]["to_world"] = (blc.translate([0.0, 0.8, 0.01]) @ blc.rotate([1, 0, 0], -90)
                              @ blc.scale([0.23, 0.19, 0.19]))
    up = scene_from_dict(d)
    fused = load_dict({"type": "path_test", "max_depth": max_depth, "rr_depth": max_depth + 1})
    spp_b = 16
    t_b = timed(lambda: integ.render_film(up, seed=1, spp=spp_b, rfilter="box"), 3, 1)
    t_p = timed(lambda: fused.render_film(up, seed=1, spp=256, rfilter="box"), 3, 1)
    spp_p = max(1, int(round(256 * t_b["median_ms"] / t_p["median_ms"])))
    t_eq = timed(lambda: fused.render_film(up, seed=1, spp=spp_p, rfilter="box"), 3, 1)
    ref_spp = 16384 if side <= 64 else 2048
    ref = np.asarray(develop(fused.render_film(up, seed=999, spp=ref_spp, rfilter="box"), 0), np.float64)

    def rmse(img):
        return float(np.sqrt(((np.asarray(img, np.float64) - ref) ** 2).mean()))

    e_b = [rmse(develop(integ.render_film(up, seed=10 + i, spp=spp_b, rfilter="box").cpu().numpy(), 0))
           for i in range(4)]
    e_p = [rmse(develop(fused.render_film(up, seed=10 + i, spp=spp_p, rfilter="box"), 0)) for i in range(4)]
    return {"scene": "cornell_box", "film": [side, side], "spp": spp, "lanes": n, "max_depth": max_depth,
            "pass": {"record_ms": rec, "connect_ms": con, "connect_without_visibility_ms": con_free,
                     "render_film_ms": whole},
            "strategies_per_pass": strategies,
            "strategies_per_s": round(strategies / (con["median_ms"] * 1e-3), 1),
            "equal_time_light_faces_ceiling": {
                "reference": {"integrator": "path_test", "spp": ref_spp, "mean": float(ref.mean())},
                "bdpt": {"spp": spp_b, **t_b, "rmse": [round(e, 5) for e in e_b],
                         "rmse_mean": round(float(np.mean(e_b)), 5)},
                "path_test": {"spp": spp_p, **t_eq, "rmse": [round(e, 5) for e in e_p],
                              "rmse_mean": round(float(np.mean(e_p)), 5)}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="small,full")
    ap.add_argument("--only", default="blocks", choices=["blocks", "film", "light", "bdpt"],
                    help="blocks: the per-block rows and the composed sample(); film: sensor rays, Film.put / raw "
                         "and the composed render_film (default --out: profiles/blocks_film_probe.json); light: "
                         "sample_emitter_ray, sample_direction and a ptracer frame (profiles/blocks_light_probe.json); "
                         "bdpt: a bdpt pass split into recording and connecting, and bdpt against path_test at equal "
                         "time (profiles/blocks_bdpt_probe.json)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", {"blocks": "blocks_probe.json", "film": "blocks_film_probe.json",
                                                "light": "blocks_light_probe.json",
                                                "bdpt": "blocks_bdpt_probe.json"}[a.only])
    import torch
    from mtx import scene

    if not torch.cuda.is_available():
        raise SystemExit("blocks_probe: needs a GPU (no time is reported from a CPU)")
    doc = {"probe": {"blocks": "blocks", "film": "blocks film", "light": "blocks light", "bdpt": "blocks bdpt"}[a.only],
           "hbm_peak_GBps": HBM_PEAK_GBS,
           "timing": "host clock around calls that end in a device "
           "synchronise; medians of --reps calls after warm-up", "scenes": []}
    if a.only == "bdpt":
        for side in (32, 256):
            doc["scenes"].append(probe_bdpt(side, a.reps))
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        print(json.dumps(doc))
        return
    for label in a.scenes.split(","):
        sc = scene.bedroom(width=64, height=36, scale=0.02, tex_res=64) if label == "small" else scene.bedroom()
        probe = {"blocks": probe_scene, "film": probe_film, "light": probe_light}[a.only]
        doc["scenes"].append(probe(label, sc, 1 << a.log2n, a.reps))
        with open(a.out, "w") as f:  # after each scene: a later failure keeps what was measured
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
