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

Usage: python tools/blocks_probe.py [--log2n 22] [--reps 5] [--scenes small,full] [--out profiles/blocks_probe.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="small,full")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks_probe.json"))
    a = ap.parse_args()
    import torch
    from mtx import scene

    if not torch.cuda.is_available():
        raise SystemExit("blocks_probe: needs a GPU (no time is reported from a CPU)")
    doc = {"probe": "blocks", "hbm_peak_GBps": HBM_PEAK_GBS, "timing": "host clock around calls that end in a device "
           "synchronise; medians of --reps calls after warm-up", "scenes": []}
    for label in a.scenes.split(","):
        sc = scene.bedroom(width=64, height=36, scale=0.02, tex_res=64) if label == "small" else scene.bedroom()
        doc["scenes"].append(probe_scene(label, sc, 1 << a.log2n, a.reps))
        with open(a.out, "w") as f:  # after each scene: a later failure keeps what was measured
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
