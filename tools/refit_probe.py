"""Vertex-update probe on the full bedroom (not a bench.py workload): one JSON
line with

* the median time of mtx_scene_update_vertices from a device tensor and from
  host numpy (wall clock of the call, which is complete on return);
* the host refit (Scene.with_vertices);
* the only route before vertex updates: rebuild both trees from the new
  vertices and upload the scene again;
* the bytes the device path moves by its byte model, against the HBM peak;
* the cost of a stale topology: closest-hit and shadow trace ms per step on
  the refit trees against trees built fresh from the same vertices.

The deformation is a sinusoidal displacement (amplitude 0.05) of every vertex
that is not an emitter's; the update alternates between it and the original.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mitsuba3-experiments_amd"))

HBM_PEAK_GBS = 8000.0  # as bench.py: 8.0 TB/s spec


def sine(scene):
    v = scene.vpos.reshape(-1, 3).astype(np.float32).copy()
    em = np.array([sh.emitter >= 0 for sh in scene.shapes], bool)
    keep = np.unique(scene.tri_vidx.reshape(-1, 3)[em[scene.tri_shape]])
    d = (0.05 * np.sin(7.0 * v[:, [1, 2, 0]].astype(np.float64) + np.array([0.3, 1.1, 2.3]))).astype(np.float32)
    d[keep] = 0
    return v + d


def byte_model(s, normals: bool) -> int:
    """Bytes the device passes read and write (refit.hip), every array once per pass."""
    nt, nv, n4, n8 = int(s.n_tris), len(s.vpos.reshape(-1, 3)), int(s.n_nodes), int(s.n_occ_nodes)
    per_vert = 12 + 24 * (2 if normals else 1)            # box / finite scan; copy into the scene's vpos (vnormal)
    per_tri = (12 + 36 + 4)                               # pre-pass: indices, gathered vertices, shape
    per_tri += 12 + 36 + 4 + 36 + 36 + 24 + (72 if normals else 0)  # triangle pass: record, shading rows, box
    per_tri += 4 + 36 + 36 + 24                           # occlusion gather: perm, record in, record out, box
    per_tri += 24 + 24                                    # leaf boxes read by the two trees' level passes
    per_n4 = 64 + 40 + 24 + 24                            # node in, words out, own box out, read by the parent
    per_n8 = 80 + 64 + 24 + 24
    return nv * per_vert + nt * per_tri + n4 * per_n4 + n8 * per_n8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="bedroom triangle budget (1.0 = the benchmark scene)")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--spp", type=int, default=16, help="samples per pixel of the stale-topology renders")
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()

    import torch

    from mtx import PathIntegrator, scene
    from mtx._lib import Context
    from mtx.integrators import _bind_scene

    def note(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    note("building the scene")
    s = scene.Scene.bedroom(scale=a.scale)
    vA, vB = s.vpos.reshape(-1, 3).copy(), sine(s)

    t0 = time.perf_counter()
    sB = s.with_vertices(vB)
    host_refit_s = time.perf_counter() - t0
    note(f"host refit {host_refit_s:.3f} s; rebuilding from the new vertices")

    # the route without vertex updates: build again, upload again
    fresh = copy.copy(s)
    fresh.vpos = vB.reshape(s.vpos.shape).copy()
    t0 = time.perf_counter()
    fresh._build_bvh(s.tri_vidx.reshape(-1, 3), s.tri_shape)
    rebuild_s = time.perf_counter() - t0
    ctx_f = Context(0)
    t0 = time.perf_counter()
    _bind_scene(ctx_f, fresh)
    upload_s = time.perf_counter() - t0
    note(f"rebuild {rebuild_s:.3f} s, upload {upload_s:.3f} s; timing the updates")

    ctx = Context(0)
    _bind_scene(ctx, s)
    dA, dB = torch.as_tensor(vA, device="cuda"), torch.as_tensor(vB, device="cuda")

    def timed(x):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ctx.update_vertices(x)
        return (time.perf_counter() - t) * 1e3

    timed(dB)  # the first update allocates the scratch
    dev = [timed(dA if i % 2 == 0 else dB) for i in range(a.reps)]
    host = [timed(vA if i % 2 == 0 else vB) for i in range(a.reps)]

    # stale topology: the refit trees against fresh trees over the same vertices
    integ = PathIntegrator({"max_depth": 8, "rr_depth": 2})

    def trace_ms(c, sc):
        integ.render_film(sc, seed=99, spp=a.spp, ctx=c)
        acc = {"trace_ms": 0.0, "shadow_ms": 0.0}
        for i in range(a.steps):
            st = integ.render_film(sc, seed=i, spp=a.spp, ctx=c, stats=True)[1]
            for k in acc:
                acc[k] += st[k] / a.steps
        return {k: round(x, 3) for k, x in acc.items()}

    refit_trace = trace_ms(ctx, sB)  # the host refit's nodes: the same words the device refit leaves
    fresh_trace = trace_ms(ctx_f, fresh)
    nbytes = byte_model(s, normals=False)
    med = statistics.median(dev)
    out = {
        "probe": "refit", "scene": f"bedroom-proxy scale={a.scale:g}", "n_tris": int(s.n_tris),
        "n_verts": len(vA), "n_nodes": int(s.n_nodes), "n_occ_nodes": int(s.n_occ_nodes),
        "levels": [int(s.bvh_depth), int(s.occ_depth)], "reps": a.reps,
        "update_device_tensor_ms": {"median": round(med, 3), "min": round(min(dev), 3), "max": round(max(dev), 3)},
        "update_host_numpy_ms": {"median": round(statistics.median(host), 3), "min": round(min(host), 3),
                                 "max": round(max(host), 3)},
        "host_with_vertices_s": round(host_refit_s, 3),
        "rebuild_s": round(rebuild_s, 3), "upload_s": round(upload_s, 3),
        "rebuild_plus_upload_s": round(rebuild_s + upload_s, 3),
        "model_bytes": nbytes, "model_floor_ms_at_hbm_peak": round(nbytes / (HBM_PEAK_GBS * 1e9) * 1e3, 4),
        "model_GBps_at_median": round(nbytes / (med / 1e3) / 1e9, 1), "hbm_peak_GBps": HBM_PEAK_GBS,
        "stale_topology": {"deformation": "sine 0.05", "spp": a.spp, "steps": a.steps, "refit_trees": refit_trace,
                           "fresh_trees": fresh_trace},
    }
    print(json.dumps(out), flush=True)
    ctx.close()
    ctx_f.close()


if __name__ == "__main__":
    main()
