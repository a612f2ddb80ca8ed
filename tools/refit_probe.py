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

``--section light`` (one JSON line, probe "moving_emitters"): the same update
on the bedroom with its largest mesh as one mesh light -- the light's vertices
move, so its tables are rebuilt -- against the same scene with that mesh as a
non-emitter, the two contexts alternating. ``--section fallback``: one
synthetic emitter that fails the exactness predicate (one triangle of area 1,
2^18 slivers of 2^-60), so its prefix is summed by one lane in entry order.
The per-pass kernel times are read from a kernel trace of these sections
(rocprofv3 --kernel-trace --stats: k_em_areas, k_em_scan, k_em_scan_ordered,
k_em_commit), which slows the host: the wall-clock figures come from a run
without it.
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


def light_spec(spec):
    """The bedroom with its largest proxy mesh as one mesh light; returns the
    spec and the shape's id."""
    from mtx import proxy

    spec = copy.deepcopy(spec)
    cands = [sd for sd in spec["shapes"] if sd["type"] != "rectangle" and "emitter" not in sd and sd.get("lfs_size")]
    sd = max(cands[1:], key=lambda x: proxy.budget_from_lfs(x.get("lfs_size"), 1.0))  # not the room itself
    sd["emitter"] = {"type": "area", "radiance": [3.0, 3.0, 3.0]}
    return spec, sd["id"]


def timed_pair(ctxs, xs, reps):
    """Median / min / max ms of update_vertices on each context, alternating
    between the contexts and between the two vertex sets."""
    import torch

    out = [[] for _ in ctxs]
    for i in range(reps + 1):
        for k, c in enumerate(ctxs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            c.update_vertices(xs[k][i % 2])
            if i:  # the first round warms up
                out[k].append((time.perf_counter() - t) * 1e3)
    return [{"median": round(statistics.median(o), 3), "min": round(min(o), 3), "max": round(max(o), 3)} for o in out]


def section_light(a):
    import torch

    from mtx import scene
    from mtx._lib import Context
    from mtx.integrators import _bind_scene

    base = scene.Scene.bedroom(scale=a.scale)
    spec, sid = light_spec(scene.load_bedroom_spec())
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lit = scene.Scene.bedroom(scale=a.scale, spec=spec)
    assert np.array_equal(base.vpos, lit.vpos)
    vA, vB = base.vpos.reshape(-1, 3).copy(), sine(base)  # sine(base): the light's mesh moves, the rectangles stay
    n_light = int(sum(e.mesh["count"] for e in lit.emitters if e.is_mesh))
    assert n_light and not np.array_equal(lit.with_vertices(vB, move_emitters=True).tables, lit.tables)
    ctxs = [Context(0), Context(0)]
    _bind_scene(ctxs[0], base)
    _bind_scene(ctxs[1], lit)
    dev = [torch.as_tensor(vB, device="cuda"), torch.as_tensor(vA, device="cuda")]
    res = timed_pair(ctxs, [dev, dev], a.reps)
    print(json.dumps({"probe": "moving_emitters", "section": "light", "scene": f"bedroom-proxy scale={a.scale:g}",
                      "n_tris": int(base.n_tris), "light_shape": sid, "light_triangles": n_light, "reps": a.reps,
                      "update_ms_light_as_non_emitter": res[0], "update_ms_mesh_light": res[1],
                      "table_passes_ms_by_difference": round(res[1]["median"] - res[0]["median"], 3)}), flush=True)
    for c in ctxs:
        c.close()


def section_fallback(a):
    import tempfile

    import torch

    from mtx._lib import Context
    from mtx.integrators import _bind_scene
    from mtx.mitsuba_dict import scene_from_dict

    side = 512
    j = np.arange(side * side)
    p0 = np.stack([(j % side) * 2.0 ** -26, (j // side) * 2.0 ** -26, np.zeros(len(j))], 1)
    tri = np.stack([p0, p0 + [2.0 ** -29, 0, 0], p0 + [0, 2.0 ** -30, 0]], 1)
    tri = np.concatenate([[[[-4.0, 0, 0], [-2.0, 0, 0], [-4.0, 1.0, 0]]], tri]).reshape(-1, 3)
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "slivers.obj"), "w") as fh:
        fh.write("".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in tri))
        fh.write("".join("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(len(tri) // 3)))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = scene_from_dict({
            "type": "scene",
            "sensor": {"type": "perspective", "fov": 60.0, "to_world": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 6], [0, 0, 0, 1]],
                       "film": {"type": "hdrfilm", "width": 16, "height": 16}},
            "grey": {"type": "diffuse", "reflectance": {"type": "rgb", "value": 0.5}},
            "light": {"type": "obj", "filename": "slivers.obj", "bsdf": {"type": "ref", "id": "grey"},
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [1.0, 1.0, 1.0]}}}}, base_dir=d)
    pmf = s.tables[s.emitters[0].mesh["offset"]:][: s.emitters[0].mesh["count"]]
    n = len(pmf)
    M, m = int(np.floor(np.log2(pmf.max()))), int(np.floor(np.log2(pmf[pmf > 0].min()))) - 23
    assert M + 1 + int(np.ceil(np.log2(n))) - m > 53  # fails the exactness predicate: the ordered fallback
    vA = s.vpos.reshape(-1, 3).copy()
    vB = vA * np.array([1, -1, 1], np.float32)
    ctx = Context(0)
    _bind_scene(ctx, s)
    dev = [torch.as_tensor(vB, device="cuda"), torch.as_tensor(vA, device="cuda")]
    res = timed_pair([ctx], [dev], a.reps)[0]
    ctx.update_vertices(vA)
    ok = np.array_equal(ctx.scene_read("tables"), s.tables[: s.n_tables])
    print(json.dumps({"probe": "moving_emitters", "section": "fallback", "entries": n, "reps": a.reps,
                      "update_ms_whole_call": res, "tables_equal_host": bool(ok),
                      "entries_per_s_whole_call": round(n / (res["median"] / 1e3))}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=["refit", "light", "fallback"], default="refit")
    ap.add_argument("--scale", type=float, default=1.0, help="bedroom triangle budget (1.0 = the benchmark scene)")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--spp", type=int, default=16, help="samples per pixel of the stale-topology renders")
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    if a.section != "refit":
        return {"light": section_light, "fallback": section_fallback}[a.section](a)

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
