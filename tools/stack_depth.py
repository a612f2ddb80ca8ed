"""Stack depth of the closest-hit traversal on the bench's scene (CPU, the
oracle's visit order; tools/probes/stack_depth.cpp): which stack entries the
pushes of camera rays and of three diffuse bounces behind them write, and how
deep a ray's stack gets. Sizes the LDS part of k_trace_closest's stack
(DevScene::lds_entries / ring_lds_entries, DESIGN.md §7 "Prepared-ray ring"):
a push to entry e >= the LDS entries is a store to and a load from the global
spill area. Rays as in tools/top_visits.py: random film positions, then
cosine-distributed directions off the geometric normal of each hit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "mitsuba3-experiments_amd"), os.path.join(ROOT, "oracle"), HERE]
H = 64


def probe():
    out = os.path.join(ROOT, ".cache", "stack_depth.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "probes", "stack_depth.cpp"), "-o", out], check=True)
    fn = C.CDLL(out).stack_depth_hist
    fn.argtypes = [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 2 + [C.c_uint32, C.c_void_p]
    fn.restype = None
    return fn


def bounce(sc, rng, o, d, t, prim):
    """Cosine-distributed rays off the hits (t, prim) of rays (o, d)."""
    g = sc.tri_geom.reshape(-1, 3, 4)[prim]
    nrm = np.cross(g[:, 1, :3], g[:, 2, :3])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= -np.sign(np.sum(nrm * d, 1, keepdims=True))
    p = o + t[:, None] * d + nrm * 1e-3
    u1, u2 = rng.random(len(p)), rng.random(len(p))
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    a = np.where(np.abs(nrm[:, :1]) > 0.9, np.array([[0, 1, 0]]), np.array([[1, 0, 0]]))
    tt = np.cross(nrm, a)
    tt /= np.linalg.norm(tt, axis=1, keepdims=True)
    bb = np.cross(nrm, tt)
    dd = tt * (r * np.cos(phi))[:, None] + bb * (r * np.sin(phi))[:, None] + nrm * np.sqrt(1 - u1)[:, None]
    return p.astype(np.float32), dd.astype(np.float32)


def main(n=200_000):
    import binding as oracle
    from mtx import scene

    sc = scene.bedroom(cache_dir=os.path.join(ROOT, ".cache"))
    fn = probe()
    nodes = np.ascontiguousarray(sc.nodes, np.int32)
    geom = np.ascontiguousarray(sc.tri_geom, np.float32)
    rng = np.random.default_rng(0)
    cam = sc.camera
    pos = rng.random((n, 2)).astype(np.float32)
    tx, ty = np.float32(cam.tan_x), np.float32(cam.tan_y)
    dl = np.stack([(1 - 2 * pos[:, 0]) * tx, (1 - 2 * pos[:, 1]) * ty, np.ones(n, np.float32)], 1)
    dl /= np.linalg.norm(dl, axis=1, keepdims=True)
    M = np.stack([np.array(cam.axis_x), np.array(cam.axis_y), np.array(cam.axis_z)], 1).astype(np.float32)
    d = (dl @ M.T).astype(np.float32)
    o = np.tile(np.array(cam.origin, np.float32), (n, 1))
    print(f"scene: {sc.n_tris} triangles, {int(sc.n_nodes)} nodes; {n} camera rays", flush=True)
    for b in range(4):
        rays = np.zeros((len(o), 8), np.float32)
        rays[:, 0:3], rays[:, 4:7], rays[:, 3] = o, d, 3e38
        push, mx, visits = np.zeros(H, np.uint64), np.zeros(H, np.uint64), C.c_uint64(0)
        fn(nodes.ctypes.data, geom.ctypes.data, rays.ctypes.data, len(rays), push.ctypes.data, mx.ctypes.data, H,
           C.byref(visits))
        tot = float(push.sum())
        deep = {L: float(push[L:].sum()) for L in (7, 9, 12, 16, 20)}
        cmx = np.cumsum(mx) / mx.sum()
        print(f"bounce {b}: {len(rays)} rays, node visits/ray {visits.value / len(rays):.2f}, pushes/ray {tot / len(rays):.2f}; "
              "pushes to entry >= L per ray (share of pushes): "
              + ", ".join(f"L={L}: {deep[L] / len(rays):.4f} ({deep[L] / tot:.4%})" for L in deep)
              + "; rays whose stack stays within 7 / 9 / 12 / 16 entries: "
              + " / ".join(f"{cmx[L]:.4f}" for L in (7, 9, 12, 16))
              + f"; deepest {int(np.nonzero(mx)[0].max())}", flush=True)
        h, _ = oracle.trace(sc, rays)
        h = h.reshape(-1, 4)
        ok = h[:, 1] != 0xFFFFFFFF
        o, d = bounce(sc, rng, o[ok], d[ok], h[ok, 0].view(np.float32), h[ok, 1])


if __name__ == "__main__":
    main()
