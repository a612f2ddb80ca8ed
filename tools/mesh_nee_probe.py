"""Cost of next-event estimation towards a mesh light against a rectangle's
(not a bench.py workload): one JSON line.

A closed two-sided diffuse box [-2, 2]^3, camera inside, lit by one emitter on
the wall x = -1.75 covering y, z in [-1, 1]: a `rectangle`, or an emitting
`obj` of that extent tessellated into a jittered grid of 2 n^2 triangles
(n = 10: 200 triangles, 8 bisection steps; n = 100: 20,000, 15 steps). path_test
at 1280x720; per scene the median over `--steps` renders of the shade kernels'
time (HIP events, stats=True) and of the whole step. The shade time carries
the difference: the cdf search, the table and vertex gathers."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mitsuba3-experiments_amd"))


def write_patch(path, n, seed=7):
    rng = np.random.default_rng(seed)
    m = n + 1
    step = 2.0 / n
    with open(path, "w") as fh:
        for i in range(m):
            for j in range(m):
                jy, jz = rng.uniform(-0.3, 0.3, 2) * step * (0 < i < n, 0 < j < n)
                fh.write("v -1.75 %r %r\n" % (float(-1 + i * step + jy), float(-1 + j * step + jz)))
        for i in range(n):
            for j in range(n):
                a, b, c, d = i * m + j + 1, (i + 1) * m + j + 1, (i + 1) * m + j + 2, i * m + j + 2
                fh.write("f %d %d %d\nf %d %d %d\n" % (a, b, c, a, c, d))


def scene_dict(light, width, height):
    M = np.eye(4)
    M[:3, :3] = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]  # unit square's +z -> +x; columns: x -> -z, y -> y
    M[:3, 3] = [-1.75, 0, 0]
    cam = np.eye(4)
    cam[:3, 0], cam[:3, 1], cam[:3, 2], cam[:3, 3] = [-1, 0, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1.9]
    d = {"type": "scene",
         "sensor": {"type": "perspective", "fov": 70.0, "to_world": cam,
                    "film": {"type": "hdrfilm", "width": width, "height": height}},
         "box": {"type": "cube", "to_world": np.diag([2.0, 2.0, 2.0, 1.0]),
                 "bsdf": {"type": "twosided", "nested": {"type": "diffuse", "reflectance": {"type": "rgb", "value": 0.6}}}},
         "light": dict(light, emitter={"type": "area", "radiance": {"type": "rgb", "value": [4.0, 4.0, 4.0]}})}
    if light["type"] == "rectangle":
        d["light"]["to_world"] = M
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    a = ap.parse_args()
    from mtx import load_dict
    from mtx.mitsuba_dict import scene_from_dict

    integ = load_dict({"type": "path_test", "max_depth": 8})
    out = {"workload": "mesh_nee_probe", "integrator": "path_test", "film": [a.width, a.height], "spp": a.spp,
           "steps": a.steps, "scenes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        lights = {"rectangle": {"type": "rectangle"}}
        for n in (10, 100):
            write_patch(os.path.join(tmp, f"patch{n}.obj"), n)
            lights[f"mesh_{2 * n * n}"] = {"type": "obj", "filename": f"patch{n}.obj"}
        for name, light in lights.items():
            sc = scene_from_dict(scene_dict(light, a.width, a.height), base_dir=tmp)
            integ.render_film(sc, seed=0, spp=a.spp)  # warm-up, upload
            shade, total, mean = [], [], 0.0
            for k in range(a.steps):
                film, st = integ.render_film(sc, seed=1 + k, spp=a.spp, stats=True)
                shade.append(st["shade_ms"])
                total.append(st["trace_ms"] + st["shadow_ms"] + st["shade_ms"] + st["other_ms"])
                mean = float(film[1:-1, 1:-1, :3].sum() / max(film[1:-1, 1:-1, 3].sum(), 1e-30))
            out["scenes"][name] = {"shade_ms": round(statistics.median(shade), 3), "step_ms": round(statistics.median(total), 3),
                                   "shade_ms_all": [round(x, 3) for x in shade], "n_tris": int(sc.n_tris),
                                   "image_mean": round(mean, 5)}
    r = out["scenes"]["rectangle"]["shade_ms"]
    for k, v in out["scenes"].items():
        v["shade_vs_rectangle"] = round(v["shade_ms"] / r, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
