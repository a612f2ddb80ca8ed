"""Deformations shared by the vertex-update tests (test_refit.py on the host,
test_refit_gpu.py on the device). Emitter shapes are never touched."""
import numpy as np

KINDS = ("translate", "sine", "collapse", "scale50")


def movable_shapes(scene):
    """Non-emitter shapes, largest triangle count first."""
    counts = np.bincount(scene.tri_shape, minlength=len(scene.shapes))
    ids = [i for i in range(len(scene.shapes)) if scene.shapes[i].emitter < 0 and counts[i] > 0]
    return sorted(ids, key=lambda i: (-int(counts[i]), i))


def shape_vertices(scene, shape):
    return np.unique(scene.tri_vidx.reshape(-1, 3)[scene.tri_shape == shape])


def emitter_vertices(scene):
    em = np.array([sh.emitter >= 0 for sh in scene.shapes], bool)
    return np.unique(scene.tri_vidx.reshape(-1, 3)[em[scene.tri_shape]])


def deform(scene, kind):
    """New (n_verts, 3) float32 positions for one of KINDS:
    translate: a rigid translation of one shape;
    sine:      a sinusoidal displacement (amplitude 0.05) of every vertex of a non-emitter shape;
    collapse:  one shape collapsed to a point (zero-extent boxes, the exponent floor);
    scale50:   one shape scaled x50 about its centroid (extent and exponents grow)."""
    v = scene.vpos.reshape(-1, 3).astype(np.float32).copy()
    shapes = movable_shapes(scene)
    pick = shapes[1 % len(shapes)]  # not the largest (the room itself on the bedroom)
    if kind == "translate":
        idx = shape_vertices(scene, pick)
        v[idx] += np.array([0.3, 0.1, -0.2], np.float32)
    elif kind == "sine":
        keep = emitter_vertices(scene)
        d = (0.05 * np.sin(7.0 * v[:, [1, 2, 0]].astype(np.float64) + np.array([0.3, 1.1, 2.3]))).astype(np.float32)
        d[keep] = 0
        v += d
    elif kind == "collapse":
        idx = shape_vertices(scene, shapes[2 % len(shapes)])
        v[idx] = v[idx].mean(0, dtype=np.float64).astype(np.float32)
    elif kind == "scale50":
        idx = shape_vertices(scene, shapes[3 % len(shapes)])
        c = v[idx].mean(0, dtype=np.float64)
        v[idx] = (c + 50.0 * (v[idx].astype(np.float64) - c)).astype(np.float32)
    else:
        raise ValueError(kind)
    return v
