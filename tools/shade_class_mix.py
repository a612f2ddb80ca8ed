"""What the waves of the mixed shade loop hold (diagnostic): runs one headline
render (path-mis, bedroom 1280x720, spp 256) with the MTX_DIAG_CLASSES
library variant (`make -C mitsuba3-experiments_amd/csrc variant NAME=diagcls
DEFS=-DMTX_DIAG_CLASSES=1`) and MTX_SHADE_CLASSES=0, and prints per bounce
the share of k_shade<2>'s wave-steps that hold 1, 2 and 3 shading classes
(mtx_core/shade_class.h) and the classes' shares of the entries. Bounce 0 of
a film render is k_shade_cam's and is not counted."""
import ctypes as C
import json
import os
import sys

os.environ["MTX_LIB_VARIANT"] = os.environ.get("MTX_CLASS_MIX_VARIANT", "diagcls")
os.environ["MTX_SHADE_CLASSES"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mitsuba3-experiments_amd"))

BOUNCES, CLASSES = 16, 3


def main():
    import torch

    from mtx import PathIntegrator, _lib, scene

    lib = _lib.lib()
    lib.mtx_diag_shade_class_mix.argtypes = [C.c_void_p]
    lib.mtx_diag_shade_class_mix.restype = C.c_int
    sc = scene.bedroom()
    integ = PathIntegrator({"max_depth": 8, "rr_depth": 2})
    out = torch.empty((sc.height + 2, sc.width + 2, 4), dtype=torch.float32, device="cuda:0")
    buf = (C.c_ulonglong * (BOUNCES * 2 * CLASSES))()
    integ.render_film(sc, seed=0, spp=256, out=out)
    torch.cuda.synchronize()
    assert lib.mtx_diag_shade_class_mix(buf) == 2 * CLASSES, "not an MTX_DIAG_CLASSES build"
    rows, tot_w, tot_e = [], [0] * CLASSES, [0] * CLASSES
    for b in range(BOUNCES):
        w = [int(buf[b * 2 * CLASSES + k]) for k in range(CLASSES)]
        e = [int(buf[b * 2 * CLASSES + CLASSES + k]) for k in range(CLASSES)]
        if not sum(w):
            continue
        rows.append({"bounce": b, "wave_steps": sum(w), "share_with_n_classes": [round(x / sum(w), 4) for x in w],
                     "entries": sum(e), "class_share_of_entries": [round(x / sum(e), 4) for x in e]})
        if b >= 1:
            tot_w = [a + x for a, x in zip(tot_w, w)]
            tot_e = [a + x for a, x in zip(tot_e, e)]
    res = {"variant": os.environ["MTX_LIB_VARIANT"], "per_bounce": rows,
           "bounces_ge_1": {"wave_steps": sum(tot_w),
                            "share_with_n_classes": [round(x / max(1, sum(tot_w)), 4) for x in tot_w],
                            "share_with_more_than_one_class": round(1 - tot_w[0] / max(1, sum(tot_w)), 4),
                            "class_share_of_entries": [round(x / max(1, sum(tot_e)), 4) for x in tot_e]}}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
