"""Loader for the in-tree libmtx.so (the HIP product library).

The library is loaded from this package directory only; there is no CPU or
Python fallback for the hot path: if the library is missing or no gfx950
device is visible, the calls that need it raise :class:`MtxError`.

torch, when importable, is imported first so that torch and libmtx share one
HIP runtime (torch bundles its own libamdhip64.so.7; loading the system copy
first would put two runtimes in one process).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from . import _abi

try:  # one HIP runtime per process: torch's, if torch is present
    import torch as _torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for host-only use
    _torch = None

# MTX_LIB_VARIANT selects an in-tree tuning build (e.g. "shade4" ->
# libmtx_shade4.so, see csrc/Makefile `variants`); default libmtx.so.
_VARIANT = os.environ.get("MTX_LIB_VARIANT", "")
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        f"libmtx_{_VARIANT}.so" if _VARIANT else "libmtx.so")


class MtxError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load libmtx.so (raises MtxError if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MtxError(
            f"libmtx.so not found at {LIB_PATH}; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path."
        )
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    sig = {
        "mtx_abi_version": ([], C.c_int),
        "mtx_last_error": ([], C.c_char_p),
        "mtx_ctx_create": ([C.c_int, C.POINTER(vp)], C.c_int),
        "mtx_ctx_destroy": ([vp], None),
        "mtx_bvh_build": ([vp, u32, vp, u32, vp, C.POINTER(u32), vp, vp, C.POINTER(u32)], C.c_int),
        "mtx_bvh_build_occlusion": ([vp, u32, vp, C.POINTER(u32), vp, vp, C.POINTER(u32)], C.c_int),
        "mtx_roughplastic_tables": ([u32, C.c_float, C.c_float, vp, C.POINTER(C.c_float)], C.c_int),
        "mtx_scene_upload": ([vp, C.POINTER(_abi.SceneDesc)], C.c_int),
        "mtx_render": ([vp, C.POINTER(_abi.RenderArgs), vp, C.c_int, C.POINTER(_abi.Stats)], C.c_int),
        "mtx_last_device_ms": ([vp], C.c_double),
        "mtx_field_upload": ([vp, C.POINTER(_abi.FieldDesc)], C.c_int),
        "mtx_field_features": ([vp, u64, vp, vp, vp], C.c_int),
        "mtx_field_mlp": ([vp, u64, vp, vp], C.c_int),
        "mtx_field_eval": ([vp, u64, vp, vp, vp], C.c_int),
        "mtx_set_camera": ([vp, C.POINTER(_abi.Camera)], C.c_int),
        "mtx_restir_rows": ([vp, C.c_int, u32, u32, vp, C.c_int], C.c_int),
        "mtx_restir_state": ([vp, C.c_int, vp, u64], C.c_int),
        "mtx_sample_rays": ([vp, C.POINTER(_abi.RenderArgs), u64, vp, vp, u32, vp, vp], C.c_int),
        "mtx_sample_rays_dev": ([vp, C.POINTER(_abi.RenderArgs), u64, vp, vp, u32, vp, vp], C.c_int),
        "mtx_trace": ([vp, u64, vp, C.c_int, vp, vp], C.c_int),
        "mtx_trace_dev": ([vp, u64, vp, C.c_int, vp, vp], C.c_int),
        "mtx_prefix_sum_u32": ([vp, vp, vp, u64, C.c_int], C.c_int),
        "mtx_prefix_sum_f32_hs": ([vp, vp, vp, u64], C.c_int),
        "mtx_prefix_sum_u32_dev": ([vp, vp, vp, u64, C.c_int], C.c_int),
        "mtx_prefix_sum_f32_hs_dev": ([vp, vp, vp, u64], C.c_int),
        "mtx_hashgrid_build": ([vp, vp, u64, u32, u32, vp, vp, vp, vp], C.c_int),
        "mtx_hashgrid_build_dev": ([vp, vp, u64, u32, u32, vp, vp, vp, vp], C.c_int),
        "mtx_scatter_reduce_f32": ([vp, C.c_int, vp, u64, vp, vp, u64], C.c_int),
        "mtx_scatter_reduce_f32_dev": ([vp, C.c_int, vp, u64, vp, vp, u64], C.c_int),
        "mtx_group_by_u32": ([vp, vp, u64, u32, vp, vp, vp], C.c_int),
        "mtx_group_by_u32_dev": ([vp, vp, u64, u32, vp, vp, vp], C.c_int),
        "mtx_field_train_init": ([vp, C.POINTER(_abi.FieldOpt)], C.c_int),
        "mtx_field_grad": ([vp, u64, vp, vp, vp, C.c_float, vp, C.POINTER(C.c_double), vp, vp], C.c_int),
        "mtx_field_train_step": ([vp, u64, vp, vp, vp, C.POINTER(_abi.TrainStats)], C.c_int),
        "mtx_field_params": ([vp, vp, vp, vp, vp], C.c_int),
        "mtx_nerad_upload": ([vp, C.POINTER(_abi.NeradTables)], C.c_int),
        "mtx_nerad_lhs": ([vp, C.POINTER(_abi.NeradArgs), vp], C.c_int),
        "mtx_nerad_rhs": ([vp, C.POINTER(_abi.NeradArgs), vp, vp], C.c_int),
        "mtx_nerad_step": ([vp, C.POINTER(_abi.NeradArgs), C.POINTER(_abi.TrainStats)], C.c_int),
        "mtx_rfilter_info": ([u32, C.POINTER(u32), C.POINTER(C.c_float)], C.c_int),
        "mtx_rfilter_eval": ([u32, vp, vp, u64], C.c_int),
        "mtx_bvh_refit": ([vp, u32, vp, u32, vp, u32, vp], C.c_int),
        "mtx_bvh_refit_occlusion": ([vp, vp, u32, vp, u32, vp], C.c_int),
        "mtx_scene_update_vertices": ([vp, vp, vp, u32, C.c_int], C.c_int),
        "mtx_scene_read": ([vp, C.c_int, vp, u64], C.c_int),
        "mtx_tri_area_f32": ([vp, u64, vp], C.c_int),
        "mtx_blocks_sampler_seed_dev": ([vp, u64, u32, vp, u32, vp], C.c_int),
        "mtx_blocks_sampler_next_dev": ([vp, u64, vp, C.c_int, vp], C.c_int),
        "mtx_blocks_ray_intersect_dev": ([vp, u64, vp, vp, vp, vp, C.POINTER(_abi.SiPlanes)], C.c_int),
        "mtx_blocks_ray_test_dev": ([vp, u64, vp, vp, vp, vp, vp], C.c_int),
        "mtx_blocks_interact_dev": ([vp, u64, vp, vp, vp, vp, vp, vp, C.POINTER(_abi.SiPlanes)], C.c_int),
        "mtx_blocks_spawn_dev": ([vp, u64, vp, vp, vp, C.c_int, vp, vp, vp], C.c_int),
        "mtx_blocks_sample_emitter_dev": ([vp, u64, vp, vp, vp, vp, C.c_int, C.POINTER(_abi.DsPlanes), vp], C.c_int),
        "mtx_blocks_emitter_dev": ([vp, u64, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "mtx_blocks_bsdf_dev": ([vp, u64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(_abi.BsdfPlanes), vp], C.c_int),
        "mtx_blocks_math_dev": ([vp, C.c_int, u64, vp, vp, vp, vp], C.c_int),
        "mtx_blocks_sensor_ray_dev": ([vp, u64, vp, vp, vp, vp, vp], C.c_int),
        "mtx_blocks_sample_emitter_ray_dev": ([vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "mtx_blocks_sensor_direction_dev": ([vp, u64, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp], C.c_int),
        "mtx_blocks_light_host": ([C.POINTER(_abi.SceneDesc), C.c_int, u64, vp, vp], C.c_int),
        "mtx_blocks_bdpt_connect_dev": ([vp, u64, C.POINTER(_abi.PathPlanes), C.POINTER(_abi.PathPlanes), C.c_int,
                                         C.c_int, u32, u32, vp, vp, vp], C.c_int),
        "mtx_blocks_bdpt_host": ([C.POINTER(_abi.SceneDesc), u64, C.POINTER(_abi.PathPlanes),
                                  C.POINTER(_abi.PathPlanes), C.c_int, C.c_int, u32, u32, vp, vp], C.c_int),
        "mtx_blocks_film_put_dev": ([vp, vp, u32, u32, u32, u32, u64, vp, vp, vp, u32, u32, u32, u32, C.POINTER(u64)],
                                    C.c_int),
        "mtx_blocks_film_gather_dev": ([vp, vp, u32, u32, u32, u32, vp], C.c_int),
        "mtx_hashgrid_query_count_dev": ([vp, C.POINTER(_abi.HashGridView), vp, u64, vp, u32, vp], C.c_int),
        "mtx_hashgrid_query_fill_dev": ([vp, C.POINTER(_abi.HashGridView), vp, u64, vp, u32, vp, u64, vp, vp], C.c_int),
        "mtx_blocks_photon_gather_dev": ([vp, C.POINTER(_abi.HashGridView), C.POINTER(_abi.PhotonPlanes),
                                          C.POINTER(_abi.VisiblePlanes), u64, vp, u32, u32, vp, vp], C.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    if L.mtx_abi_version() != _abi.MTX_ABI_VERSION:
        raise MtxError("libmtx ABI version mismatch; rebuild the library")
    _lib = L
    return L


def check(rc: int, what: str = "libmtx call") -> None:
    if rc != 0:
        msg = lib().mtx_last_error().decode("utf-8", "replace")
        raise MtxError(f"{what} failed with {_abi.ERRORS.get(rc, rc)}: {msg}")


def ptr(a) -> int | None:
    """Address of a contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data


class Context:
    """One libmtx context bound to one HIP device (mirrors mtx_ctx)."""

    def __init__(self, device: int = 0):
        L = lib()
        h = C.c_void_p()
        check(L.mtx_ctx_create(int(device), C.byref(h)), f"mtx_ctx_create(device={device})")
        self._h = h
        self.device = device
        self.scene = None
        self.n_refits = 0  # vertex updates applied (update_vertices)

    @property
    def handle(self):
        return self._h

    def update_vertices(self, vpos, vnormal=None) -> None:
        """New vertex positions (and optionally normals) for the uploaded
        scene without a re-upload (mtx_scene_update_vertices): assigning
        ``vertex_positions`` and calling ``params.update()`` on
        ``mi.traverse(scene)``. `vpos` / `vnormal`: (n_verts, 3) float32
        numpy arrays, or torch CUDA tensors on this context's device (a
        simulation that lives on the GPU: nothing passes through the host; the
        tensors' producer is synchronised first). Topology stays; mesh
        emitters move with their vertices (their tables and records are
        rebuilt on the device); rectangle emitter shapes must not move;
        MtxError with the reason otherwise, and the device scene is then
        unchanged.

        The host ``Scene`` this context was bound to is stale afterwards: the
        context forgets it, so the next scene rendered through it is uploaded
        in full. Make the matching host scene with ``Scene.with_vertices``
        when one is needed (the oracle, another context)."""
        import numpy as np

        def prep(a):
            if a is None:
                return None, None, False
            if hasattr(a, "data_ptr"):  # torch tensor
                import torch
                if not a.is_cuda or a.device.index != self.device:
                    raise MtxError(f"update_vertices: tensor on {a.device}, the context is on cuda:{self.device}")
                t = a.detach().to(torch.float32).contiguous().reshape(-1, 3)
                torch.cuda.current_stream(t.device).synchronize()
                return t, t.data_ptr(), True
            h = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
            return h, h.ctypes.data, False

        p, pp, pdev = prep(vpos)
        n, np_, ndev = prep(vnormal)
        if n is not None and (ndev != pdev or len(n) != len(p)):
            raise MtxError("update_vertices: vpos and vnormal must both be numpy arrays or both CUDA tensors, "
                           "of one length")
        self._scene_key = None
        self._geom_token = None
        self.scene = None
        check(lib().mtx_scene_update_vertices(self._h, pp, np_, len(p), 1 if pdev else 0),
              "mtx_scene_update_vertices")
        self.n_refits += 1

    def scene_read(self, which: str):
        """The device copy of one scene array (mtx_scene_read; tests and
        debugging): 'nodes', 'occ_nodes', 'tri', 'occ_tri', 'shade_rec',
        'vpos', 'vnormal', 'env_sphere', 'tables' or 'emitters' (the records
        as uint32 words, 16 each). `n_*` come from the bound scene."""
        import numpy as np
        names = ["nodes", "occ_nodes", "tri", "occ_tri", "shade_rec", "vpos", "vnormal", "env_sphere", "tables",
                 "emitters"]
        s = getattr(self, "_read_counts", None)
        if s is None:
            raise MtxError("scene_read: no scene was bound to this context")
        size = {"nodes": (16 * s["n_nodes"], np.int32), "occ_nodes": (20 * s["n_occ_nodes"], np.int32),
                "tri": (9 * s["n_tris"], np.float32), "occ_tri": (9 * s["n_tris"], np.float32),
                "shade_rec": (32 * s["n_tris"], np.float32), "vpos": (3 * s["n_verts"], np.float32),
                "vnormal": (3 * s["n_verts"], np.float32), "env_sphere": (4, np.float32),
                "tables": (s["n_tables"], np.float32), "emitters": (16 * s["n_emitters"], np.uint32)}[which]
        out = np.zeros(size[0], size[1])
        check(lib().mtx_scene_read(self._h, names.index(which), out.ctypes.data, out.nbytes), "mtx_scene_read")
        return out

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mtx_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_contexts: dict[int, Context] = {}


def context(device: int | None = None) -> Context:
    """Process-wide context per device (default: torch's current device once
    torch has initialised HIP, else LOCAL_RANK or 0)."""
    if device is None:
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_initialized():
            device = torch.cuda.current_device()
        else:
            device = int(os.environ.get("LOCAL_RANK", "0"))
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]
