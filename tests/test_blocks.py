"""The building blocks' surface without a GPU: the C ABI declares, lists and
exports the mtx_blocks_* entries, the module imports on a machine without a
device, and binding a scene there fails as the rest of the facade does."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = [
    "mtx_blocks_sampler_seed_dev",
    "mtx_blocks_sampler_next_dev",
    "mtx_blocks_ray_intersect_dev",
    "mtx_blocks_ray_test_dev",
    "mtx_blocks_interact_dev",
    "mtx_blocks_spawn_dev",
    "mtx_blocks_sample_emitter_dev",
    "mtx_blocks_emitter_dev",
    "mtx_blocks_bsdf_dev",
    "mtx_blocks_math_dev",
]


def test_entries_are_declared_listed_and_exported():
    from mtx import _abi, _lib

    src = open(os.path.join(ROOT, "include", "mtx.h")).read()
    declared = set(re.findall(r"\b(mtx_[a-z0-9_]+)\s*\(", src))
    L = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, name
        assert name in _abi.EXPORTS, name
        assert hasattr(L, name), name
    assert _abi.MTX_ABI_VERSION == 8 and L.mtx_abi_version() == 8  # entries were added, nothing changed
    for name in ENTRIES:  # every declaration says which reference call it replaces
        head = src[: src.index("int " + name)]
        comment = head[head.rindex("/*"):]
        assert re.search(r"\.py:\d+", comment), name


def test_plane_structs_match_the_header():
    """The ctypes plane sets hold one pointer per member of the C struct, in order."""
    from mtx import _abi

    src = open(os.path.join(ROOT, "include", "mtx.h")).read()
    for cname, cls in (("mtx_si_planes", _abi.SiPlanes), ("mtx_ds_planes", _abi.DsPlanes),
                       ("mtx_bsdf_planes", _abi.BsdfPlanes)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = re.findall(r"\*\s*([a-z_0-9]+)", body)
        assert members == [k for k, _ in cls._fields_], cname
        assert C.sizeof(cls) == 8 * len(members)


def test_math_op_codes_match_the_header():
    from mtx import _abi

    src = open(os.path.join(ROOT, "include", "mtx.h")).read()
    codes = dict(re.findall(r"(MTX_MATH_[A-Z0-9_]+) = (\d+)", src))
    assert len(codes) == 11
    for k, v in codes.items():
        assert getattr(_abi, k) == int(v), k


def test_blocks_import_without_a_device():
    import mtx
    from mtx import blocks

    assert mtx.blocks is blocks
    for name in ("Scene", "Sampler", "SurfaceInteraction", "fma", "div", "rcp", "sqrt", "dot", "norm", "normalize",
                 "mis_weight", "to_local", "to_world"):
        assert hasattr(blocks, name), name


def test_scene_without_gpu_raises(small_scene):
    import torch
    from mtx import MtxError, blocks

    if torch.cuda.is_available():
        return
    with pytest.raises(MtxError):
        blocks.Scene(small_scene)
    with pytest.raises(MtxError):
        blocks.Sampler(1, [0, 1, 2])
