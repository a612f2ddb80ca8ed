"""Device-tensor building blocks: write an integrator in Python.

The calls the reference's integrators are composed of -- ``scene.ray_intersect``,
``si.spawn_ray``, ``scene.sample_emitter_direction``, ``bsdf.eval_pdf_sample``,
``sampler.next_1d``, ``dr.fma``, ``mis_weight`` -- on torch CUDA tensors, one
HIP kernel of libmtx each (``mtx_blocks_*_dev``, include/mtx.h). Every kernel
calls the per-lane functions the fixed integrators and the CPU oracle share,
so a loop written on these blocks reproduces the fused ``sample()`` bit for
bit (tests/blocks_integrators.py).

Layout: Dr.Jit's. A quantity of C components over N lanes is a contiguous
float32 (int32 for indices and flags) tensor of shape (C, N), a scalar
quantity (N,), a mask (N,) bool or uint8. ``prim`` and the BSDF type / flag
words are uint32 bit patterns in int32 tensors. Nothing is converted or
copied for the caller: a host tensor, another dtype, a non-contiguous tensor
or a length that differs from the call's N raises :class:`MtxError` naming the
argument, before any launch. N = 0 returns empty tensors without a launch.

``active=None`` means all lanes; a masked-off lane gets the zero / invalid
values and never reaches a traversal. Plain ``+ - * < min max where`` stay
torch operations (each is one IEEE operation); everything whose rounding torch
does not pin -- fused multiply-add, division, square root, dot products, frame
transforms, the MIS weights -- goes through the exact helpers below.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._lib import MtxError, check, context, lib


def _torch():
    import torch

    return torch


def _arg(name: str, t, dtypes, comps: int | None, n: int | None, dev=None):
    """Validate one tensor argument; returns its lane count."""
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise MtxError(f"{name}: expected a torch CUDA tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise MtxError(f"{name}: a host tensor (device {t.device}); the blocks take CUDA tensors")
    if dev is not None and t.device != dev:
        raise MtxError(f"{name}: on {t.device}, the call's other tensors are on {dev}")
    if t.dtype not in dtypes:
        raise MtxError(f"{name}: dtype {t.dtype}, expected {' or '.join(str(d) for d in dtypes)}")
    shape = tuple(t.shape)
    if comps is None:
        if len(shape) != 1:
            raise MtxError(f"{name}: shape {shape}, expected (N,)")
    elif len(shape) != 2 or shape[0] != comps:
        raise MtxError(f"{name}: shape {shape}, expected ({comps}, N)")
    if n is not None and shape[-1] != n:
        raise MtxError(f"{name}: {shape[-1]} lanes, the call has N = {n}")
    if not t.is_contiguous():
        raise MtxError(f"{name}: not contiguous (the kernels read whole planes; call .contiguous() yourself)")
    return shape[-1]


def _f32(name, t, comps, n, dev=None):
    return _arg(name, t, (_torch().float32,), comps, n, dev)


def _i32(name, t, n, dev=None):
    return _arg(name, t, (_torch().int32,), None, n, dev)


def _mask(name, t, n, dev):
    """A mask's data pointer (None = all lanes)."""
    if t is None:
        return None, None
    torch = _torch()
    _arg(name, t, (torch.bool, torch.uint8), None, n, dev)
    return t, t.data_ptr()


def _ctx_of(dev):
    torch = _torch()
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    torch.cuda.current_stream(dev).synchronize()  # libmtx runs on its own stream
    return context(idx)


def _empty(dev, comps, n, dtype=None):
    torch = _torch()
    return torch.empty((n,) if comps is None else (comps, n), dtype=dtype or torch.float32, device=dev)


# ------------------------------------------------------------- exact math --

def _math(op: int, name: str, args, comps_in, comps_out):
    """One launch of the elementwise kernel. args: tensors, each of comps_in
    components (None = a scalar plane or any shape for the flat ops)."""
    torch = _torch()
    a0 = args[0]
    if not isinstance(a0, torch.Tensor):
        raise MtxError(f"{name}: expected torch CUDA tensors")
    dev = a0.device
    flat = comps_in == "flat"
    if flat:
        for k, a in enumerate(args):
            if not isinstance(a, torch.Tensor) or not a.is_cuda:
                raise MtxError(f"{name}: argument {'abc'[k]} is not a CUDA tensor")
            if a.dtype != torch.float32:
                raise MtxError(f"{name}: argument {'abc'[k]} has dtype {a.dtype}, expected torch.float32")
            if not a.is_contiguous():
                raise MtxError(f"{name}: argument {'abc'[k]} is not contiguous")
            if a.device != dev:
                raise MtxError(f"{name}: argument {'abc'[k]} is on {a.device}, a is on {dev}")
        try:
            bc = torch.broadcast_tensors(*args)
        except RuntimeError as e:
            raise MtxError(f"{name}: shapes {[tuple(a.shape) for a in args]} do not broadcast") from e
        ins = [b.contiguous() for b in bc]  # (N,) against (3, N): one value per lane, repeated per component
        out = torch.empty_like(ins[0])
        n = out.numel()
    else:
        n = None
        for k, (a, c) in enumerate(zip(args, comps_in)):
            n = _f32(f"{name}: argument {'abc'[k]}", a, c, n, dev)
        ins = list(args)
        out = _empty(dev, comps_out, n)
    if n == 0:
        return out
    ctx = _ctx_of(dev)
    p = [t.data_ptr() for t in ins] + [None] * (3 - len(ins))
    check(lib().mtx_blocks_math_dev(ctx.handle, op, n, p[0], p[1], p[2], out.data_ptr()), "mtx_blocks_math_dev")
    return out


def fma(a, b, c):
    """dr.fma(a, b, c) = fmaf per element (path-mis.py:117); (N,) operands broadcast against (3, N)."""
    return _math(_abi.MTX_MATH_FMA, "fma", (a, b, c), "flat", None)


def div(a, b):
    """a / b, correctly rounded."""
    return _math(_abi.MTX_MATH_DIV, "div", (a, b), "flat", None)


def rcp(a):
    """dr.rcp: 1 / a, correctly rounded."""
    return _math(_abi.MTX_MATH_RCP, "rcp", (a,), "flat", None)


def sqrt(a):
    return _math(_abi.MTX_MATH_SQRT, "sqrt", (a,), "flat", None)


def dot(a, b):
    """dr.dot of (3, N) vectors: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    return _math(_abi.MTX_MATH_DOT3, "dot", (a, b), (3, 3), None)


def norm(a):
    return _math(_abi.MTX_MATH_NORM3, "norm", (a,), (3,), None)


def normalize(a):
    """a * (1 / sqrt(dot(a, a)))."""
    return _math(_abi.MTX_MATH_NORMALIZE3, "normalize", (a,), (3,), 3)


def to_local(sh_n, v):
    """v in the shading frame of the normal sh_n (Frame3f(sh_n).to_local)."""
    return _math(_abi.MTX_MATH_TO_LOCAL, "to_local", (sh_n, v), (3, 3), 3)


def to_world(sh_n, v):
    return _math(_abi.MTX_MATH_TO_WORLD, "to_world", (sh_n, v), (3, 3), 3)


def mis_weight(pdf_a, pdf_b, variant: str = "b"):
    """The power heuristic: variant "a" = path.py:10-18 (a^2 / (a^2 + b^2), 0 if
    not finite), "b" = path-mis.py:9-15 (a^2 / fma(b, b, a^2) where a > 0)."""
    if variant not in ("a", "b"):
        raise MtxError(f"mis_weight: variant {variant!r} (a or b)")
    op = _abi.MTX_MATH_MIS_A if variant == "a" else _abi.MTX_MATH_MIS_B
    return _math(op, "mis_weight", (pdf_a, pdf_b), (None, None), None)


# ---------------------------------------------------------------- sampler --

class Sampler:
    """IndependentSampler over the given lane ids: per-lane PCG32 seeded with
    sample_tea_32(seed, lane) and advanced by `skip` draws. ``lanes``: an
    int32 CUDA tensor (uint32 bit patterns) or a host integer array, which is
    copied to `device`. The state is an (N, 2) int64 tensor of 64-bit
    patterns (state, sequence id); every draw advances all lanes."""

    def __init__(self, seed: int, lanes, skip: int = 0, device=None):
        torch = _torch()
        if isinstance(lanes, torch.Tensor):
            n = _i32("lanes", lanes, None)
            dev = lanes.device
        else:
            if not torch.cuda.is_available():
                raise MtxError("blocks.Sampler: no GPU (the blocks have no CPU fallback)")
            dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
            lanes = torch.as_tensor(np.ascontiguousarray(lanes, np.uint32).view(np.int32), device=dev)
            n = len(lanes)
        self.seed, self.n, self.device = int(seed), n, dev
        self.state = torch.empty((n, 2), dtype=torch.int64, device=dev)
        if n:
            ctx = _ctx_of(dev)
            check(lib().mtx_blocks_sampler_seed_dev(ctx.handle, n, self.seed & 0xffffffff, lanes.data_ptr(), int(skip),
                                                    self.state.data_ptr()), "mtx_blocks_sampler_seed_dev")

    def _next(self, dims):
        out = _empty(self.device, None if dims == 1 else 2, self.n)
        if self.n:
            ctx = _ctx_of(self.device)
            check(lib().mtx_blocks_sampler_next_dev(ctx.handle, self.n, self.state.data_ptr(), dims, out.data_ptr()),
                  "mtx_blocks_sampler_next_dev")
        return out

    def next_1d(self):
        return self._next(1)

    def next_2d(self):
        return self._next(2)


# ------------------------------------------------------------ interaction --

class SurfaceInteraction:
    """SurfaceInteraction3f as planes: p, n, sh_n (3, N), uv (2, N), wi (3, N,
    local), t (N), prim, material, emitter (N, int32), bary (2, N: the hit
    record's barycentrics) and valid (N, bool). The shading frame is
    frame_from_normal(sh_n), rebuilt by every consumer."""

    _PLANES = (("p", 3), ("n", 3), ("sh_n", 3), ("uv", 2), ("wi", 3), ("t", None), ("prim", None), ("material", None),
               ("emitter", None), ("bary", 2))

    def __init__(self, dev, n):
        torch = _torch()
        for k, c in self._PLANES:
            setattr(self, k, _empty(dev, c, n, torch.int32 if k in ("prim", "material", "emitter") else None))
        self.valid = None

    def _planes(self):
        return _abi.SiPlanes(*[getattr(self, k).data_ptr() for k, _ in self._PLANES])

    def _done(self):
        self.valid = self.material >= 0
        return self

    def _spawn(self, x, to, name):
        n = _f32(name, x, 3, self.p.shape[1], self.p.device)
        o, d, maxt = _empty(x.device, 3, n), _empty(x.device, 3, n), _empty(x.device, None, n)
        if n:
            ctx = _ctx_of(x.device)
            check(lib().mtx_blocks_spawn_dev(ctx.handle, n, self.p.data_ptr(), self.n.data_ptr(), x.data_ptr(), to,
                                             o.data_ptr(), d.data_ptr(), maxt.data_ptr()), "mtx_blocks_spawn_dev")
        return o, d, maxt

    def spawn_ray(self, d):
        """si.spawn_ray(d) -> (o, d, maxt): the origin offset along the geometric normal."""
        return self._spawn(d, 0, "spawn_ray: d")

    def spawn_ray_to(self, target):
        """si.spawn_ray_to(target) -> (o, d, maxt): normalised direction, maxt short of the target."""
        return self._spawn(target, 1, "spawn_ray_to: target")

    def to_local(self, v):
        return to_local(self.sh_n, v)

    def to_world(self, v):
        return to_world(self.sh_n, v)


class DirectionSample:
    """DirectionSample3f planes: p, n, d (3, N), dist, pdf (N), emitter (N, int32)."""

    _PLANES = (("p", 3), ("n", 3), ("d", 3), ("dist", None), ("pdf", None), ("emitter", None))

    def __init__(self, dev, n):
        torch = _torch()
        for k, c in self._PLANES:
            setattr(self, k, _empty(dev, c, n, torch.int32 if k == "emitter" else None))


class BSDFSample:
    """BSDFSample3f planes: wo (3, N, local), pdf, eta (N), sampled_type (N, int32 BSDFFlags bits)."""

    def __init__(self, wo, pdf, eta, sampled_type):
        self.wo, self.pdf, self.eta, self.sampled_type = wo, pdf, eta, sampled_type


# BSDFFlags (mtx_core/bsdf.h)
BF_NULL, BF_SMOOTH, BF_DELTA = 0x01, 0x02 | 0x04 | 0x08 | 0x10, 0x01 | 0x20 | 0x40


class Scene:
    """An ``mtx.scene.Scene`` bound to a device, with the reference's scene
    calls as methods on CUDA tensors. The context of a device is shared with
    the rest of the facade; every call re-binds this scene if another one was
    rendered in between."""

    def __init__(self, scene, device=None):
        from .integrators import _bind_scene, mtx_scene_of

        self.scene = mtx_scene_of(scene)
        self.ctx = context(device)  # MtxError without a gfx950 device
        self._bind = _bind_scene
        self._bind(self.ctx, self.scene)

    @property
    def has_environment(self) -> bool:
        return getattr(self.scene, "env_radiance", None) is not None

    def _call(self, dev):
        torch = _torch()
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        if idx != self.ctx.device:
            raise MtxError(f"tensors on cuda:{idx}, the scene is bound to cuda:{self.ctx.device}")
        torch.cuda.current_stream(dev).synchronize()  # libmtx runs on its own stream
        self._bind(self.ctx, self.scene)
        return self.ctx.handle

    # ------------------------------------------------------------ tracing --
    def ray_intersect(self, o, d, maxt=None, active=None) -> SurfaceInteraction:
        """scene.ray_intersect(ray): closest hit and its interaction in one
        launch. d need not be normalised; its largest component magnitude must
        lie in [2^-40, 2^60] (mtx_trace's contract, include/mtx.h)."""
        n = _f32("ray_intersect: o", o, 3, None)
        dev = o.device
        _f32("ray_intersect: d", d, 3, n, dev)
        if maxt is not None:
            _f32("ray_intersect: maxt", maxt, None, n, dev)
        _, am = _mask("ray_intersect: active", active, n, dev)
        si = SurfaceInteraction(dev, n)
        if n:
            pl = si._planes()
            check(lib().mtx_blocks_ray_intersect_dev(self._call(dev), n, o.data_ptr(), d.data_ptr(),
                                                     maxt.data_ptr() if maxt is not None else None, am, C.byref(pl)),
                  "mtx_blocks_ray_intersect_dev")
        return si._done()

    def ray_test(self, o, d, maxt, active=None):
        """scene.ray_test(ray): True where the ray is occluded within maxt."""
        torch = _torch()
        n = _f32("ray_test: o", o, 3, None)
        dev = o.device
        _f32("ray_test: d", d, 3, n, dev)
        _f32("ray_test: maxt", maxt, None, n, dev)
        _, am = _mask("ray_test: active", active, n, dev)
        out = _empty(dev, None, n, torch.uint8)
        if n:
            check(lib().mtx_blocks_ray_test_dev(self._call(dev), n, o.data_ptr(), d.data_ptr(), maxt.data_ptr(), am,
                                                out.data_ptr()), "mtx_blocks_ray_test_dev")
        return out.bool()

    def interact(self, d, t, prim, u, v, active=None) -> SurfaceInteraction:
        """The interaction of hit records the caller holds (``trace_rays``'
        t, prim, u, v) for rays of direction d; prim = -1 (0xffffffff) is a miss."""
        n = _f32("interact: d", d, 3, None)
        dev = d.device
        _f32("interact: t", t, None, n, dev)
        _i32("interact: prim", prim, n, dev)
        _f32("interact: u", u, None, n, dev)
        _f32("interact: v", v, None, n, dev)
        _, am = _mask("interact: active", active, n, dev)
        si = SurfaceInteraction(dev, n)
        if n:
            pl = si._planes()
            check(lib().mtx_blocks_interact_dev(self._call(dev), n, d.data_ptr(), t.data_ptr(), prim.data_ptr(),
                                                u.data_ptr(), v.data_ptr(), am, C.byref(pl)),
                  "mtx_blocks_interact_dev")
        return si._done()

    # ----------------------------------------------------------- emitters --
    def sample_emitter_direction(self, si, u, test_visibility: bool = True, active=None):
        """scene.sample_emitter_direction(si, u, test_visibility, active) ->
        (DirectionSample, weight (3, N)); with test_visibility the shadow ray
        runs in the same launch and an occluded sample's weight is zero."""
        n = _f32("sample_emitter_direction: si.p", si.p, 3, None)
        dev = si.p.device
        _f32("sample_emitter_direction: si.n", si.n, 3, n, dev)
        _f32("sample_emitter_direction: u", u, 2, n, dev)
        _, am = _mask("sample_emitter_direction: active", active, n, dev)
        ds, w = DirectionSample(dev, n), _empty(dev, 3, n)
        if n:
            pl = _abi.DsPlanes(*[getattr(ds, k).data_ptr() for k, _ in ds._PLANES])
            check(lib().mtx_blocks_sample_emitter_dev(self._call(dev), n, si.p.data_ptr(), si.n.data_ptr(),
                                                      u.data_ptr(), am, int(bool(test_visibility)), C.byref(pl),
                                                      w.data_ptr()), "mtx_blocks_sample_emitter_dev")
        return ds, w

    def _emitter(self, name, emitter, d, dist, nrm, wi, active, want_pdf, want_le):
        n = _i32(f"{name}: emitter", emitter, None)
        dev = emitter.device
        if want_pdf:
            _f32(f"{name}: d", d, 3, n, dev)
            _f32(f"{name}: dist", dist, None, n, dev)
            _f32(f"{name}: n", nrm, 3, n, dev)
        if want_le:
            _f32(f"{name}: wi", wi, 3, n, dev)
        _, am = _mask(f"{name}: active", active, n, dev)
        pdf = _empty(dev, None, n) if want_pdf else None
        le = _empty(dev, 3, n) if want_le else None
        if n:
            q = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
            check(lib().mtx_blocks_emitter_dev(self._call(dev), n, emitter.data_ptr(), q(d) if want_pdf else None,
                                               q(dist) if want_pdf else None, q(nrm) if want_pdf else None,
                                               q(wi) if want_le else None, am, q(pdf), q(le)),
                  "mtx_blocks_emitter_dev")
        return pdf, le

    def pdf_emitter(self, emitter, d, dist, n, active=None):
        """Scene::pdf_emitter_direction on explicit planes: the solid-angle pdf
        of the direction d (3, N) at distance dist towards the emitter index
        of each lane, whose surface normal is n; 0 for -1."""
        return self._emitter("pdf_emitter", emitter, d, dist, n, None, active, True, False)[0]

    def pdf_emitter_direction(self, prev_p, si, active=None):
        """scene.pdf_emitter_direction(prev_si, DirectionSample3f(scene, si,
        prev_si)): ds.d = (si.p - prev_p) / |si.p - prev_p| for a valid
        interaction, else -to_world(si.wi) (an environment hit), ds.dist the
        norm, ds.n the shading normal."""
        torch = _torch()
        n = _f32("pdf_emitter_direction: prev_p", prev_p, 3, None)
        _f32("pdf_emitter_direction: si.p", si.p, 3, n, prev_p.device)
        rel = si.p - prev_p
        dist = norm(rel)
        ds_d = torch.where(si.valid, div(rel, dist), -si.to_world(si.wi))
        return self.pdf_emitter(si.emitter, ds_d, dist, si.sh_n, active)

    def emitter_eval(self, si, active=None):
        """si.emitter(scene).eval(si): the radiance seen from the front side (3, N)."""
        return self._emitter("emitter_eval", si.emitter, None, None, None, si.wi, active, False, True)[1]

    # --------------------------------------------------------------- BSDF --
    def bsdf_eval_pdf_sample(self, si, wo, u1, u2, active=None):
        """bsdf.eval_pdf_sample(ctx, si, wo, u1, u2) -> (value (3, N), pdf (N),
        BSDFSample, weight (3, N)). wo is local. material < 0 is the null
        BSDF: zeros. Needs si.material, si.uv and si.wi."""
        torch = _torch()
        n = _i32("bsdf_eval_pdf_sample: si.material", si.material, None)
        dev = si.material.device
        _f32("bsdf_eval_pdf_sample: si.uv", si.uv, 2, n, dev)
        _f32("bsdf_eval_pdf_sample: si.wi", si.wi, 3, n, dev)
        _f32("bsdf_eval_pdf_sample: wo", wo, 3, n, dev)
        _f32("bsdf_eval_pdf_sample: u1", u1, None, n, dev)
        _f32("bsdf_eval_pdf_sample: u2", u2, 2, n, dev)
        _, am = _mask("bsdf_eval_pdf_sample: active", active, n, dev)
        val, pdf, weight = _empty(dev, 3, n), _empty(dev, None, n), _empty(dev, 3, n)
        bs = BSDFSample(_empty(dev, 3, n), _empty(dev, None, n), _empty(dev, None, n),
                        _empty(dev, None, n, torch.int32))
        if n:
            pl = _abi.BsdfPlanes(val.data_ptr(), pdf.data_ptr(), bs.wo.data_ptr(), bs.pdf.data_ptr(),
                                 bs.eta.data_ptr(), bs.sampled_type.data_ptr(), weight.data_ptr())
            check(lib().mtx_blocks_bsdf_dev(self._call(dev), n, si.material.data_ptr(), si.uv.data_ptr(),
                                            si.wi.data_ptr(), wo.data_ptr(), u1.data_ptr(), u2.data_ptr(), am,
                                            C.byref(pl), None), "mtx_blocks_bsdf_dev")
        return val, pdf, bs, weight

    def bsdf_flags(self, si):
        """bsdf.flags() of each lane's material (N, int32 BSDFFlags bits); 0 for an invalid interaction."""
        torch = _torch()
        n = _i32("bsdf_flags: si.material", si.material, None)
        dev = si.material.device
        out = _empty(dev, None, n, torch.int32)
        if n:
            check(lib().mtx_blocks_bsdf_dev(self._call(dev), n, si.material.data_ptr(), None, None, None, None, None,
                                            None, None, out.data_ptr()), "mtx_blocks_bsdf_dev")
        return out
