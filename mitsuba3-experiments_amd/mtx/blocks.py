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

Around a ``sample()`` written this way, :class:`Sensor` (``sensor.sample_ray``),
:class:`Film` (``ImageBlock.put`` and the film's fixed order, on planes the
caller owns) and :class:`SamplingIntegrator` (the render loop of
path.py:103-192; ``mtx.register_integrator`` / ``mtx.load_dict`` take a
subclass) make it a renderer whose raw film equals the fused integrator's
bit for bit when the loop restates that integrator.

Paths may also start at the lights: ``Scene.sample_emitter_ray`` emits,
``Sensor.sample_direction`` connects a surface point to the camera,
:class:`AdjointIntegrator` is the render loop that splats through
``Film.put``'s general path, and :class:`ParticleTracer` (``"ptracer"``) is
the estimator built on them.

The two meet in :class:`PathVertices` (a vertex store per subpath),
:func:`connect_subpaths` (every connection strategy (s, t) with its shadow
ray and its power-heuristic weight, one kernel; include/mtx_core/bdpt.h) and
:class:`BidirectionalPathTracer` (``"bdpt"``).

Photons: ``mtx.primitives.HashGrid.query`` finds the samples within a radius
of each query point in a fixed walk order, :meth:`Scene.photon_gather` fuses
that walk with the density estimate at visible points (one kernel, equal to
its composition from the blocks bit for bit) and :class:`PhotonMapper`
(``"sppm"``) is the progressive photon mapper built on them.
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


class EmitterSample:
    """The start of a light path: p, n (3, N), the unoffset position and the
    normal the direction was drawn about, and emitter (N, int32), the picked
    index (the environment: n_emitters; -1: no emitter, or a masked-off lane)."""

    def __init__(self, p, n, emitter):
        self.p, self.n, self.emitter = p, n, emitter


class SensorDirectionSample:
    """sensor.sample_direction planes: pos (2, N) film position in pixels,
    d (3, N) unit direction towards the camera, dist, weight (N), valid (N, bool)."""

    def __init__(self, pos, d, dist, weight, valid):
        self.pos, self.d, self.dist, self.weight, self.valid = pos, d, dist, weight, valid


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

    def sample_emitter_ray(self, u_pos, u_dir, active=None):
        """scene.sample_emitter_ray(time, sample1, u_pos, u_dir, active)
        (bdpt02.py:86-88) -> (Ray, weight (3, N), EmitterSample). u_pos.x picks
        the emitter and is reused; the position is the emitter's
        sample_position, the direction a cosine hemisphere about its normal;
        weight = radiance * pi / pdf_pos * count (the environment: radiance *
        4 pi^2 r^2 * count, from the scene's bounding sphere)."""
        torch = _torch()
        n = _f32("sample_emitter_ray: u_pos", u_pos, 2, None)
        dev = u_pos.device
        _f32("sample_emitter_ray: u_dir", u_dir, 2, n, dev)
        _, am = _mask("sample_emitter_ray: active", active, n, dev)
        o, d, maxt, w = _empty(dev, 3, n), _empty(dev, 3, n), _empty(dev, None, n), _empty(dev, 3, n)
        es = EmitterSample(_empty(dev, 3, n), _empty(dev, 3, n), _empty(dev, None, n, torch.int32))
        if n:
            check(lib().mtx_blocks_sample_emitter_ray_dev(self._call(dev), n, u_pos.data_ptr(), u_dir.data_ptr(), am,
                                                          o.data_ptr(), d.data_ptr(), maxt.data_ptr(), w.data_ptr(),
                                                          es.p.data_ptr(), es.n.data_ptr(), es.emitter.data_ptr()),
                  "mtx_blocks_sample_emitter_ray_dev")
        return Ray(o, d, maxt), w, es

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

    # ------------------------------------------------------------ photons --
    def photon_gather(self, grid, si, depth_q, radius, d_p, beta_p, depth_p, max_depth):
        """The density estimate at the visible points `si` over the photons
        of `grid` (a ``mtx.primitives.HashGrid`` built over their positions)
        within `radius` (a float or an (N,) tensor), one fused kernel:
        ``grid.query`` 's walk, and per neighbour j of lane i, in walk order,
        ``depth_q[i] + depth_p[j] <= max_depth``; wo = to_local(si.sh_n, d_p[j]);
        val = bsdf.eval(si, wo) (with its shading cosine, as
        :meth:`bsdf_eval_pdf_sample` returns it); cg = dot(si.n, d_p[j]); the
        pair counts where cg * wo.z > 0 and si.wi.z * wo.z > 0; sum += val *
        beta_p[j] / |cg|. Returns (sum (3, N), count (N, int32): the pairs
        that counted). d_p, beta_p (3, n): each photon's world direction
        towards where it came from and its weight; depth_p (n, int32),
        depth_q (an int or (N,) int32): segments of the two subpaths.
        si.material < 0: the null BSDF, nothing is gathered. Needs si.p,
        material, uv, wi, sh_n and n. The result equals the composition
        query / index_select / to_local / bsdf_eval_pdf_sample / dot / div /
        scatter_reduce_with("add") bit for bit."""
        torch = _torch()
        name = "photon_gather"
        if not hasattr(grid, "_query_args"):
            raise MtxError(f"{name}: grid: expected a mtx.primitives.HashGrid")
        m = _f32(f"{name}: si.p", si.p, 3, None)
        dev = si.p.device
        _, rad, stride = grid._query_args(si.p, radius, name)
        _i32(f"{name}: si.material", si.material, m, dev)
        _f32(f"{name}: si.uv", si.uv, 2, m, dev)
        _f32(f"{name}: si.wi", si.wi, 3, m, dev)
        _f32(f"{name}: si.sh_n", si.sh_n, 3, m, dev)
        _f32(f"{name}: si.n", si.n, 3, m, dev)
        if isinstance(depth_q, torch.Tensor):
            _i32(f"{name}: depth_q", depth_q, m, dev)
        else:
            depth_q = torch.full((m,), int(depth_q), dtype=torch.int32, device=dev)
        n = grid.n_samples
        _f32(f"{name}: d_p", d_p, 3, n, dev)
        _f32(f"{name}: beta_p", beta_p, 3, n, dev)
        _i32(f"{name}: depth_p", depth_p, n, dev)
        max_depth = int(max_depth)
        if not 0 <= max_depth < 2 ** 32:
            raise MtxError(f"{name}: max_depth = {max_depth}: expected a segment count in [0, 2^32)")
        out, cnt = torch.zeros((3, m), dtype=torch.float32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
        if m and n:
            view = grid._view()
            ph = _abi.PhotonPlanes(d_p.data_ptr(), beta_p.data_ptr(), depth_p.data_ptr())
            vp = _abi.VisiblePlanes(si.p.data_ptr(), si.material.data_ptr(), si.uv.data_ptr(), si.wi.data_ptr(),
                                    si.sh_n.data_ptr(), si.n.data_ptr(), depth_q.data_ptr())
            check(lib().mtx_blocks_photon_gather_dev(self._call(dev), C.byref(view), C.byref(ph), C.byref(vp), m,
                                                     rad.data_ptr(), stride, max_depth, out.data_ptr(),
                                                     cnt.data_ptr()), "mtx_blocks_photon_gather_dev")
        return out, cnt


# ------------------------------------------------------------------ sensor --

class Ray:
    """A wavefront of rays: o, d (3, N) and maxt (N; None = unbounded)."""

    def __init__(self, o, d, maxt=None):
        self.o, self.d, self.maxt = o, d, maxt


def _mtx_scene(scene):
    from .integrators import mtx_scene_of

    return scene.scene if isinstance(scene, Scene) else mtx_scene_of(scene)


class Sensor:
    """The scene's camera, or `sensor` in any form :func:`mtx.scene_with_sensor`
    takes (an ``mtx_camera``, ``Scene.sensors()[i]``, a perspective sensor
    dictionary, ...), with the reference's ``sensor.sample_ray`` on CUDA
    tensors (path.py:45-62)."""

    def __init__(self, scene, sensor=None, device=None):
        from .integrators import _bind_scene, scene_with_sensor

        self.scene = scene_with_sensor(_mtx_scene(scene), sensor)
        self.ctx = context(device)
        self._bind = _bind_scene
        self._bind(self.ctx, self.scene)

    @property
    def width(self) -> int:
        return int(self.scene.width)

    @property
    def height(self) -> int:
        return int(self.scene.height)

    def sample_ray(self, pos, active=None) -> Ray:
        """Rays through the film positions pos (2, N) in pixels (pixel +
        jitter, path.py:45): camera_ray(pos / size), the camera rays of the
        fixed integrators. ``maxt`` reaches the far clip, as theirs does.
        Masked-off lanes get zeros."""
        torch = _torch()
        n = _f32("sample_ray: pos", pos, 2, None)
        dev = pos.device
        _, am = _mask("sample_ray: active", active, n, dev)
        o, d, maxt = _empty(dev, 3, n), _empty(dev, 3, n), _empty(dev, None, n)
        if n:
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            if idx != self.ctx.device:
                raise MtxError(f"tensors on cuda:{idx}, the sensor is bound to cuda:{self.ctx.device}")
            torch.cuda.current_stream(dev).synchronize()  # libmtx runs on its own stream
            self._bind(self.ctx, self.scene)
            check(lib().mtx_blocks_sensor_ray_dev(self.ctx.handle, n, pos.data_ptr(), am, o.data_ptr(), d.data_ptr(),
                                                  maxt.data_ptr()), "mtx_blocks_sensor_ray_dev")
        return Ray(o, d, maxt)

    def sample_direction(self, p, n, test_visibility: bool = True, active=None) -> SensorDirectionSample:
        """sensor.sample_direction(it, ..): connect the points p (3, N), whose
        geometric normals are n (3, N), to the pinhole. ``weight`` is the
        importance over the squared distance, importance = 1 / (4 tan_x tan_y
        cos^3 theta); outside the clip range or the frustum a lane is not
        ``valid`` and all its outputs are zero. With test_visibility the
        connection ray spawn_ray_to(p, n, origin) runs through the any-hit
        tree in the same launch and an occluded sample's weight is zero."""
        torch = _torch()
        cnt = _f32("sample_direction: p", p, 3, None)
        dev = p.device
        _f32("sample_direction: n", n, 3, cnt, dev)
        _, am = _mask("sample_direction: active", active, cnt, dev)
        pos, d, dist, w = _empty(dev, 2, cnt), _empty(dev, 3, cnt), _empty(dev, None, cnt), _empty(dev, None, cnt)
        valid = _empty(dev, None, cnt, torch.uint8)
        if cnt:
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            if idx != self.ctx.device:
                raise MtxError(f"tensors on cuda:{idx}, the sensor is bound to cuda:{self.ctx.device}")
            torch.cuda.current_stream(dev).synchronize()  # libmtx runs on its own stream
            self._bind(self.ctx, self.scene)
            check(lib().mtx_blocks_sensor_direction_dev(self.ctx.handle, cnt, p.data_ptr(), n.data_ptr(), am,
                                                        int(bool(test_visibility)), pos.data_ptr(), d.data_ptr(),
                                                        dist.data_ptr(), w.data_ptr(), valid.data_ptr()),
                  "mtx_blocks_sensor_direction_dev")
        return SensorDirectionSample(pos, d, dist, w, valid.bool())


def light_host(scene, op: int, values) -> np.ndarray:
    """The CPU twin of the two light-path kernels (mtx_blocks_light_host,
    include/mtx.h): needs no GPU. ``scene``: an ``mtx.scene.Scene``; ``op``:
    ``_abi.MTX_LIGHT_*``; ``values``: the (C, N) float32 input planes. Returns
    the (C', N) float32 output planes, integer outputs as bit patterns."""
    rows = {_abi.MTX_LIGHT_EMITTER_RAY: (4, 17), _abi.MTX_LIGHT_SENSOR_DIRECTION: (3, 8),
            _abi.MTX_LIGHT_PROJECT: (3, 3)}
    if op not in rows:
        raise MtxError(f"light_host: unknown op {op!r}")
    a = np.ascontiguousarray(values, np.float32)
    if a.ndim != 2 or a.shape[0] != rows[op][0]:
        raise MtxError(f"light_host: input of shape {a.shape}, expected ({rows[op][0]}, N)")
    out = np.zeros((rows[op][1], a.shape[1]), np.float32)
    desc = _mtx_scene(scene).desc()
    check(lib().mtx_blocks_light_host(C.byref(desc), int(op), a.shape[1], a.ctypes.data, out.ctypes.data),
          "mtx_blocks_light_host")
    return out


# -------------------------------------------------------------------- film --

def _rfilter_id(rfilter) -> int:
    fid = _abi.RFILTERS.get(rfilter, rfilter)
    if fid not in _abi.RFILTER_BORDER:
        raise MtxError(f"unknown reconstruction filter {rfilter!r}; supported: {sorted(_abi.RFILTERS)}")
    return fid


def develop(raw, border: int):
    """hdrfilm develop of a raw film tensor (rows + 2b, W + 2b, 4): the inner
    pixels, RGB / weight by the exact division (0 where the weight is 0)."""
    torch = _torch()
    border = int(border)
    if border < 0 or 2 * border >= min(raw.shape[0], raw.shape[1]):
        raise MtxError(f"border {border} does not fit a film of shape {tuple(raw.shape)}")
    inner = raw[border: raw.shape[0] - border, border: raw.shape[1] - border]
    w = inner[..., 3:4]
    lit = w != 0
    rgb = div(inner[..., :3].contiguous(), torch.where(lit, w, torch.ones_like(w)).expand(-1, -1, 3).contiguous())
    return torch.where(lit, rgb, torch.zeros_like(rgb))


class Film:
    """The film of rows [y0, y1) of an image `width` wide, filled by
    :meth:`put` (ImageBlock.put, path.py:101) and read by :meth:`raw` /
    :meth:`develop`: the two stages and the fixed order of the fixed
    integrators' film (DESIGN.md "Film"), so equal samples give equal bits.
    The state is ``planes``, a zeroed (8, K, band pixels, 4) tensor: 8 partial
    slots x K = (2b + 1)^2 taps of the filter (b = its reach)."""

    def __init__(self, width: int, y0: int, y1: int, rfilter="tent", device=None):
        torch = _torch()
        self.rfilter = _rfilter_id(rfilter)
        self.border = _abi.RFILTER_BORDER[self.rfilter]
        self.width, self.y0, self.y1 = int(width), int(y0), int(y1)
        if self.width <= 0 or self.y0 < 0 or self.y1 <= self.y0:
            raise MtxError(f"Film: bad band (width {width}, rows [{y0}, {y1}))")
        if not torch.cuda.is_available():
            raise MtxError("blocks.Film: no GPU (the blocks have no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.band_px = (self.y1 - self.y0) * self.width
        self.planes = torch.zeros((8, (2 * self.border + 1) ** 2, self.band_px, 4), dtype=torch.float32,
                                  device=self.device)

    def put(self, pos, L, active=None, spp_total=None, sample_offset: int = 0, pixel_major_spp: int = 0,
            px0: int | None = None) -> int:
        """Splat the samples (pos (2, N) in pixels, L (3, N)) and return how
        many were dropped for a non-finite position or a source pixel
        (floor(pos)) outside the band; inactive lanes are skipped silently.

        Per source pixel the call's kept samples, in ascending lane order,
        are samples ``sample_offset + 0, 1, ..`` of ``spp_total`` (None: the
        pixel's count in this call) and fall into the 8 slots accordingly;
        the accumulators continue from the planes. So passes of whole
        pixels, and sample ranges with ``spp_total`` / ``sample_offset``,
        leave the planes of the single put.

        ``pixel_major_spp = s``: lane i belongs to pixel ``px0 + i // s``
        (y * width + x; default px0: the band's first pixel), the layout of
        a render loop. No grouping pass then; the claim is verified on the
        device first, and a false one raises with the planes unchanged."""
        n = _f32("put: pos", pos, 2, None)
        dev = pos.device
        _f32("put: L", L, 3, n, dev)
        _, am = _mask("put: active", active, n, dev)
        if dev != self.planes.device:
            raise MtxError(f"put: pos: on {dev}, the film is on {self.planes.device}")
        s = int(pixel_major_spp)
        if s < 0 or int(sample_offset) < 0 or (spp_total is not None and int(spp_total) <= 0):
            raise MtxError("put: pixel_major_spp, sample_offset >= 0 and spp_total > 0 expected")
        if n == 0:
            return 0
        dropped = C.c_uint64(0)
        check(lib().mtx_blocks_film_put_dev(_ctx_of(dev).handle, self.planes.data_ptr(), self.width, self.y0, self.y1,
                                            self.rfilter, n, pos.data_ptr(), L.data_ptr(), am, int(spp_total or 0),
                                            int(sample_offset), s, int(self.y0 * self.width if px0 is None else px0),
                                            C.byref(dropped)), "mtx_blocks_film_put_dev")
        return int(dropped.value)

    def raw(self):
        """The raw film (rows + 2b, W + 2b, 4) RGBW: mtx_render's layout and order."""
        torch = _torch()
        b = self.border
        out = torch.empty((self.y1 - self.y0 + 2 * b, self.width + 2 * b, 4), dtype=torch.float32, device=self.device)
        check(lib().mtx_blocks_film_gather_dev(_ctx_of(self.device).handle, self.planes.data_ptr(), self.width,
                                               self.y0, self.y1, self.rfilter, out.data_ptr()),
              "mtx_blocks_film_gather_dev")
        return out

    def develop(self):
        """(rows, W, 3): the border cropped, RGB / weight."""
        return develop(self.raw(), self.border)


# -------------------------------------------------------------- integrator --

class SamplingIntegrator:
    """Base class of an integrator written on the blocks. Override
    :meth:`sample`; :meth:`render_film` / :meth:`render` are the reference's
    render loop (path.py:103-192) on device tensors: per pass the lane ids
    ``pixel * spp_total + sample_offset + s``, a :class:`Sampler` seeded with
    them, ``next_2d`` as the film jitter, ``Sensor.sample_ray``, ``sample()``
    with the sampler after those two draws, ``Film.put``. A subclass that
    restates a fixed integrator renders that integrator's raw film bit for
    bit. Register one with ``mtx.register_integrator(name, Cls)`` and load it
    with ``mtx.load_dict({"type": name, ...})``."""

    name = ""

    def __init__(self, props=None):
        from .integrators import Properties

        self.props = Properties(props or {})
        self.rfilter = self.props.get("rfilter", "tent")  # "tent", "box", "gaussian" or "scene"

    def rfilter_id(self, scene, rfilter=None) -> int:
        """As the fixed integrators' ``rfilter_id``: the argument, else the
        ``rfilter`` property; "scene" = the filter the scene's film declares."""
        from .integrators import SamplingIntegrator as Fixed

        return Fixed.rfilter_id(self, _mtx_scene(scene), rfilter)

    def sample(self, scene, sampler, ray, medium=None, active=None):
        """-> (L (3, N), valid (N), aovs). scene: :class:`Scene`, sampler:
        :class:`Sampler`, ray: ``.o`` / ``.d`` (3, N) and ``.maxt`` (N)."""
        raise NotImplementedError(f"{type(self).__name__} does not override sample()")

    def render_film(self, scene, seed: int = 0, spp: int = 1, y0: int = 0, y1: int | None = None,
                    spp_total: int | None = None, sample_offset: int = 0, sensor=None, rfilter=None,
                    max_lanes: int | None = None):
        """The raw film tensor of rows [y0, y1) (see the fixed integrators'
        ``render_film``). ``max_lanes``: at most that many lanes per pass
        (whole pixels, at least one); the film does not depend on it."""
        torch = _torch()
        fid = self.rfilter_id(scene, rfilter)  # an unknown filter is refused before anything is bound or launched
        sens = Sensor(scene, sensor)
        scn = Scene(sens.scene, sens.ctx.device)
        W, H = sens.width, sens.height
        y0, y1 = int(y0), int(H if y1 is None else y1)
        spp, T, off = int(spp), int(spp_total or spp), int(sample_offset)
        if spp <= 0 or not 0 <= y0 < y1 <= H or off < 0 or T < off + spp:
            raise MtxError("render_film: bad rows / spp arguments")
        film = Film(W, y0, y1, fid, sens.ctx.device)
        dev = film.device
        n_px = (y1 - y0) * W
        per_pass = n_px if max_lanes is None else max(1, int(max_lanes) // spp)
        smp = torch.arange(spp, dtype=torch.int64, device=dev)
        for p0 in range(0, n_px, per_pass):
            pix = torch.arange(y0 * W + p0, y0 * W + min(n_px, p0 + per_pass), dtype=torch.int64, device=dev)
            pix = pix.repeat_interleave(spp)
            lanes = (pix * T + off + smp.repeat(len(pix) // spp)) & 0xffffffff
            lanes = torch.where(lanes >= 2 ** 31, lanes - 2 ** 32, lanes).to(torch.int32)  # uint32 bit patterns
            sampler = Sampler(seed, lanes)
            u = sampler.next_2d()  # the film jitter (path.py:45)
            pos = torch.stack([(pix % W).to(torch.float32) + u[0], (pix // W).to(torch.float32) + u[1]])
            ray = sens.sample_ray(pos)
            L, _valid, _aovs = self.sample(scn, sampler, ray, None, None)
            film.put(pos, L.contiguous(), spp_total=T, sample_offset=off, pixel_major_spp=spp, px0=y0 * W + p0)
        return film.raw()

    def render(self, scene, sensor=None, seed: int = 0, spp: int = 1, develop: bool = True, evaluate: bool = True,
               rfilter=None):
        """SamplingIntegrator.render (path.py:103-192): the (H, W, 3) image
        tensor, or the raw film with develop=False."""
        raw = self.render_film(scene, seed=seed, spp=spp, sensor=sensor, rfilter=rfilter)
        if not develop:
            return raw
        return globals()["develop"](raw, _abi.RFILTER_BORDER[self.rfilter_id(scene, rfilter)])


# ----------------------------------------------------- adjoint integrators --

class AdjointIntegrator:
    """Base class of an integrator that starts its paths at the lights and
    splats onto the film (Mitsuba's ``AdjointIntegrator``). Override
    :meth:`sample`, which emits ``sampler.n`` particles and adds their
    contributions with :meth:`splat`.

    :meth:`render_film` traces ``spp * width * height`` particles in passes
    of at most ``samples_per_pass`` (property, default 2^20), each with a
    :class:`Sampler` seeded by the global particle indices of the pass, so the
    film depends on the seed and the particle count alone: the same seed and
    count give the same bits. Contributions are scaled by ``sample_scale =
    pixel_count / total_particles``. The raw film it returns has the layout
    of :meth:`SamplingIntegrator.render_film`, with the weight channel set to
    1 (the sum of the splats is the estimate; Mitsuba overwrites the channel
    the same way), so ``develop`` applies unchanged.

    Filters: "box" (the default here) and "tent", whose taps sum to 1. With
    the tent the outermost pixels miss the share of splats that would arrive
    from positions outside the frustum. "gaussian" is refused: its taps do
    not sum to 1."""

    name = ""

    def __init__(self, props=None):
        from .integrators import Properties

        self.props = Properties(props or {})
        self.rfilter = self.props.get("rfilter", "box")
        self.samples_per_pass = int(self.props.get("samples_per_pass", 1 << 20))
        if self.samples_per_pass <= 0:
            raise MtxError(f"samples_per_pass = {self.samples_per_pass}: expected a positive particle count")

    def rfilter_id(self, scene, rfilter=None) -> int:
        from .integrators import SamplingIntegrator as Fixed

        fid = Fixed.rfilter_id(self, _mtx_scene(scene), rfilter)
        if fid == _abi.RFILTERS["gaussian"]:
            raise MtxError("an adjoint integrator splats unnormalised contributions: the gaussian filter's taps do "
                           "not sum to 1; use 'box' or 'tent'")
        return fid

    def check_scene(self, scene) -> None:
        """Refuse a scene the estimator cannot render (MtxError); the default accepts all."""

    def sample(self, scene, sensor, sampler, film, sample_scale) -> None:
        """Emit sampler.n particles into `film`. scene: :class:`Scene`,
        sensor: :class:`Sensor`, sampler: :class:`Sampler` (untouched),
        sample_scale: the factor every contribution carries."""
        raise NotImplementedError(f"{type(self).__name__} does not override sample()")

    def splat(self, film, pos, value, active) -> None:
        """``Film.put`` of the contributions value (3, N) at the film
        positions pos (2, N) through the general path. Lanes that are off, or
        whose position lies on the film's upper edge or outside the band, are
        masked, so the put drops nothing."""
        on = active & (pos[0] >= 0) & (pos[0] < film.width) & (pos[1] >= film.y0) & (pos[1] < film.y1)
        dropped = film.put(pos, value.contiguous(), active=on)
        if dropped:
            raise MtxError(f"splat: {dropped} contributions with a non-finite film position")

    def render_film(self, scene, seed: int = 0, spp: int = 1, y0: int = 0, y1: int | None = None, sensor=None,
                    rfilter=None, samples_per_pass: int | None = None):
        """The raw film tensor of rows [y0, y1): (rows + 2b, W + 2b, 4), RGB =
        the scaled sum of the splats, weight = 1. The particles are those of
        the whole film whatever the band."""
        torch = _torch()
        fid = self.rfilter_id(scene, rfilter)
        sens = Sensor(scene, sensor)
        scn = Scene(sens.scene, sens.ctx.device)
        self.check_scene(scn)
        W, H = sens.width, sens.height
        y0, y1 = int(y0), int(H if y1 is None else y1)
        spp = int(spp)
        per_pass = int(self.samples_per_pass if samples_per_pass is None else samples_per_pass)
        total = spp * W * H
        if spp <= 0 or not 0 <= y0 < y1 <= H or per_pass <= 0 or total >= 2 ** 32:
            raise MtxError("render_film: bad rows / spp / samples_per_pass arguments (spp * W * H < 2^32)")
        film = Film(W, y0, y1, fid, sens.ctx.device)
        dev = film.device
        scale = float(np.float32(W * H) / np.float32(total))
        for i0 in range(0, total, per_pass):
            lanes = torch.arange(i0, min(total, i0 + per_pass), dtype=torch.int64, device=dev)
            lanes = torch.where(lanes >= 2 ** 31, lanes - 2 ** 32, lanes).to(torch.int32)  # uint32 bit patterns
            self.sample(scn, sens, Sampler(seed, lanes), film, scale)
        raw = film.raw()
        raw[..., 3] = 1.0
        return raw

    def render(self, scene, sensor=None, seed: int = 0, spp: int = 1, develop: bool = True, rfilter=None,
               samples_per_pass: int | None = None):
        """The (H, W, 3) image tensor, or the raw film with develop=False."""
        raw = self.render_film(scene, seed=seed, spp=spp, sensor=sensor, rfilter=rfilter,
                               samples_per_pass=samples_per_pass)
        if not develop:
            return raw
        return globals()["develop"](raw, _abi.RFILTER_BORDER[self.rfilter_id(scene, rfilter)])


class _Point:
    """The p, n planes a block reads from an interaction."""

    def __init__(self, p, n):
        self.p, self.n = p, n


class ParticleTracer(AdjointIntegrator):
    """Mitsuba's ``ptracer`` on the blocks: particles leave the emitters, and
    every vertex of a light path is connected to the pinhole.

    Properties (defaults are Mitsuba's): ``max_depth`` (-1 = unbounded; counts
    segments as path_test does: 1 renders the directly visible emitters only,
    2 adds emitter - surface - camera, ...), ``rr_depth`` (5: Russian roulette
    starts once a light path has that many segments), ``hide_emitters``
    (False), ``samples_per_pass`` (2^20 here; Mitsuba's default is one pass).

    Phase 1, directly visible emitters: the light path's own starting point
    (``EmitterSample``) is connected to the sensor and carries Le cos =
    weight / pi * cos. For the environment the point is instead sampled as a
    direction from the camera (``sample_emitter_direction`` at the camera
    origin), as Mitsuba does for infinite emitters: the bounding sphere need
    not contain the camera.

    Phase 2, per bounce: ``ray_intersect``; the sensor connection with its
    shadow ray; ``bsdf_eval_pdf_sample`` for the value towards the camera and
    for the continuation; the shading-normal correction of the adjoint BSDF
    (Veach, p. 155), |wi.n_s wo.n_g| / |wo.n_s wi.n_g| with wi towards the
    previous vertex, and no transport where a direction lies on different
    sides of the two normals; Russian roulette on the throughput relative to
    the emitted weight; ``spawn_ray``. The BSDF block evaluates in radiance
    mode: the only asymmetric material it can connect through is the smooth
    dielectric, whose transmitted sample carries eta_ti^2, undone here from
    ``sampled_type`` and ``eta``. A ``roughdielectric`` is refused."""

    name = "ptracer"

    def __init__(self, props=None):
        super().__init__(props)
        self.max_depth = int(self.props.get("max_depth", -1))
        self.rr_depth = int(self.props.get("rr_depth", 5))
        self.hide_emitters = bool(self.props.get("hide_emitters", False))
        if self.max_depth < -1:
            raise MtxError(f"max_depth = {self.max_depth}: expected -1 (unbounded) or a segment count >= 0")

    def check_scene(self, scene) -> None:
        for i, m in enumerate(scene.scene.materials):
            if m.type == _abi.MTX_MAT_ROUGHDIELECTRIC:
                raise MtxError(f"ptracer: material {i} is a roughdielectric: connecting a light path through it needs "
                               "the adjoint of its BSDF (its eta), which the blocks evaluate in radiance mode only")

    @staticmethod
    def _adjoint(si, wi_g, wo_local, wo_world):
        """(mask, correction) of the adjoint BSDF for the outgoing direction."""
        torch = _torch()
        wo_g = dot(si.n, wo_world)
        cwi, cwo = si.wi[2], wo_local[2]
        ok = (wi_g * cwi > 0) & (wo_g * cwo > 0)
        den = cwo * wi_g
        corr = torch.abs(div(cwi * wo_g, torch.where(ok, den, torch.ones_like(den))))
        return ok, corr

    def sample(self, scene, sensor, sampler, film, sample_scale) -> None:
        torch = _torch()
        n, dev = sampler.n, sampler.device
        max_depth = 2 ** 31 - 1 if self.max_depth < 0 else self.max_depth
        if n == 0 or max_depth == 0:
            return
        ray, weight, es = scene.sample_emitter_ray(sampler.next_2d(), sampler.next_2d())
        alive = es.emitter >= 0
        if not self.hide_emitters:
            p, nrm = es.p, es.n
            le = weight * float(np.float32(1.0 / np.pi))
            env = None
            if scene.has_environment:
                # the sky seen directly: a direction from the camera, pdf 1 / (4 pi), target two radii away
                env = es.emitter == len(scene.scene.emitters)
                cam = torch.tensor(list(sensor.scene.camera.origin), dtype=torch.float32, device=dev)
                ref = _Point(cam[:, None].expand(3, n).contiguous(), torch.zeros((3, n), device=dev))
                count = len(scene.scene.emitters) + 1
                u = sampler.next_2d()
                u = torch.stack([(u[0] + float(count - 1)) / float(count), u[1]])  # the pick: the sky
                ds, le_env = scene.sample_emitter_direction(ref, u, False, env)
                p, nrm = torch.where(env, ds.p, p), torch.where(env, ds.n, nrm)
            sd = sensor.sample_direction(p, nrm, True, alive)
            cos_l = dot(nrm, sd.d)
            geom = cos_l
            if env is not None:
                geom = torch.where(env, sd.dist * sd.dist, cos_l)
                le = torch.where(env, le_env, le)
            on = alive & sd.valid & (cos_l > 0)
            self.splat(film, sd.pos, le * (geom * sd.weight * float(sample_scale)), on)
        # the light paths: k segments so far; a connection makes it k + 1
        throughput, rel = weight, torch.ones((3, n), device=dev)
        eta = torch.ones(n, device=dev)
        o, d, maxt = ray.o, ray.d, ray.maxt
        k = 1
        while k + 1 <= max_depth and bool(alive.any()):
            si = scene.ray_intersect(o, d, maxt, alive)
            alive = alive & si.valid
            wi_g = dot(si.n, si.to_world(si.wi))
            sd = sensor.sample_direction(si.p, si.n, True, alive)
            wo = si.to_local(sd.d)
            s1, s2 = sampler.next_1d(), sampler.next_2d()
            val, _pdf, bs, bw = scene.bsdf_eval_pdf_sample(si, wo, s1, s2, alive)
            ok, corr = self._adjoint(si, wi_g, wo, sd.d)
            self.splat(film, sd.pos, throughput * val * (corr * sd.weight * float(sample_scale)),
                       alive & sd.valid & ok)
            k += 1
            if k + 1 > max_depth:
                break
            wo_w = si.to_world(bs.wo)
            ok, corr = self._adjoint(si, wi_g, bs.wo, wo_w)
            transmitted = (bs.sampled_type & 0x40) != 0  # BF_DELTA_TRANSMISSION: undo the radiance scale eta_ti^2
            bw = torch.where(transmitted, bw * (bs.eta * bs.eta), bw) * corr
            throughput, rel = throughput * bw, rel * bw
            eta = eta * bs.eta
            fmax = torch.fmax(torch.fmax(rel[0], rel[1]), rel[2])
            alive = alive & ok & (fmax > 0)
            if k >= self.rr_depth:
                q = torch.fmin(fmax * (eta * eta), fmax.new_tensor(0.95))
                alive = alive & (sampler.next_1d() < q)
                inv_q = rcp(torch.where(alive, q, torch.ones_like(q)))
                throughput, rel = throughput * inv_q, rel * inv_q
            o, d, maxt = si.spawn_ray(wo_w)


# ---------------------------------------------------------- photon mapping --

class _Visible:
    """The planes :meth:`Scene.photon_gather` reads from an interaction."""

    def __init__(self, si, material):
        self.p, self.material, self.uv, self.wi, self.sh_n, self.n = si.p, material, si.uv, si.wi, si.sh_n, si.n


class PhotonMapper(SamplingIntegrator):
    """Progressive photon mapping on the blocks (``"sppm"``): what the
    reference's sppm.py set out to do, finished in the other direction. The
    grid holds the photons of a pass and the visible points query it, so every
    pixel sums its photons in the walk's fixed order and the film is
    deterministic; the reference's grid held visible points, and scattering
    photons into them is race-ordered.

    Properties: ``max_depth`` (-1 = unbounded), ``rr_depth`` (5),
    ``hide_emitters`` (False): as ``ptracer``, counting segments;
    ``photons_per_pass`` (the film's pixel count); ``initial_radius`` (the
    radius of the scene's bounding sphere / 200); ``alpha`` (2 / 3);
    ``rfilter``.

    ``render(scene, sensor, seed, spp)`` runs spp passes. Pass i gathers with
    r_i, r_i^2 = r_0^2 prod_{k=1..i} (k - 1 + alpha) / k: the global radius
    schedule of Knaus and Zwicker's probabilistic formulation, the limit of
    SPPM's per-pixel statistics with no per-pixel state (float64 on the host,
    rounded once).

    Photon stage: the light walk of :class:`ParticleTracer` (emission,
    ``ray_intersect``, the BSDF sample with the adjoint correction and the
    eta^2 undo, Russian roulette) without the sensor connections; every hit
    on a material with a smooth lobe deposits (p, the direction back along the
    path, the throughput, the segments so far). One
    ``mtx.primitives.HashGrid`` over the deposits, resolution =
    clamp(floor(extent / (2 r_i)), 1, 1024).

    Camera stage: one jittered sample per pixel, sample i of spp in the film.
    At every vertex the emitted radiance counts where ``ptracer`` counts it
    (seen directly, or through a chain of delta lobes); a material with a
    smooth lobe adds throughput * sum / (pi r_i^2 photons_per_pass) from one
    :meth:`Scene.photon_gather`; then the BSDF sample is drawn and the path
    continues only where the sampled lobe is a delta or null lobe, with its
    weight (sppm.py:226 follows the sampled non-smooth lobe): the gather
    accounts for the smooth part in full, so a material with both is
    estimated without bias in the lobe choice. sppm.py:207's fixed depth 6 is
    ``max_depth``. The film depends on seed, spp, photons_per_pass and the
    properties alone."""

    name = "sppm"

    def __init__(self, props=None):
        super().__init__(props)
        self.max_depth = int(self.props.get("max_depth", -1))
        self.rr_depth = int(self.props.get("rr_depth", 5))
        self.hide_emitters = bool(self.props.get("hide_emitters", False))
        ppp, r0 = self.props.get("photons_per_pass", None), self.props.get("initial_radius", None)
        self.photons_per_pass = None if ppp is None else int(ppp)
        self.initial_radius = None if r0 is None else float(r0)
        self.alpha = float(self.props.get("alpha", 2.0 / 3.0))
        if self.max_depth < -1:
            raise MtxError(f"max_depth = {self.max_depth}: expected -1 (unbounded) or a segment count >= 0")
        if self.photons_per_pass is not None and self.photons_per_pass <= 0:
            raise MtxError(f"photons_per_pass = {self.photons_per_pass}: expected a positive photon count")
        if self.initial_radius is not None and not self.initial_radius > 0:
            raise MtxError(f"initial_radius = {self.initial_radius}: expected a positive radius")
        if not 0 < self.alpha <= 1:
            raise MtxError(f"alpha = {self.alpha}: expected 0 < alpha <= 1")

    def check_scene(self, scene) -> None:
        for i, m in enumerate(scene.scene.materials):
            if m.type == _abi.MTX_MAT_ROUGHDIELECTRIC:
                raise MtxError(f"sppm: material {i} is a roughdielectric: a light path through it needs the adjoint "
                               "of its BSDF (its eta), which the blocks evaluate in radiance mode only")

    def radius(self, i: int, r0: float) -> float:
        """r_i of pass i (0-based) as the float32 the kernels use."""
        r2 = float(r0) ** 2
        for k in range(1, int(i) + 1):
            r2 *= (k - 1 + self.alpha) / k
        return float(np.float32(np.sqrt(r2)))

    @staticmethod
    def _default_radius(scene) -> float:
        v = np.asarray(scene.scene.vpos, np.float64).reshape(-1, 3)
        return float(0.5 * np.linalg.norm(v.max(0) - v.min(0)) / 200.0)

    def trace_photons(self, scene, sampler, max_depth):
        """One light walk of sampler.n photons -> (p, d_p, beta_p (3, n),
        depth_p (n, int32)): the deposits, compacted in (bounce, lane) order."""
        torch = _torch()
        n, dev = sampler.n, sampler.device
        ray, weight, es = scene.sample_emitter_ray(sampler.next_2d(), sampler.next_2d())
        alive = es.emitter >= 0
        throughput, rel = weight, torch.ones((3, n), device=dev)
        eta = torch.ones(n, device=dev)
        o, d, maxt = ray.o, ray.d, ray.maxt
        P, D, B, K = [], [], [], []
        k = 1  # segments of the ray being traced; a visible point adds at least one
        while k + 1 <= max_depth and bool(alive.any()):
            si = scene.ray_intersect(o, d, maxt, alive)
            alive = alive & si.valid
            wi_w = si.to_world(si.wi)
            wi_g = dot(si.n, wi_w)
            keep = alive & ((scene.bsdf_flags(si) & BF_SMOOTH) != 0)
            P.append(si.p[:, keep])
            D.append(wi_w[:, keep])
            B.append(throughput[:, keep])
            K.append(torch.full((int(keep.sum().item()),), k, dtype=torch.int32, device=dev))
            k += 1
            if k + 1 > max_depth:
                break
            s1, s2 = sampler.next_1d(), sampler.next_2d()
            _val, _pdf, bs, bw = scene.bsdf_eval_pdf_sample(si, si.wi, s1, s2, alive)
            wo_w = si.to_world(bs.wo)
            ok, corr = ParticleTracer._adjoint(si, wi_g, bs.wo, wo_w)
            transmitted = (bs.sampled_type & 0x40) != 0  # BF_DELTA_TRANSMISSION: undo the radiance scale eta_ti^2
            bw = torch.where(transmitted, bw * (bs.eta * bs.eta), bw) * corr
            throughput, rel = throughput * bw, rel * bw
            eta = eta * bs.eta
            fmax = torch.fmax(torch.fmax(rel[0], rel[1]), rel[2])
            alive = alive & ok & (fmax > 0)
            if k >= self.rr_depth:
                q = torch.fmin(fmax * (eta * eta), fmax.new_tensor(0.95))
                alive = alive & (sampler.next_1d() < q)
                inv_q = rcp(torch.where(alive, q, torch.ones_like(q)))
                throughput, rel = throughput * inv_q, rel * inv_q
            o, d, maxt = si.spawn_ray(wo_w)
        if not P:
            z = torch.zeros((3, 0), device=dev)
            return z, z.clone(), z.clone(), torch.zeros(0, dtype=torch.int32, device=dev)
        return (torch.cat(P, 1).contiguous(), torch.cat(D, 1).contiguous(), torch.cat(B, 1).contiguous(),
                torch.cat(K).contiguous())

    def build_grid(self, p, radius):
        """The pass's hash grid over the deposit positions p (3, n), n > 0."""
        from .primitives import HashGrid

        torch = _torch()
        ext = float((torch.amax(p) - torch.amin(p)).item())
        res = int(min(max(np.floor(ext / (2.0 * radius)) if radius > 0 else 1, 1), 1024))
        return HashGrid(p, res)

    def gather_pass(self, scene, sampler, ray, grid, photons, radius, n_photons, max_depth):
        """The camera stage of one pass -> L (3, N)."""
        torch = _torch()
        n, dev = sampler.n, sampler.device
        L = torch.zeros((3, n), device=dev)
        thr = torch.ones((3, n), device=dev)
        active = torch.ones(n, dtype=torch.bool, device=dev)
        o, d, maxt = ray.o, ray.d, ray.maxt
        scale = float(1.0 / (np.pi * float(radius) ** 2 * float(n_photons)))
        depth = 1  # segments of the camera path once this ray has hit
        while depth <= max_depth and bool(active.any()):
            si = scene.ray_intersect(o, d, maxt, active)
            if depth > 1 or not self.hide_emitters:
                L = L + thr * scene.emitter_eval(si, active)
            active = active & si.valid
            if depth + 1 > max_depth:
                break
            smooth = active & ((scene.bsdf_flags(si) & BF_SMOOTH) != 0)
            if grid is not None and bool(smooth.any()):
                vis = _Visible(si, torch.where(smooth, si.material, torch.full_like(si.material, -1)))
                total, _cnt = scene.photon_gather(grid, vis, depth, radius, photons[0], photons[1], photons[2],
                                                  max_depth)
                L = L + thr * total * scale
            s1, s2 = sampler.next_1d(), sampler.next_2d()
            _val, _pdf, bs, bw = scene.bsdf_eval_pdf_sample(si, si.wi, s1, s2, active)
            fmax = torch.fmax(torch.fmax(bw[0], bw[1]), bw[2])
            active = active & ((bs.sampled_type & BF_DELTA) != 0) & (fmax > 0)
            thr = thr * bw
            depth += 1
            if depth >= self.rr_depth:
                tmax = torch.fmax(torch.fmax(thr[0], thr[1]), thr[2])
                q = torch.fmin(tmax, tmax.new_tensor(0.95))
                active = active & (sampler.next_1d() < q)
                thr = thr * rcp(torch.where(active, q, torch.ones_like(q)))
            o, d, maxt = si.spawn_ray(si.to_world(bs.wo))
        return L

    def render_film(self, scene, seed: int = 0, spp: int = 1, sensor=None, rfilter=None):
        """The raw film tensor (H + 2b, W + 2b, 4) after spp passes."""
        torch = _torch()
        fid = self.rfilter_id(scene, rfilter)
        sens = Sensor(scene, sensor)
        scn = Scene(sens.scene, sens.ctx.device)
        self.check_scene(scn)
        W, H = sens.width, sens.height
        spp = int(spp)
        n_px = W * H
        n_ph = n_px if self.photons_per_pass is None else self.photons_per_pass
        if spp <= 0 or spp * max(n_px, n_ph) >= 2 ** 32:
            raise MtxError("render_film: spp > 0 and spp * max(pixels, photons_per_pass) < 2^32 expected")
        r0 = self._default_radius(scn) if self.initial_radius is None else self.initial_radius
        max_depth = 2 ** 31 - 1 if self.max_depth < 0 else self.max_depth
        film = Film(W, 0, H, fid, sens.ctx.device)
        dev = film.device

        def lanes_of(a):
            a = a & 0xffffffff
            return torch.where(a >= 2 ** 31, a - 2 ** 32, a).to(torch.int32)  # uint32 bit patterns

        pix = torch.arange(n_px, dtype=torch.int64, device=dev)
        px, py = (pix % W).to(torch.float32), (pix // W).to(torch.float32)
        for i in range(spp):
            r = self.radius(i, r0)
            grid, photons = None, None
            if max_depth >= 2:
                ids = torch.arange(i * n_ph, (i + 1) * n_ph, dtype=torch.int64, device=dev)
                # the photons' streams: another seed than the camera samples' (lane ids overlap)
                p, d_p, beta_p, depth_p = self.trace_photons(scn, Sampler((int(seed) + 0x9e3779b9) & 0xffffffff,
                                                                          lanes_of(ids)), max_depth)
                if p.shape[1]:
                    grid, photons = self.build_grid(p, r), (d_p, beta_p, depth_p)
            sampler = Sampler(seed, lanes_of(pix * spp + i))
            u = sampler.next_2d()  # the film jitter
            pos = torch.stack([px + u[0], py + u[1]])
            L = self.gather_pass(scn, sampler, sens.sample_ray(pos), grid, photons, r, n_ph, max_depth)
            film.put(pos, L.contiguous(), spp_total=spp, sample_offset=i, pixel_major_spp=1, px0=0)
        return film.raw()

    def render(self, scene, sensor=None, seed: int = 0, spp: int = 1, develop: bool = True, rfilter=None):
        """The (H, W, 3) image tensor, or the raw film with develop=False."""
        raw = self.render_film(scene, seed=seed, spp=spp, sensor=sensor, rfilter=rfilter)
        if not develop:
            return raw
        return globals()["develop"](raw, _abi.RFILTER_BORDER[self.rfilter_id(scene, rfilter)])


# ------------------------------------------------- bidirectional connections --

_PATH_PLANES = (("p", 3, "float32"), ("n", 3, "float32"), ("sh_n", 3, "float32"), ("wi", 3, "float32"),
                ("uv", 2, "float32"), ("material", None, "int32"), ("emitter", None, "int32"),
                ("beta", 3, "float32"), ("pdf_fwd", None, "float32"), ("pdf_rev", None, "float32"),
                ("delta", None, "uint8"))


def _path_shape(depth, comps, n):
    return (depth, n) if comps is None else (depth, comps, n)


class PathVertices:
    """A vertex store (``mtx_path_planes``, mtx_core/bdpt.h): one subpath of at
    most `depth` vertices per lane, every plane coalesced over lanes. ``len``
    (N, int32); ``p``, ``n``, ``sh_n``, ``wi``, ``beta`` (D, 3, N); ``uv``
    (D, 2, N); ``material``, ``emitter`` (D, N, int32, -1 = none);
    ``pdf_fwd``, ``pdf_rev`` (D, N) area-measure densities; ``delta`` (D, N,
    uint8). All zero (no emitter, no material) until recorded."""

    def __init__(self, device, depth: int, n: int):
        torch = _torch()
        depth, n = int(depth), int(n)
        if depth < 2 or n < 0:
            raise MtxError(f"PathVertices: depth {depth} (at least 2 vertices) or lane count {n}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise MtxError(f"PathVertices: device {self.device}; the blocks take CUDA tensors")
        self.depth, self.lanes = depth, n
        self.len = torch.zeros(n, dtype=torch.int32, device=self.device)
        for k, c, dt in _PATH_PLANES:
            t = torch.zeros(_path_shape(depth, c, n), dtype=getattr(torch, dt), device=self.device)
            if k in ("material", "emitter"):
                t -= 1
            setattr(self, k, t)

    def record(self, k: int, si, beta, pdf_fwd, delta, active) -> None:
        """Append vertex k = the interaction `si` (p, n, sh_n, wi, uv,
        material, emitter planes) with the arriving throughput beta (3, N),
        its forward area density pdf_fwd (N) and the delta flag of the lobe
        sampled at it (N, bool) to the lanes that are on; ``len`` becomes
        k + 1 there and nothing changes elsewhere."""
        torch = _torch()
        k = int(k)
        if not 0 <= k < self.depth:
            raise MtxError(f"record: vertex {k} outside a store of depth {self.depth}")
        n, dev = self.lanes, self.device
        for name in ("p", "n", "sh_n", "wi"):
            _f32(f"record: si.{name}", getattr(si, name), 3, n, dev)
        _f32("record: si.uv", si.uv, 2, n, dev)
        _i32("record: si.material", si.material, n, dev)
        _i32("record: si.emitter", si.emitter, n, dev)
        _f32("record: beta", beta, 3, n, dev)
        _f32("record: pdf_fwd", pdf_fwd, None, n, dev)
        _arg("record: delta", delta, (torch.bool, torch.uint8), None, n, dev)
        _arg("record: active", active, (torch.bool, torch.uint8), None, n, dev)
        on = active.bool()
        for name, src in (("p", si.p), ("n", si.n), ("sh_n", si.sh_n), ("wi", si.wi), ("uv", si.uv),
                          ("material", si.material), ("emitter", si.emitter), ("beta", beta), ("pdf_fwd", pdf_fwd),
                          ("delta", delta.to(torch.uint8))):
            plane = getattr(self, name)[k]
            plane.copy_(torch.where(on, src, plane))
        self.len.copy_(torch.where(on, torch.full_like(self.len, k + 1), self.len))

    def set_pdf_rev(self, k: int, pdf) -> None:
        """The stored reverse density of vertex k (N): with which it would
        have been generated from vertex k + 1."""
        k = int(k)
        if not 0 <= k < self.depth:
            raise MtxError(f"set_pdf_rev: vertex {k} outside a store of depth {self.depth}")
        _f32("set_pdf_rev: pdf", pdf, None, self.lanes, self.device)
        self.pdf_rev[k].copy_(pdf)

    def host(self) -> dict:
        """The planes as numpy arrays (the layout :func:`bdpt_host` takes)."""
        out = {k: getattr(self, k).cpu().numpy() for k, _, _ in _PATH_PLANES}
        out["len"] = self.len.cpu().numpy()
        return out


def _check_store(name, store):
    """Validate a device store's planes; returns its ctypes mirror."""
    torch = _torch()
    if not isinstance(store, PathVertices):
        raise MtxError(f"{name}: expected a blocks.PathVertices, got {type(store).__name__}")
    D, n, dev = store.depth, store.lanes, store.device
    planes = [("len", None, "int32")] + list(_PATH_PLANES)
    ptrs = {}
    for k, c, dt in planes:
        t = getattr(store, k)
        if not isinstance(t, torch.Tensor):
            raise MtxError(f"{name}.{k}: expected a torch CUDA tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise MtxError(f"{name}.{k}: a host tensor (device {t.device}); the blocks take CUDA tensors")
        if t.device != dev:
            raise MtxError(f"{name}.{k}: on {t.device}, the store is on {dev}")
        if t.dtype != getattr(torch, dt):
            raise MtxError(f"{name}.{k}: dtype {t.dtype}, expected torch.{dt}")
        want = (n,) if k == "len" else _path_shape(D, c, n)
        if tuple(t.shape) != want:
            raise MtxError(f"{name}.{k}: shape {tuple(t.shape)}, expected {want}")
        if not t.is_contiguous():
            raise MtxError(f"{name}.{k}: not contiguous")
        ptrs[k] = t.data_ptr()
    return _abi.PathPlanes(D, *[ptrs[k] for k, _, _ in planes])


def _strategy(fn, s, t, max_depth, depth):
    """(s, t, single) for the ABI; refusals name the cause."""
    if (s is None) != (t is None):
        raise MtxError(f"{fn}: s and t: give both (one strategy) or neither (their sum)")
    if not isinstance(max_depth, (int, np.integer)) or isinstance(max_depth, bool) or max_depth < 1:
        raise MtxError(f"{fn}: max_depth = {max_depth!r}: expected a segment count >= 1")
    if s is None:
        return -1, -1, False
    s, t = int(s), int(t)
    if t in (0, 1):
        raise MtxError(f"{fn}: t = {t}: only strategies with t >= 2 exist (t = 1 splats onto the film)")
    if s < 0 or t < 0 or s > depth or t > depth:
        raise MtxError(f"{fn}: strategy (s = {s}, t = {t}) outside the stores' depth {depth}")
    return s, t, True


def connect_subpaths(scene, camera, light, max_depth, s=None, t=None, mis=True, test_visibility=True, active=None):
    """Join the camera subpaths and the light subpaths of two
    :class:`PathVertices` lane by lane in one launch (mtx_core/bdpt.h has the
    conventions). Without s, t: L (3, N), the sum over every strategy (s, t),
    t >= 2, of s + t - 1 <= max_depth segments, each weighed by the power
    heuristic (``mis``; else weight 1) and, with ``test_visibility``, zero
    where the connection's shadow ray is occluded. With s and t: ``(L,
    weight)`` of that strategy alone."""
    fn = "connect_subpaths"
    if not isinstance(scene, Scene):
        raise MtxError(f"{fn}: scene: expected a blocks.Scene, got {type(scene).__name__}")
    cam, lit = _check_store(f"{fn}: camera", camera), _check_store(f"{fn}: light", light)
    if camera.depth != light.depth:
        raise MtxError(f"{fn}: depth mismatch: camera holds {camera.depth} vertices per lane, light {light.depth}")
    if camera.lanes != light.lanes:
        raise MtxError(f"{fn}: light: {light.lanes} lanes, the camera store has N = {camera.lanes}")
    if camera.device != light.device:
        raise MtxError(f"{fn}: light: on {light.device}, the camera store is on {camera.device}")
    n, dev = camera.lanes, camera.device
    s_, t_, single = _strategy(fn, s, t, max_depth, camera.depth)
    _, am = _mask(f"{fn}: active", active, n, dev)
    L = _empty(dev, 3, n)
    w = _empty(dev, None, n) if single else None
    if n:
        flags = (_abi.MTX_BDPT_MIS if mis else 0) | (_abi.MTX_BDPT_VISIBILITY if test_visibility else 0)
        check(lib().mtx_blocks_bdpt_connect_dev(scene._call(dev), n, C.byref(cam), C.byref(lit), s_, t_,
                                                int(max_depth), flags, am, L.data_ptr(),
                                                w.data_ptr() if single else None), "mtx_blocks_bdpt_connect_dev")
    return (L, w) if single else L


def bdpt_host(scene, camera: dict, light: dict, max_depth, s=None, t=None, mis=True, flags=None, want_weight=None):
    """The CPU twin of :func:`connect_subpaths` (mtx_blocks_bdpt_host): needs
    no GPU and tests no visibility. ``camera`` / ``light``: dictionaries of
    numpy planes in :class:`PathVertices`' layout (``PathVertices.host()``).
    Returns L (3, N), or (L, weight) for one strategy. ``flags`` /
    ``want_weight`` override what ``mis`` and the strategy imply (the
    refusals' tests)."""
    fn = "bdpt_host"
    keep, mirrors, depth, n = [], [], None, None
    for name, store in (("camera", camera), ("light", light)):
        ln = np.ascontiguousarray(store["len"], np.int32)
        D = int(np.shape(store["pdf_fwd"])[0])
        if n is None:
            n = len(ln)
        ptrs = [ln]
        for k, c, dt in _PATH_PLANES:
            a = np.ascontiguousarray(store[k], getattr(np, dt))
            if a.shape != _path_shape(D, c, n):
                raise MtxError(f"{fn}: {name}.{k}: shape {a.shape}, expected {_path_shape(D, c, n)}")
            ptrs.append(a)
        if len(ln) != n:
            raise MtxError(f"{fn}: {name}.len: {len(ln)} lanes, the call has N = {n}")
        keep.append(ptrs)
        mirrors.append(_abi.PathPlanes(D, *[a.ctypes.data for a in ptrs]))
        depth = D if depth is None else depth
    single = s is not None
    L = np.zeros((3, n), np.float32)
    w = np.zeros(n, np.float32) if (single if want_weight is None else want_weight) else None
    if flags is None:
        flags = _abi.MTX_BDPT_MIS if mis else 0
    desc = _mtx_scene(scene).desc()
    check(lib().mtx_blocks_bdpt_host(C.byref(desc), n, C.byref(mirrors[0]), C.byref(mirrors[1]),
                                     -1 if s is None else int(s), -1 if t is None else int(t), int(max_depth),
                                     int(flags), L.ctypes.data, None if w is None else w.ctypes.data),
          "mtx_blocks_bdpt_host")
    return (L, w) if w is not None else L


class _VertexPoint:
    """A vertex that is no surface hit (the pinhole, an emitter sample) in the
    planes :meth:`PathVertices.record` reads."""

    def __init__(self, p, n, emitter=None):
        torch = _torch()
        cnt, dev = p.shape[1], p.device
        self.p, self.n, self.sh_n = p, n, n
        self.wi = torch.zeros((3, cnt), device=dev)
        self.uv = torch.zeros((2, cnt), device=dev)
        self.material = torch.full((cnt,), -1, dtype=torch.int32, device=dev)
        self.emitter = self.material.clone() if emitter is None else emitter


class BidirectionalPathTracer(SamplingIntegrator):
    """A bidirectional path tracer on the blocks (``"bdpt"``): per sample a
    camera subpath and a light subpath are recorded into two
    :class:`PathVertices` and joined by one :func:`connect_subpaths` launch,
    which evaluates every strategy (s, t) with t >= 2 and weighs them with the
    power heuristic.

    Properties: ``max_depth`` (16, the reference's default; >= 1; counts
    segments as path_test does), ``rr_depth`` (accepted for the reference's
    dictionaries and unused: subpaths are not terminated by Russian roulette,
    which changes the variance and not the expectation), ``rfilter``.

    Not covered: the t = 1 strategies (light paths splatted onto the film:
    :class:`ParticleTracer`), so a pixel that sees the scene only through a
    chain of delta surfaces from the light's side gets what its camera paths
    find; environments and ``roughdielectric`` materials are refused."""

    name = "bdpt"

    def __init__(self, props=None):
        super().__init__(props)
        md = self.props.get("max_depth", 16)
        if isinstance(md, bool) or not isinstance(md, (int, np.integer, float)) or not np.isfinite(md) or md < 1 \
                or int(md) != md:
            raise MtxError(f"bdpt: max_depth = {md!r}: expected a finite segment count >= 1")
        self.max_depth = int(md)
        self.rr_depth = int(self.props.get("rr_depth", 5))  # unused: no Russian roulette

    def check_scene(self, scene) -> None:
        sc = _mtx_scene(scene)
        if getattr(sc, "env_radiance", None) is not None:
            raise MtxError("bdpt: the scene has a constant environment: an infinite emitter needs its own densities "
                           "in the weights, which the connection kernel does not have")
        for i, m in enumerate(sc.materials):
            if m.type == _abi.MTX_MAT_ROUGHDIELECTRIC:
                raise MtxError(f"bdpt: material {i} is a roughdielectric: connecting a light path through it needs "
                               "the adjoint of its BSDF (its eta), which the blocks evaluate in radiance mode only")

    # ------------------------------------------------------------ recording --
    @staticmethod
    def _area(pdf_dir, p_from, p_to, n_to):
        """solid-angle density -> area density at p_to: pdf * |cos| / d^2 (0 where the points coincide)."""
        torch = _torch()
        rel = p_to - p_from
        d2 = (rel * rel).sum(0)
        some = d2 > 0
        d2s = torch.where(some, d2, torch.ones_like(d2))
        cos = torch.abs((n_to * rel).sum(0)) / torch.sqrt(d2s)
        return torch.where(some, pdf_dir * cos / d2s, torch.zeros_like(d2))

    def _walk(self, scene, sampler, store, k0, last, o, d, maxt, alive, beta, pdf_dir, prev_p, prev_n, adjoint):
        """Record vertices k0 .. last of a subpath that leaves (prev_p,
        prev_n) along the ray with the solid-angle density pdf_dir. Returns
        the validity of the first hit."""
        torch = _torch()
        first = None
        k = k0
        while k <= last and bool(alive.any()):
            si = scene.ray_intersect(o, d, maxt, alive)
            alive = alive & si.valid
            if first is None:
                first = alive
            pdf_fwd = self._area(pdf_dir, prev_p, si.p, si.n)
            if k == last:  # nothing is sampled at the last vertex
                store.record(k, si, beta, pdf_fwd, torch.zeros_like(alive), alive)
                break
            s1, s2 = sampler.next_1d(), sampler.next_2d()
            _v, _p, bs, bw = scene.bsdf_eval_pdf_sample(si, si.wi, s1, s2, alive)
            store.record(k, si, beta, pdf_fwd, (bs.sampled_type & BF_DELTA) != 0, alive)
            # the reverse density of vertex k - 1: wi and wo exchanged at this vertex
            rev = SurfaceInteraction.__new__(SurfaceInteraction)
            rev.material, rev.uv, rev.wi = si.material, si.uv, bs.wo
            _v, pdf_rev, _bs, _w = scene.bsdf_eval_pdf_sample(rev, si.wi, s1, s2, alive)
            store.set_pdf_rev(k - 1, torch.where(alive, self._area(pdf_rev, si.p, prev_p, prev_n),
                                                 torch.zeros_like(pdf_rev)))
            wo_w = si.to_world(bs.wo)
            if adjoint:
                wi_g = dot(si.n, si.to_world(si.wi))
                ok, corr = ParticleTracer._adjoint(si, wi_g, bs.wo, wo_w)
                transmitted = (bs.sampled_type & 0x40) != 0  # BF_DELTA_TRANSMISSION: undo the radiance scale
                bw = torch.where(transmitted, bw * (bs.eta * bs.eta), bw) * corr
                alive = alive & ok
            beta = beta * bw
            alive = alive & (bs.pdf > 0) & (torch.fmax(torch.fmax(beta[0], beta[1]), beta[2]) > 0)
            o, d, maxt = si.spawn_ray(wo_w)
            pdf_dir, prev_p, prev_n = bs.pdf, si.p, si.n
            k += 1
        return first if first is not None else alive

    def record_camera(self, scene, sampler, ray, store, active=None):
        """z_0 = the pinhole, z_1 .. the hits along `ray` and its BSDF-sampled
        continuations, up to max_depth segments. Returns si_1.valid."""
        torch = _torch()
        n, dev = sampler.n, sampler.device
        on = torch.ones(n, dtype=torch.bool, device=dev) if active is None else active.bool()
        origin = torch.tensor(list(scene.scene.camera.origin), dtype=torch.float32, device=dev)
        p0 = origin[:, None].expand(3, n).contiguous()
        zero, one = torch.zeros(n, device=dev), torch.ones((3, n), device=dev)
        store.record(0, _VertexPoint(p0, torch.zeros((3, n), device=dev)), one, zero, torch.zeros_like(on), on)
        return self._walk(scene, sampler, store, 1, min(self.max_depth, store.depth - 1), ray.o, ray.d, ray.maxt, on,
                          one, zero, p0, torch.zeros((3, n), device=dev), False)

    def record_light(self, scene, sampler, store, active=None) -> None:
        """y_0 = the emitter sample of ``sample_emitter_ray``, y_1 .. the hits
        of the emitted ray and its continuations with the particle tracer's
        adjoint handling; y_{s-1} exists for s <= max_depth - 1."""
        torch = _torch()
        n, dev = sampler.n, sampler.device
        ray, weight, es = scene.sample_emitter_ray(sampler.next_2d(), sampler.next_2d(), active)
        alive = es.emitter >= 0
        ems = scene.scene.emitters
        if len(ems) == 0:
            return
        inv_area = torch.tensor([float(e.inv_area) for e in ems], dtype=torch.float32, device=dev)
        pdf_pos = inv_area[es.emitter.clamp(0, len(ems) - 1).long()] * float(np.float32(1.0) / np.float32(len(ems)))
        le = weight * float(np.float32(1.0 / np.pi))  # radiance / pdf_pos
        store.record(0, _VertexPoint(es.p, es.n, es.emitter), le, pdf_pos, torch.zeros_like(alive), alive)
        last = min(self.max_depth - 2, store.depth - 1)
        if last < 1:
            return
        cos0 = torch.clamp((es.n * ray.d).sum(0), min=0.0) * float(np.float32(1.0 / np.pi))
        self._walk(scene, sampler, store, 1, last, ray.o, ray.d, ray.maxt, alive, weight, cos0, es.p, es.n, True)

    def connect(self, scene, camera, light):
        """The one launch that joins the two stores; a subclass may pick a strategy."""
        return connect_subpaths(scene, camera, light, self.max_depth)

    def sample(self, scene, sampler, ray, medium=None, active=None):
        n, dev = sampler.n, sampler.device
        cam = PathVertices(dev, self.max_depth + 1, n)
        lit = PathVertices(dev, self.max_depth + 1, n)
        valid = self.record_camera(scene, sampler, ray, cam, active)
        self.record_light(scene, sampler, lit, active)
        return self.connect(scene, cam, lit), valid, []

    def render_film(self, scene, seed: int = 0, spp: int = 1, y0: int = 0, y1: int | None = None,
                    spp_total: int | None = None, sample_offset: int = 0, sensor=None, rfilter=None,
                    max_lanes: int | None = None):
        """The inherited render loop; ``max_lanes`` defaults to 2^20 lanes per
        pass: the two stores of max_depth + 1 vertices take about 0.2 KB per
        vertex and lane."""
        self.check_scene(scene)
        return super().render_film(scene, seed=seed, spp=spp, y0=y0, y1=y1, spp_total=spp_total,
                                   sample_offset=sample_offset, sensor=sensor, rfilter=rfilter,
                                   max_lanes=1 << 20 if max_lanes is None else max_lanes)
