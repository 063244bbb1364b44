"""Ray queries: what a ray of the caller's hits (rtw_cast_*, rtw_occluded_*, include/rtw.h).

A `RayCaster` answers closest-hit and occlusion queries for arbitrary rays against one uploaded world: a pick under
the cursor, a visibility or shadow test between two points, an ambient-occlusion or light-map bake, a probe of one
bounce.  The hit is the reference's `Scene::hit` over [t_start, t_end), bit for bit: the walk is the first-hit AOV
pass's, on the reference tree.  Directions need not be unit length; `times` moves Animation leaves and nothing else.
Volume leaves draw from a stream of the ray's own, (seed, ray index, stream), so a batch is reproducible.
`RayCaster.radiance` goes on from there (rtw_radiance_*): the reference's ray_color along every ray --
the whole path -- `samples` times, each sample from the stream (seed, ray index, sample index), and their mean.

numpy arrays in give numpy arrays out (staged through the device, synchronous).  torch tensors on the caster's
device give device tensors out with no host copy, asynchronously on torch's current stream; the `*_device` methods
are that path by name, as `AovAccumulator.albedo_device` is.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._native import check, lib
from .rendering import DEFAULT_SEED, DeviceWorld, RenderMode
from .world import World

RAY_WORDS = 8   # rtw_ray: origin, time, direction, t_end
HIT_WORDS = 12  # rtw_hit: t, leaf, position, normal, uv, front_face, material


@dataclass
class CastResult:
    """The closest hits of a batch, arrays (or device tensors) over the rays: hit (bool), t (the ray's own t_end on
    a miss), leaf and material (int32, -1 on a miss), position and normal (n, 3), uv (n, 2), front_face (bool), and
    albedo (n, 3) when asked for (1 on a miss and on a dielectric)."""

    hit: object
    t: object
    leaf: object
    position: object
    normal: object
    uv: object
    front_face: object
    material: object
    albedo: object = None

    def __len__(self) -> int:
        return int(self.t.shape[0])


def _cast_result(hits, ints, albedo) -> CastResult:
    """The (n, HIT_WORDS) float32 records (an array or a device tensor) and their int32 view as a CastResult."""
    return CastResult(hit=ints[:, 1] >= 0, t=hits[:, 0], leaf=ints[:, 1], position=hits[:, 2:5], normal=hits[:, 5:8],
                      uv=hits[:, 8:10], front_face=ints[:, 10] != 0, material=ints[:, 11], albedo=albedo)


def _is_tensor(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")


def _vectors(name: str, a) -> np.ndarray:
    """An (n, 3) or (3,) array of real numbers as float32 (n, 3) / (1, 3)."""
    arr = np.asarray(a)
    if arr.dtype.kind not in "fiu":
        raise ValueError(f"{name}: dtype {arr.dtype} is not a real number type")
    if arr.ndim == 1 and arr.shape == (3,):
        arr = arr[None]
    if arr.ndim != 2 or arr.shape[1] != 3:
        raise ValueError(f"{name}: shape {np.asarray(a).shape} is not (n, 3) or (3,)")
    return arr.astype(np.float32, copy=False)


def _scalars(name: str, a, default: float) -> np.ndarray:
    """A scalar or an (n,) array of real numbers as float32 (n,) / (1,)."""
    arr = np.asarray(default if a is None else a)
    if arr.dtype.kind not in "fiu":
        raise ValueError(f"{name}: dtype {arr.dtype} is not a real number type")
    if arr.ndim > 1:
        raise ValueError(f"{name}: shape {arr.shape} is not (n,) or a scalar")
    return arr.reshape(-1).astype(np.float32, copy=False)


def _count(parts: dict) -> int:
    """The batch's ray count: origins' and directions', or the scalars' when both are one vector; every argument
    holds that many rays or one (broadcast)."""
    sizes = [int(v.shape[0]) for v in parts.values()]
    n = 0 if 0 in sizes else max(sizes[:2])
    if n == 1:
        n = max(sizes)
    for name, v in parts.items():
        if int(v.shape[0]) not in (1, n):
            raise ValueError(f"{name}: holds {int(v.shape[0])} rays, the batch has {n}")
    return n


def pack_rays(origins, directions, times=None, t_end=None) -> np.ndarray:
    """The rays as the (n, 8) float32 array of rtw_ray records: origin, time, direction, t_end.  (n, 3) arrays, a
    (3,) vector or a scalar is broadcast over the batch; times defaults to 0 and t_end to +inf.  Raises ValueError
    naming the argument for a shape or dtype it cannot take."""
    parts = {"origins": _vectors("origins", origins), "directions": _vectors("directions", directions),
             "times": _scalars("times", times, 0.0), "t_end": _scalars("t_end", t_end, math.inf)}
    n = _count(parts)
    rays = np.empty((n, RAY_WORDS), np.float32)
    rays[:, 0:3] = parts["origins"]
    rays[:, 3] = parts["times"]
    rays[:, 4:7] = parts["directions"]
    rays[:, 7] = parts["t_end"]
    return rays


def _params(t_start, seed, stream, albedo: bool) -> N.CastParams:
    try:
        t_start = float(t_start)
    except (TypeError, ValueError):
        raise ValueError(f"t_start: {t_start!r} is not a number") from None
    if not math.isfinite(t_start):
        raise ValueError(f"t_start: {t_start} is not finite")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed: {seed!r} is not an integer in 0 .. 2^64 - 1")
    if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < 1 << 32:
        raise ValueError(f"stream: {stream!r} is not an integer in 0 .. 2^32 - 1")
    return N.CastParams(N.CAST_ALBEDO if albedo else 0, t_start, int(seed), int(stream), 0)


@dataclass
class RadianceResult:
    """The radiance of a batch, arrays (or device tensors) over the rays: mean (n, 3); kept (n,) with `finite`, the
    samples the mean runs over (uint32; int32 as a device tensor); samples (n, S, 3) with `per_sample`."""

    mean: object
    kept: object = None
    samples: object = None

    def __len__(self) -> int:
        return int(self.mean.shape[0])


_MAX_ITEMS = (1 << 31) - 1  # rays * samples of one rtw_radiance_samples_device call


def _integer(name: str, v, lo: int, hi: int, words: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{name}: {v!r} is not an integer in {words}")
    return int(v)


def _radiance_params(samples, max_depth, mode, seed, first_sample, first_ray, finite, max_bytes, n: int) -> N.RadianceParams:
    """rtw_radiance_params of a batch of n rays; ValueError naming the argument."""
    samples = _integer("samples", samples, 1, _MAX_ITEMS, "1 .. 2^31 - 1")
    max_depth = _integer("max_depth", max_depth, -(1 << 31), (1 << 31) - 1, "-2^31 .. 2^31 - 1")
    try:
        mode = RenderMode(mode)
    except (TypeError, ValueError):
        raise ValueError(f"mode: {mode!r} is not a RenderMode") from None
    seed = _integer("seed", seed, 0, (1 << 64) - 1, "0 .. 2^64 - 1")
    first_sample = _integer("first_sample", first_sample, 0, (1 << 32) - 1, "0 .. 2^32 - 1")
    if first_sample + samples > 1 << 32:
        raise ValueError(f"first_sample: {first_sample} + {samples} samples runs past 2^32")
    first_ray = _integer("first_ray", first_ray, 0, (1 << 32) - 1, "0 .. 2^32 - 1")
    if first_ray + n > 1 << 32:
        raise ValueError(f"first_ray: {first_ray} + {n} rays runs past 2^32")
    if not isinstance(finite, (bool, np.bool_)):
        raise ValueError(f"finite: {finite!r} is not a bool")
    _integer("max_bytes", max_bytes, 1, (1 << 63) - 1, "1 .. 2^63 - 1")
    return N.RadianceParams(N.RADIANCE_FINITE if finite else 0, int(mode), max_depth, samples, first_sample, first_ray, seed)


class RayCaster:
    """Closest-hit, occlusion and radiance queries against one World on one GPU.

    world: a `World` (uploaded here) or a `DeviceWorld` (shared with frames and accumulators, which the queries
    leave alone: they use none of the world's scratch)."""

    def __init__(self, world: World | DeviceWorld, device: int = 0):
        self.dworld = world if isinstance(world, DeviceWorld) else DeviceWorld(world, device)
        self.device = self.dworld.device

    def release(self) -> None:
        """Releases the world's device state (a shared DeviceWorld's too)."""
        self.dworld.release()

    def _handle(self):
        return self.dworld._h  # (None once released: the library refuses it)

    def _stream(self) -> int:
        import torch

        return torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream

    # ---- device tensors -------------------------------------------------------------------------
    def _pack_device(self, origins, directions, times, t_end):
        import torch

        dev = torch.device("cuda", self.device)

        def tensor(name, a, width, default=None):
            if a is None:
                a = default
            if _is_tensor(a):
                if a.device != dev:
                    raise ValueError(f"{name}: the tensor is on {a.device}, the caster on {dev}")
                if a.dtype != torch.float32:
                    raise ValueError(f"{name}: dtype {a.dtype} is not torch.float32")
            else:  # a scalar or a (3,) vector to broadcast
                arr = np.asarray(a)
                if arr.dtype.kind not in "fiu":
                    raise ValueError(f"{name}: dtype {arr.dtype} is not a real number type")
                if arr.shape not in (((3,), (1, 3)) if width == 3 else ((), (1,))):
                    raise ValueError(f"{name}: beside device tensors, give a device tensor or "
                                     f"{'a (3,) vector' if width == 3 else 'a scalar'}")
                a = torch.from_numpy(np.ascontiguousarray(arr, np.float32).reshape(-1)).to(dev)
            if width == 3:
                if a.ndim == 1 and tuple(a.shape) == (3,):
                    a = a[None]
                if a.ndim != 2 or a.shape[1] != 3:
                    raise ValueError(f"{name}: shape {tuple(a.shape)} is not (n, 3) or (3,)")
                return a
            if a.ndim > 1:
                raise ValueError(f"{name}: shape {tuple(a.shape)} is not (n,) or a scalar")
            return a.reshape(-1)

        parts = {"origins": tensor("origins", origins, 3), "directions": tensor("directions", directions, 3),
                 "times": tensor("times", times, 1, 0.0), "t_end": tensor("t_end", t_end, 1, math.inf)}
        n = _count(parts)
        rays = torch.empty((n, RAY_WORDS), dtype=torch.float32, device=dev)
        rays[:, 0:3] = parts["origins"]
        rays[:, 3] = parts["times"]
        rays[:, 4:7] = parts["directions"]
        rays[:, 7] = parts["t_end"]
        return rays

    def cast_device(self, origins, directions, times=None, t_end=None, *, t_start: float = 0.001,
                    seed: int = DEFAULT_SEED, stream: int = 0, albedo: bool = False) -> CastResult:
        """`cast` for float32 tensors on the caster's device (scalars and (3,) vectors are broadcast): device
        tensors out, no host copy, asynchronous on torch's current stream."""
        import torch

        p = _params(t_start, seed, stream, albedo)
        rays = self._pack_device(origins, directions, times, t_end)
        n = int(rays.shape[0])
        hits = torch.empty((n, HIT_WORDS), dtype=torch.float32, device=rays.device)
        alb = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if albedo else None
        if n:  # (an empty tensor has no storage to point at)
            check(lib().rtw_cast_device(self._handle(), C.byref(p), C.c_void_p(rays.data_ptr()), n, C.c_void_p(hits.data_ptr()),
                                        C.c_void_p(alb.data_ptr()) if albedo else None, C.c_void_p(self._stream() or 0)))
        return _cast_result(hits, hits.view(torch.int32), alb)

    def occluded_device(self, origins, directions, times=None, t_end=None, *, t_start: float = 0.001,
                        seed: int = DEFAULT_SEED, stream: int = 0, albedo: bool = False):
        """`occluded` for tensors on the caster's device: a bool device tensor."""
        import torch

        if albedo:
            raise ValueError("albedo: an occlusion query has no hit to read it at")
        p = _params(t_start, seed, stream, False)
        rays = self._pack_device(origins, directions, times, t_end)
        n = int(rays.shape[0])
        out = torch.empty(n, dtype=torch.uint8, device=rays.device)
        if n:
            check(lib().rtw_occluded_device(self._handle(), C.byref(p), C.c_void_p(rays.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(self._stream() or 0)))
        return out != 0

    # ---- numpy in, numpy out; tensors on the device go the way above -----------------------------
    def cast(self, origins, directions, times=None, t_end=None, *, t_start: float = 0.001, seed: int = DEFAULT_SEED,
             stream: int = 0, albedo: bool = False) -> CastResult:
        """The closest hit of every ray over [t_start, t_end).  origins and directions (n, 3) (a (3,) vector is
        broadcast), times and t_end (n,) or scalars (default 0 and +inf).  Raises ValueError naming the argument
        for a shape or dtype it cannot take, RtwError for what the library refuses."""
        if any(_is_tensor(a) for a in (origins, directions, times, t_end)):
            return self.cast_device(origins, directions, times, t_end, t_start=t_start, seed=seed, stream=stream, albedo=albedo)
        p = _params(t_start, seed, stream, albedo)
        rays = pack_rays(origins, directions, times, t_end)
        n = rays.shape[0]
        hits = np.zeros((n, HIT_WORDS), np.float32)
        alb = np.zeros((n, 3), np.float32) if albedo else None
        check(lib().rtw_cast(self._handle(), C.byref(p), C.c_void_p(rays.ctypes.data), n, C.c_void_p(hits.ctypes.data),
                             C.c_void_p(alb.ctypes.data) if albedo else None))
        return _cast_result(hits, hits.view(np.int32), alb)

    def occluded(self, origins, directions, times=None, t_end=None, *, t_start: float = 0.001, seed: int = DEFAULT_SEED,
                 stream: int = 0, albedo: bool = False):
        """Whether anything lies on each ray within [t_start, t_end): `cast(...).hit`, from a walk that leaves at
        the first leaf that accepts.  A bool array."""
        if any(_is_tensor(a) for a in (origins, directions, times, t_end)):
            return self.occluded_device(origins, directions, times, t_end, t_start=t_start, seed=seed, stream=stream,
                                        albedo=albedo)
        if albedo:
            raise ValueError("albedo: an occlusion query has no hit to read it at")
        p = _params(t_start, seed, stream, False)
        rays = pack_rays(origins, directions, times, t_end)
        n = rays.shape[0]
        out = np.zeros(n, np.uint8)
        check(lib().rtw_occluded(self._handle(), C.byref(p), C.c_void_p(rays.ctypes.data), n, C.c_void_p(out.ctypes.data)))
        return out != 0


    # ---- radiance: ray_color along the rays ------------------------------------------------------
    def _radiance(self, rays, n: int, p: N.RadianceParams, per_sample: bool, max_bytes: int) -> RadianceResult:
        """The batch of packed device rays through rtw_radiance_samples_device / rtw_radiance_resolve_device in chunks
        of rays, chunk c with first_ray + its offset: the unchunked call's bits."""
        import torch

        dev, S = rays.device, int(p.samples)
        finite = bool(p.flags & N.RADIANCE_FINITE)
        mean = torch.empty((n, 3), dtype=torch.float32, device=dev)
        kept = torch.empty(n, dtype=torch.int32, device=dev) if finite else None
        out = torch.empty((n, S, 3), dtype=torch.float32, device=dev) if per_sample else None
        chunk = _MAX_ITEMS // S  # (>= 1: _radiance_params)
        if not per_sample:
            chunk = max(1, min(chunk, max_bytes // (S * 12)))
        chunk = min(chunk, n)
        scratch = None if per_sample or not n else torch.empty((chunk, S, 3), dtype=torch.float32, device=dev)
        L, h, sp = lib(), self._handle(), C.c_void_p(self._stream() or 0)
        for at in range(0, n, max(chunk, 1)):
            m = min(chunk, n - at)
            q = N.RadianceParams(0, p.mode, p.max_depth, S, p.first_sample, p.first_ray + at, p.seed)
            colors = out[at:at + m] if per_sample else scratch
            check(L.rtw_radiance_samples_device(h, C.byref(q), C.c_void_p(rays[at:].data_ptr()), m, C.c_void_p(colors.data_ptr()), sp))
            q.flags = p.flags
            check(L.rtw_radiance_resolve_device(C.byref(q), C.c_void_p(colors.data_ptr()), m, C.c_void_p(mean[at:].data_ptr()),
                                                C.c_void_p(kept[at:].data_ptr()) if finite else None, sp))
        return RadianceResult(mean=mean, kept=kept, samples=out)

    def radiance_device(self, origins, directions, times=None, samples: int = 16, max_depth: int = 50,
                        mode: RenderMode = RenderMode.Default, seed: int = DEFAULT_SEED, first_sample: int = 0,
                        first_ray: int = 0, finite: bool = False, per_sample: bool = False,
                        max_bytes: int = 256 << 20) -> RadianceResult:
        """`radiance` for float32 tensors on the caster's device (scalars and (3,) vectors are broadcast): device
        tensors out, no host copy, asynchronous on torch's current stream."""
        rays = self._pack_device(origins, directions, times, None)
        n = int(rays.shape[0])
        p = _radiance_params(samples, max_depth, mode, seed, first_sample, first_ray, finite, max_bytes, n)
        return self._radiance(rays, n, p, bool(per_sample), int(max_bytes))

    def radiance(self, origins, directions, times=None, samples: int = 16, max_depth: int = 50,
                 mode: RenderMode = RenderMode.Default, seed: int = DEFAULT_SEED, first_sample: int = 0, first_ray: int = 0,
                 finite: bool = False, per_sample: bool = False, max_bytes: int = 256 << 20) -> RadianceResult:
        """The path-traced colour that arrives along every ray: `samples` samples of the reference's ray_color each
        (the whole path: materials, textures, volumes, the light mixture), sample k of ray i drawn from the stream
        (seed, first_ray + i, first_sample + k), and their mean in sample order.  Every segment searches
        [0.001, +inf): there is no t_end.  Directions need not be unit length; times (default 0) moves Animation
        leaves along the whole path.  finite: the mean over the samples without a NaN or infinite channel, and
        `kept`, their count (a probe on a triangle mesh is otherwise NaN where the reference divides 0 by 0).
        per_sample: `samples` (n, S, 3) too.  Without it the samples live in a scratch tensor of at most max_bytes
        and the batch goes through in chunks of rays, with the same bits.  A batch split by rays (first_ray) or by
        samples (first_sample) gives the same samples.  Raises ValueError naming the argument, RtwError for what
        the library refuses."""
        if any(_is_tensor(a) for a in (origins, directions, times)):
            return self.radiance_device(origins, directions, times, samples, max_depth, mode, seed, first_sample, first_ray,
                                        finite, per_sample, max_bytes)
        import torch

        rays = pack_rays(origins, directions, times, None)
        n = rays.shape[0]
        p = _radiance_params(samples, max_depth, mode, seed, first_sample, first_ray, finite, max_bytes, n)
        d_rays = torch.from_numpy(rays).to(torch.device("cuda", self.device))
        res = self._radiance(d_rays, n, p, bool(per_sample), int(max_bytes))
        return RadianceResult(mean=res.mean.cpu().numpy(), kept=None if res.kept is None else res.kept.cpu().numpy().view(np.uint32),
                              samples=None if res.samples is None else res.samples.cpu().numpy())


def radiance_rays(world, origins, directions, times=None, samples: int = 16, max_depth: int = 50,
                  mode: RenderMode = RenderMode.Default, seed: int = DEFAULT_SEED, first_sample: int = 0, first_ray: int = 0,
                  finite: bool = False, per_sample: bool = False, max_bytes: int = 256 << 20, device: int = 0) -> RadianceResult:
    """One batch of `RayCaster.radiance` against `world` (a World is uploaded for the call and released after it; a
    DeviceWorld is used and left alone)."""
    caster = RayCaster(world, device)
    try:
        return caster.radiance(origins, directions, times, samples, max_depth, mode, seed, first_sample, first_ray, finite,
                               per_sample, max_bytes)
    finally:
        if not isinstance(world, DeviceWorld):
            caster.release()


def cast_rays(world, origins, directions, times=None, t_end=None, *, t_start: float = 0.001, seed: int = DEFAULT_SEED,
              stream: int = 0, albedo: bool = False, device: int = 0) -> CastResult:
    """One batch against `world` (a World is uploaded for the call and released after it; a DeviceWorld is used
    and left alone)."""
    caster = RayCaster(world, device)
    try:
        return caster.cast(origins, directions, times, t_end, t_start=t_start, seed=seed, stream=stream, albedo=albedo)
    finally:
        if not isinstance(world, DeviceWorld):
            caster.release()
