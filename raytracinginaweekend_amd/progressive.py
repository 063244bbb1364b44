"""Progressive, resumable accumulation (rtw_accum, include/rtw.h).

An `Accumulator` keeps one partition's running sums of sample colours on the device: add samples in
batches, look at the image at any point, save the state and resume it later.  A sample's RNG stream
is keyed by (seed, pixel, sample) and the sums are added in sample order, so after adds of n1, n2, ...
samples the image is bit-identical to `render` at samples_per_pixel = n1 + n2 + ... -- and so to the
reference at that spp.  With ``moments=True`` the accumulator also keeps per-channel sums of squares:
`stderr()` is the standard error of each channel's mean and `noise()` one scalar for the partition.

The reference's thread_count > 1 splits a frame's samples into planes by the *final* spp
(split_work_tasks, rendering.rs:222-237), so a prefix of such a frame is not a frame: accumulators
render thread_count 1 only.

`AccumState` (the checkpoint) needs neither a GPU nor librtw.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields

import numpy as np

from . import _native as N
from ._native import check, lib
from .rendering import DEFAULT_SEED, DeviceWorld, RenderMode, Size2i, render_params
from .world import World

_U32 = ("version", "flags", "samples", "reserved")
_I32 = ("width", "height", "tile_width", "tile_height", "part_index", "part_count", "max_depth", "render_mode")
_U64 = ("seed", "world_fingerprint")
_I64 = ("slots",)
_HEADER = {**{n: np.uint32 for n in _U32}, **{n: np.int32 for n in _I32}, **{n: np.uint64 for n in _U64},
           **{n: np.int64 for n in _I64}}


@dataclass
class AccumState:
    """One accumulator's exported state: the fields of rtw_accum_info, the per-slot sums and, with
    moments, the sums of squares (float32, shape (slots, 3); padding slots of edge tiles hold zeros)."""

    version: int
    flags: int
    width: int
    height: int
    tile_width: int
    tile_height: int
    part_index: int
    part_count: int
    max_depth: int
    render_mode: int
    samples: int
    reserved: int
    seed: int
    world_fingerprint: int
    slots: int
    sums: np.ndarray
    squares: np.ndarray | None = None

    def header(self) -> dict:
        return {n: int(getattr(self, n)) for n in _HEADER}

    def save(self, path) -> None:
        """One .npz of plain arrays (numpy.savez): a 0-d array per header field, `sums`, and `squares`
        when the accumulator kept moments."""
        arrays = {n: np.asarray(getattr(self, n), dtype=t) for n, t in _HEADER.items()}
        arrays["sums"] = np.ascontiguousarray(self.sums, np.float32)
        if self.squares is not None:
            arrays["squares"] = np.ascontiguousarray(self.squares, np.float32)
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path) -> "AccumState":
        """Reads a file written by `save`.  Nothing is unpickled: a file holding anything but the plain
        arrays `save` writes is refused."""
        with np.load(path, allow_pickle=False) as z:
            names = set(z.files)
            known = set(_HEADER) | {"sums", "squares"}
            if names - known:
                raise ValueError(f"not an accumulator checkpoint: unexpected entries {sorted(names - known)}")
            missing = (set(_HEADER) | {"sums"}) - names
            if missing:
                raise ValueError(f"not an accumulator checkpoint: missing entries {sorted(missing)}")
            vals = {}
            for n, t in _HEADER.items():
                a = z[n]
                if a.dtype != np.dtype(t) or a.shape != ():
                    raise ValueError(f"accumulator checkpoint: bad header field {n}")
                vals[n] = int(a)
            arrays = {}
            for n in ("sums", "squares"):
                if n not in names:
                    continue
                a = z[n]
                if a.dtype != np.float32 or a.shape != (vals["slots"], 3):
                    raise ValueError(f"accumulator checkpoint: {n} is not float32 of shape (slots, 3)")
                arrays[n] = a
        return cls(**vals, sums=arrays["sums"], squares=arrays.get("squares"))


assert [f.name for f in fields(AccumState)][:len(_HEADER)] == [n for n, _ in N.AccumInfo._fields_]


def _f32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Accumulator:
    """A growing frame of one World on one GPU (rtw_accum_create).

    world: a `World` (uploaded here) or a `DeviceWorld` (shared: one-shot frames and several
    accumulators of one DeviceWorld may interleave freely).  The accumulator keeps it alive."""

    def __init__(self, world: World | DeviceWorld, size: Size2i, max_depth: int,
                 render_mode: RenderMode = RenderMode.Default, *, seed: int = DEFAULT_SEED, device: int = 0,
                 tile: tuple[int, int] = (8, 8), part: tuple[int, int] = (0, 1), layout: int = N.LAYOUT_IMAGE,
                 moments: bool = False, thread_count: int = 1):
        self._h = None
        self.dworld = world if isinstance(world, DeviceWorld) else DeviceWorld(world, device)
        self.device = self.dworld.device
        self.size = size
        self.moments = bool(moments)
        self.params = render_params(size, 0, max_depth, render_mode, seed, tile=tile, part=part, layout=layout,
                                    thread_count=thread_count)
        h = C.c_void_p()
        check(lib().rtw_accum_create(self.dworld._h, C.byref(self.params), N.ACCUM_MOMENTS if moments else 0,
                                     C.byref(h)))
        self._h = h
        self._out = None

    def release(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().rtw_accum_release(self._h)
            self._h = None
        self._out = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def info(self) -> N.AccumInfo:
        i = N.AccumInfo()
        check(lib().rtw_accum_get_info(self._h, C.byref(i)))
        return i

    @property
    def samples(self) -> int:
        """Samples per pixel added so far."""
        return int(self.info().samples)

    @property
    def slots(self) -> int:
        return int(self.info().slots)

    def add(self, n: int, stream_ptr: int | None = None) -> None:
        """Renders the next `n` samples of every pixel and adds them (asynchronous on `stream_ptr`)."""
        if n < 0:
            raise ValueError("n must be >= 0")
        check(lib().rtw_accum_add(self._h, n, C.c_void_p(stream_ptr or 0)))

    def resolve_into(self, ptr: int, stream_ptr: int | None = None) -> None:
        """sum / samples into the device buffer at `ptr`, in the accumulator's layout (asynchronous)."""
        check(lib().rtw_accum_resolve(self._h, C.c_void_p(ptr), C.c_void_p(stream_ptr or 0)))

    def _rows(self) -> int:
        return self.slots if self.params.layout == N.LAYOUT_TILES else self.size.width * self.size.height

    def _resolved(self, fn) -> np.ndarray:
        import torch

        dev = torch.device("cuda", self.device)
        # (zeros: with part_count > 1 an IMAGE-layout resolve leaves the other partitions' pixels alone)
        out = torch.zeros(self._rows() * 3, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev)
        check(fn(self._h, C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        return out.cpu().numpy().reshape(-1, 3)

    def image(self) -> np.ndarray:
        """The image so far on the host: (W*H, 3) f32 (LAYOUT_IMAGE) or (slots, 3) (LAYOUT_TILES)."""
        return self._resolved(lib().rtw_accum_resolve)

    def stderr(self) -> np.ndarray:
        """The standard error of each channel's mean, laid out as `image()` (moments, samples >= 2)."""
        return self._resolved(lib().rtw_accum_resolve_stderr)

    def noise(self, stream_ptr: int | None = None) -> tuple[float, int]:
        """(mean over the pixels of (se_r + se_g + se_b) / (mean_r + mean_g + mean_b + 0.01), pixels
        counted); pixels whose value is not finite are left out (moments, samples >= 2)."""
        v, n = C.c_double(), C.c_int64()
        check(lib().rtw_accum_noise(self._h, C.c_void_p(stream_ptr or 0), C.byref(v), C.byref(n)))
        return v.value, n.value

    def state(self) -> AccumState:
        i = self.info()
        sums = np.zeros((i.slots, 3), np.float32)
        squares = np.zeros((i.slots, 3), np.float32) if self.moments else None
        check(lib().rtw_accum_export(self._h, _f32p(sums), _f32p(squares) if squares is not None else None))
        return AccumState(**{n: int(getattr(i, n)) for n in _HEADER}, sums=sums, squares=squares)

    def load_state(self, state: AccumState) -> None:
        """Continue `state`'s frame here.  Raises RtwError naming the field when the state belongs to another
        world, geometry, max_depth, render mode, seed or flags."""
        i = N.AccumInfo()
        for n in _HEADER:
            setattr(i, n, getattr(state, n))
        sums = np.ascontiguousarray(state.sums, np.float32)
        squares = None if state.squares is None else np.ascontiguousarray(state.squares, np.float32)
        if sums.size != 3 * state.slots or (squares is not None and squares.size != sums.size):
            raise ValueError("state arrays do not hold 3 * slots floats")
        check(lib().rtw_accum_import(self._h, C.byref(i), _f32p(sums), _f32p(squares) if squares is not None else None))


def world_fingerprint(world: World) -> int:
    """rtw_world_fingerprint: 64-bit FNV-1a over the world's contents (host only)."""
    v = C.c_uint64()
    check(lib().rtw_world_fingerprint(world.ptr(), C.byref(v)))
    return v.value


def render_progressive(size: Size2i, max_depth: int, world, batches, **kw):
    """Yields (samples, image) after each batch of `batches` (sample counts to add in turn)."""
    acc = Accumulator(world, size, max_depth, **kw)
    try:
        for n in batches:
            acc.add(int(n))
            yield acc.samples, acc.image()
    finally:
        acc.release()


def render_to_noise(size: Size2i, max_depth: int, world, target: float, max_samples: int, batch: int = 16, **kw):
    """Adds `batch` samples at a time (the last batch cut to `max_samples`) until noise() <= target or
    samples == max_samples.  Returns (image, samples, noise)."""
    if max_samples < 2 or batch < 1:
        raise ValueError("max_samples must be >= 2 and batch >= 1")
    kw["moments"] = True
    acc = Accumulator(world, size, max_depth, **kw)
    try:
        noise = float("inf")
        while acc.samples < max_samples:
            acc.add(min(batch, max_samples - acc.samples))
            if acc.samples >= 2:
                noise = acc.noise()[0]
                if noise <= target:
                    break
        return acc.image(), acc.samples, noise
    finally:
        acc.release()
