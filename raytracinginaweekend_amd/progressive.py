"""Progressive, resumable accumulation (rtw_accum, include/rtw.h).

An `Accumulator` keeps one partition's running sums of sample colours on the device: add samples in
batches, look at the image at any point, save the state and resume it later.  A sample's RNG stream
is keyed by (seed, pixel, sample) and the sums are added in sample order, so after adds of n1, n2, ...
samples the image is bit-identical to `render` at samples_per_pixel = n1 + n2 + ... -- and so to the
reference at that spp.  With ``moments=True`` the accumulator also keeps per-channel sums of squares:
`stderr()` is the standard error of each channel's mean and `noise()` one scalar for the partition.

With ``adaptive=True`` (implies moments) the noise estimate also places the samples: `adapt(target)` stops
every tile whose worst pixel's relative standard error is at most `target`, and `add` renders the active
tiles only.  A stopped tile stays stopped; it holds, bit for bit, the pixels of `render` at
samples_per_pixel = its own count (`tile_stops()`, `sample_counts()`), so the image stays exact tile by
tile, with the stop map as part of the output.  `render_adaptive` is the loop.

With ``finite=True`` the accumulate pass leaves out every sample with a NaN or infinite channel (the reference's
0/0 pdf quirk makes an occasional whole sample NaN, and one such sample turns a plain accumulator's pixel NaN for
good): the sample adds nothing and is not counted, `kept_counts()` holds the samples that entered each pixel's sum
and `rejected_counts()` the rest, and `image()`, `stderr()`, `noise()`, `adapt()` and `denoised()` divide by the
pixel's own kept count.  On a pixel with no rejected sample every value is the plain accumulator's, bit for bit.
Dropping samples biases the estimate (the dropped paths carried energy): a plain accumulator's `image()` and
`render` stay the exact reference image.  Combines with moments and adaptive.  `render_finite` is the one-call form.

With ``clamp=L`` (implies finite; include/rtw_clamp.h) the accumulate pass also scales every finite sample whose largest
channel exceeds L down to it (firefly control: one sample of 27 no longer holds a tile's noise estimate up).  The hue
is kept and no accumulated channel exceeds L.  `clamped_counts()` holds the samples it scaled per pixel and
`clamp_loss()` the mean radiance it removed, so `image() + clamp_loss()` is the unclamped finite mean up to rounding.
`image()`, `stderr()`, `noise()`, `adapt()` and `denoised()` work on the clamped sums.  On a pixel without a clamped
sample every value is the finite accumulator's, bit for bit.  Clamping biases the estimate: it is opt-in.
`render_clamped` is the one-call form.

The reference's thread_count > 1 splits a frame's samples into planes by the *final* spp
(split_work_tasks, rendering.rs:222-237), so a prefix of such a frame is not a frame: accumulators
render thread_count 1 only.

Across GPUs (distributed.py has the rank wrapper): every rank holds an accumulator of part (rank, N); `pack_into`
writes its state as one record (include/rtw_parts.h), the records are gathered, and `merge_parts` places them
into an accumulator of part (0, 1), which then is, bit for bit, the accumulator one GPU would hold.
`AccumState.merge` / `AccumState.split` do the same to checkpoints, so one written by N ranks resumes on M.

`AccumState` (the checkpoint) needs neither a GPU nor librtw.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields

import numpy as np

from . import _native as N
from . import _parts
from ._native import check, lib
from .aov import AovAccumulator
from .rendering import DEFAULT_SEED, DeviceWorld, RenderMode, Size2i, render_params
from .world import World

_U32 = ("version", "flags", "samples", "reserved")
_I32 = ("width", "height", "tile_width", "tile_height", "part_index", "part_count", "max_depth", "render_mode")
_U64 = ("seed", "world_fingerprint")
_I64 = ("slots",)
_HEADER = {**{n: np.uint32 for n in _U32}, **{n: np.int32 for n in _I32}, **{n: np.uint64 for n in _U64},
           **{n: np.int64 for n in _I64}}
# The state arrays beside the header, in the order of the packed record's sections (rtw_device.hip's ACC_DESC is the
# same table; a new state array is one row there and one here): the field, the flag that calls for it (0: every
# accumulator), the dtype, the shape in terms of slots and tiles, and record_layout's key of its section.
_ARRAYS = (("sums", 0, np.float32, ("slots", 3), "sums"),
           ("squares", N.ACCUM_MOMENTS, np.float32, ("slots", 3), "squares"),
           ("kept", N.ACCUM_FINITE, np.uint32, ("slots",), "kept"),
           ("clamped", N.ACCUM_CLAMP, np.uint32, ("slots",), "clamped"),
           ("lost", N.ACCUM_CLAMP, np.float32, ("slots", 3), "lost"),
           ("tile_stop", N.ACCUM_ADAPTIVE, np.uint32, ("tiles",), "stop"))
_CONVERTED = ("sums", "squares")  # taken as any array numpy converts to float32; the others must come as they are


def _dims(shape: tuple, slots: int, tiles: int) -> tuple:
    return tuple({"slots": int(slots), "tiles": int(tiles)}.get(d, d) for d in shape)


def _shape_text(shape: tuple) -> str:
    return "(" + ", ".join(map(str, shape)) + (",)" if len(shape) == 1 else ")")


def _zeros(flags: int, slots: int, tiles: int) -> dict:
    """A zeroed array per row of _ARRAYS that `flags` call for, None for the others."""
    return {name: np.zeros(_dims(shape, slots, tiles), dtype) if flag == 0 or flags & flag else None
            for name, flag, dtype, shape, _ in _ARRAYS}


def _pointer(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float if a.dtype == np.float32 else C.c_uint32))


RECORD_VERSION = _parts.VERSION  # RTW_PARTS_VERSION
RECORD_HEADER_WORDS = _parts.HEADER_WORDS


def record_layout(width: int, height: int, tile: tuple[int, int], flags: int, part_count: int) -> dict:
    """The packed record of include/rtw_parts.h in numpy's terms: per_tile, n_tiles, tiles0, slots0, the word
    offsets sums / squares / kept / clamped / lost / stop (None: the flags do not call for the section) and words."""
    tw, th = tile
    per_tile = tw * th
    lay = _parts.section_offsets(-(-width // tw) * -(-height // th), part_count, per_tile,
                                 tuple((key, flag == 0 or flags & flag, int(np.prod(_dims(shape, per_tile, 1))))
                                       for _, flag, _, shape, key in _ARRAYS))
    lay["per_tile"] = per_tile
    return lay


@dataclass
class AccumState:
    """One accumulator's exported state: the fields of rtw_accum_info, the per-slot sums and, with
    moments, the sums of squares (float32, shape (slots, 3); padding slots of edge tiles hold zeros);
    of an adaptive accumulator also the stop map (uint32, shape (tiles,), tiles = slots / (tile_width *
    tile_height): 0 = active, else the sample count the tile stopped at); of a finite accumulator also the kept
    counts (uint32, shape (slots,): the samples that entered each slot's sums; padding slots hold 0); of a clamp
    accumulator also the clamped counts (uint32, shape (slots,)) and the lost sums (float32, shape (slots, 3)), zero
    in padding slots, and the level: `clamp`, whose f32 bits the header's `reserved` holds."""

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
    tile_stop: np.ndarray | None = None
    kept: np.ndarray | None = None
    clamped: np.ndarray | None = None
    lost: np.ndarray | None = None

    @property
    def clamp(self) -> float | None:
        """The clamp level (None: the flags hold no RTW_ACCUM_CLAMP)."""
        if not int(self.flags) & N.ACCUM_CLAMP:
            return None
        return float(np.array(int(self.reserved), np.uint32).view(np.float32))

    def header(self) -> dict:
        return {n: int(getattr(self, n)) for n in _HEADER}

    @property
    def tiles(self) -> int:
        """Local tiles of the partition (entries of the stop map)."""
        return int(self.slots) // (int(self.tile_width) * int(self.tile_height))

    def save(self, path) -> None:
        """One .npz of plain arrays (numpy.savez): a 0-d array per header field, `sums`, `squares`
        when the accumulator kept moments, `tile_stop` when it was adaptive, `kept` when it was finite and `clamped`
        and `lost` when it clamped (the level travels in `reserved`)."""
        arrays = {n: np.asarray(getattr(self, n), dtype=t) for n, t in _HEADER.items()}
        if (self.clamped is None) != (self.lost is None):
            raise ValueError("clamped and lost go together")
        for name, _, dtype, shape, _ in _ARRAYS:
            a = getattr(self, name)
            if a is None:
                continue
            if name not in _CONVERTED:
                a = np.asarray(a)
                if a.dtype != dtype or a.shape != _dims(shape, self.slots, self.tiles):
                    raise ValueError(f"{name} is not {np.dtype(dtype).name} of shape {_shape_text(shape)}")
            arrays[name] = np.ascontiguousarray(a, dtype)
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path) -> "AccumState":
        """Reads a file written by `save`.  Nothing is unpickled: a file holding anything but the plain
        arrays `save` writes is refused."""
        with np.load(path, allow_pickle=False) as z:
            names = set(z.files)
            known = set(_HEADER) | {row[0] for row in _ARRAYS}
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
            tiles = vals["slots"] // max(1, vals["tile_width"] * vals["tile_height"])
            for n, _, dtype, shape, _ in _ARRAYS:
                if n not in names:
                    continue
                a = z[n]
                if a.dtype != dtype or a.shape != _dims(shape, vals["slots"], tiles):
                    raise ValueError(f"accumulator checkpoint: {n} is not {np.dtype(dtype).name} of shape {_shape_text(shape)}")
                arrays[n] = a
            if ("clamped" in names) != ("lost" in names):
                raise ValueError("accumulator checkpoint: clamped and lost go together")
        return cls(**vals, **arrays)

    def _frame_tiles(self) -> int:
        return -(-int(self.width) // int(self.tile_width)) * -(-int(self.height) // int(self.tile_height))

    @classmethod
    def merge(cls, states) -> "AccumState":
        """The whole image's state (part (0, 1)) from the states of parts (0..N-1, N) of one frame, in any order:
        a placement of tile blocks, bit for bit the state one accumulator would hold.  Raises ValueError naming
        the field when the states differ in geometry, max_depth, render_mode, seed, world_fingerprint, version or
        flags, when a part is missing or comes twice, when slots or an array does not fit the part, when the clamp
        levels differ ("clamp"), and when samples differ between parts that are not adaptive.  Adaptive: samples is the largest of the parts' (a
        part whose tiles have all stopped no longer counts, `Accumulator.add`)."""
        states = list(states)
        for s in states[1:]:  # (before `reserved`, which holds the level's bits)
            if int(s.flags) == int(states[0].flags) and int(s.flags) & N.ACCUM_CLAMP and int(s.reserved) != int(states[0].reserved):
                raise ValueError(f"the states are not parts of one frame: clamp differs ({s.clamp!r} against {states[0].clamp!r})")
        by_part = _parts.parts_in_order(states, ("version", "flags", "width", "height", "tile_width", "tile_height", "part_count",
                                                 "max_depth", "render_mode", "reserved", "seed", "world_fingerprint"))
        first, count = states[0], len(by_part)
        flags = int(first.flags)
        adaptive = bool(flags & N.ACCUM_ADAPTIVE)
        per_tile, n_tiles = int(first.tile_width) * int(first.tile_height), first._frame_tiles()
        slots = n_tiles * per_tile
        whole = _zeros(flags, slots, n_tiles)
        samples = int(first.samples)
        for r in range(count):
            s = by_part[r]
            tiles, at = _parts.part_tiles(n_tiles, (r, count)), _parts.part_slots(n_tiles, per_tile, (r, count))
            if int(s.slots) != at.size:
                raise ValueError(f"part {r}: slots differs from the partition's ({at.size})")
            if not adaptive and int(s.samples) != samples:
                raise ValueError(f"part {r}: samples differs (only adaptive parts may differ)")
            samples = max(samples, int(s.samples))
            for name, _, _, shape, _ in _ARRAYS:
                src, dst, shape = getattr(s, name), whole[name], _dims(shape, at.size, tiles.size)
                if (src is None) != (dst is None):
                    raise ValueError(f"part {r}: {name} does not go with the flags")
                if dst is None:
                    continue
                src = np.asarray(src)
                if src.shape != shape or src.dtype != dst.dtype:
                    raise ValueError(f"part {r}: {name} is not {dst.dtype} of shape {shape}")
                # (bit patterns, not values: a NaN's payload travels)
                dst.view(np.uint32)[tiles if name == "tile_stop" else at] = src.view(np.uint32)
            if adaptive:
                bad = (s.tile_stop == 1) | (s.tile_stop > int(s.samples))
                if bad.any():
                    raise ValueError(f"part {r}: tile_stop[{int(np.flatnonzero(bad)[0])}] is 1 or above the part's samples")
        head = first.header()
        head.update(part_index=0, part_count=1, samples=samples, slots=slots)
        return cls(**head, **whole)

    def split(self, part_count: int) -> list["AccumState"]:
        """The inverse of `merge`: the states of parts (0..part_count-1, part_count) of this whole-image state.  A
        stopped tile keeps its stop; a part's samples is this state's when the part has an active tile (or the
        state is not adaptive), else the largest stop among its tiles (0 for a part without tiles): what that
        rank's accumulator would hold.  `merge(s.split(M))` is `s` for every M, so `merge` then `split(M)`
        re-partitions a checkpoint of N ranks for M (each loads its part with `Accumulator.load_state`)."""
        if (int(self.part_index), max(1, int(self.part_count))) != (0, 1):
            raise ValueError("split needs the whole image's state: part_index / part_count is not 0 / 1")
        if part_count < 1:
            raise ValueError("part_count must be >= 1")
        per_tile, n_tiles = int(self.tile_width) * int(self.tile_height), self._frame_tiles()
        if int(self.slots) != n_tiles * per_tile:
            raise ValueError("slots differs from the frame's")
        if self.tile_stop is not None and n_tiles and (self.tile_stop != 0).all() and int(self.tile_stop.max()) != int(self.samples):
            raise ValueError("samples is above the largest stop although every tile has stopped: no accumulator "
                             "holds such a state, and its parts could not tell")
        out = []
        for r in range(part_count):
            tiles, at = _parts.part_tiles(n_tiles, (r, part_count)), _parts.part_slots(n_tiles, per_tile, (r, part_count))
            part = {}
            for name, _, _, shape, _ in _ARRAYS:
                a = getattr(self, name)
                part[name] = None if a is None else np.ascontiguousarray(a[tiles if shape[0] == "tiles" else at])
            stop = part["tile_stop"]
            samples = int(self.samples)
            if stop is not None and not (stop == 0).any():
                samples = int(stop.max()) if stop.size else 0
            head = self.header()
            head.update(part_index=r, part_count=part_count, samples=samples, slots=int(at.size))
            out.append(AccumState(**head, **part))
        return out

    def packed(self, stride_bytes: int | None = None) -> np.ndarray:
        """This state as the record `Accumulator.pack_into` writes (uint32 words, include/rtw_parts.h), padded
        with zeros to `stride_bytes`: what a rank without device-aware collectives sends."""
        count = max(1, int(self.part_count))
        lay = record_layout(int(self.width), int(self.height), (int(self.tile_width), int(self.tile_height)), int(self.flags), count)
        sections = tuple((key, getattr(self, name)) for name, _, _, _, key in _ARRAYS)
        for name, arr in sections:
            if (arr is None) != (lay[name] is None):
                raise ValueError(f"{name} does not go with the flags")
        header = (RECORD_VERSION, int(self.flags), int(self.part_index), count, int(self.samples), int(self.slots), self.tiles,
                  int(self.reserved) if int(self.flags) & N.ACCUM_CLAMP else 0)
        return _parts.pack_record(header, lay["words"], stride_bytes, [(lay[name], arr) for name, arr in sections if arr is not None])


assert [f.name for f in fields(AccumState)][:len(_HEADER)] == [n for n, _ in N.AccumInfo._fields_]


class Accumulator:
    """A growing frame of one World on one GPU (rtw_accum_create).

    world: a `World` (uploaded here) or a `DeviceWorld` (shared: one-shot frames and several
    accumulators of one DeviceWorld may interleave freely).  The accumulator keeps it alive."""

    def __init__(self, world: World | DeviceWorld, size: Size2i, max_depth: int,
                 render_mode: RenderMode = RenderMode.Default, *, seed: int = DEFAULT_SEED, device: int = 0,
                 tile: tuple[int, int] = (8, 8), part: tuple[int, int] = (0, 1), layout: int = N.LAYOUT_IMAGE,
                 moments: bool = False, adaptive: bool = False, finite: bool = False, thread_count: int = 1,
                 clamp: float | None = None):
        self._h = None
        self._denoiser = None  # made by the first denoised()
        self.dworld = world if isinstance(world, DeviceWorld) else DeviceWorld(world, device)
        self.device = self.dworld.device
        self.size = size
        self.adaptive = bool(adaptive)
        self.moments = bool(moments) or self.adaptive
        self.clamp = None if clamp is None else float(np.float32(clamp))  # the level (an f32), or None
        self.finite = bool(finite) or self.clamp is not None
        self.params = render_params(size, 0, max_depth, render_mode, seed, tile=tile, part=part, layout=layout,
                                    thread_count=thread_count)
        h = C.c_void_p()
        flags = (N.ACCUM_MOMENTS if self.moments else 0) | (N.ACCUM_ADAPTIVE if self.adaptive else 0)
        flags |= N.ACCUM_FINITE if self.finite else 0
        if self.clamp is not None:
            check(lib().rtw_accum_create_clamp(self.dworld._h, C.byref(self.params), flags | N.ACCUM_CLAMP, self.clamp, C.byref(h)))
        else:
            check(lib().rtw_accum_create(self.dworld._h, C.byref(self.params), flags, C.byref(h)))
        self._h = h
        self._out = None

    def release(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().rtw_accum_release(self._h)
            self._h = None
        if getattr(self, "_denoiser", None) is not None:
            self._denoiser.release()
            self._denoiser = None
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
        """Samples per pixel added so far (adaptive: of the active tiles, the frontier)."""
        return int(self.info().samples)

    @property
    def slots(self) -> int:
        return int(self.info().slots)

    def add(self, n: int, stream_ptr: int | None = None) -> None:
        """Renders the next `n` samples of every pixel and adds them (asynchronous on `stream_ptr`).  Adaptive:
        of the pixels of the active tiles only; with none active the call does nothing."""
        if n < 0:
            raise ValueError("n must be >= 0")
        check(lib().rtw_accum_add(self._h, n, C.c_void_p(stream_ptr or 0)))

    def resolve_into(self, ptr: int, stream_ptr: int | None = None) -> None:
        """sum / samples into the device buffer at `ptr`, in the accumulator's layout (asynchronous)."""
        check(lib().rtw_accum_resolve(self._h, C.c_void_p(ptr), C.c_void_p(stream_ptr or 0)))

    def _rows(self) -> int:
        return self.slots if self.params.layout == N.LAYOUT_TILES else self.size.width * self.size.height

    def _resolved(self, fn, channels: int = 3, dtype=None) -> np.ndarray:
        import torch

        dev = torch.device("cuda", self.device)
        # (zeros: with part_count > 1 an IMAGE-layout resolve leaves the other partitions' pixels alone)
        out = torch.zeros(self._rows() * channels, dtype=dtype or torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev)
        check(fn(self._h, C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        return out.cpu().numpy().reshape(-1, channels)

    def image(self) -> np.ndarray:
        """The image so far on the host: (W*H, 3) f32 (LAYOUT_IMAGE) or (slots, 3) (LAYOUT_TILES)."""
        return self._resolved(lib().rtw_accum_resolve)

    def stderr(self) -> np.ndarray:
        """The standard error of each channel's mean, laid out as `image()` (moments, samples >= 2)."""
        return self._resolved(lib().rtw_accum_resolve_stderr)

    def _resolved_device(self, fn):
        import torch

        dev = torch.device("cuda", self.device)
        out = torch.zeros((self.size.width * self.size.height, 3), dtype=torch.float32, device=dev)
        check(fn(self._h, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return out

    def denoised(self, guide=None, albedo=None, **options):
        """A denoised preview of the image so far: (W*H, 3) f32 on the host (with variance=True also the (W*H,)
        variance of each filtered pixel).  Resolves the image and `stderr()` on the device and runs a cached
        `Denoiser` on them (denoise.py; options: iterations, sigma_l, sigma_g, variance).  `guide` is an
        array or device tensor of shape (W*H, 1..4), or another Accumulator of this size and device whose image
        is taken -- one in `RenderMode.Normals`, say -- or an `AovAccumulator`, whose normal image is taken.
        `albedo` is an array or device tensor of shape (W*H, 3) or an `AovAccumulator`, whose albedo image is
        taken: the filter then runs on the demodulated image (`Denoiser.run`).  An AOV accumulator of another size
        or device, or one without samples, raises ValueError.  Needs moments=True and samples >= 2.
        Non-destructive: the sums are only read, `image()` stays the exact image and further adds continue the frame.

        A filter needs the whole image: an accumulator with LAYOUT_TILES or part != (0, 1) raises ValueError.
        Rank users gather the image and the standard error and call `Denoiser.run` on rank 0."""
        import torch

        from .denoise import Denoiser

        if self.params.layout != N.LAYOUT_IMAGE:
            raise ValueError("denoised() needs the whole image: the accumulator's layout is LAYOUT_TILES")
        if (self.params.part_index, max(1, self.params.part_count)) != (0, 1):
            raise ValueError("denoised() needs the whole image: the accumulator holds one partition of it "
                             "(gather the image and the standard error and call Denoiser.run on rank 0)")
        if not self.moments:
            raise ValueError("denoised() needs an accumulator with moments=True")
        if self.samples < 2:
            raise ValueError("denoised() needs samples >= 2")
        dev = torch.device("cuda", self.device)

        def aov_image(name: str, aov: AovAccumulator, channel: str):
            if (aov.size.width, aov.size.height) != (self.size.width, self.size.height) or aov.device != self.device:
                raise ValueError(f"the {name} AOV accumulator has another size or device")
            if aov.samples < 1:
                raise ValueError(f"the {name} AOV accumulator holds no samples")
            return aov.normal_device() if channel == "normal" else aov.albedo_device()

        if isinstance(albedo, AovAccumulator):
            albedo = aov_image("albedo", albedo, "albedo")
        elif albedo is not None and not hasattr(albedo, "data_ptr"):
            albedo = torch.from_numpy(np.ascontiguousarray(albedo, np.float32)).to(dev)
        if isinstance(guide, AovAccumulator):
            guide = aov_image("guide", guide, "normal")
        elif isinstance(guide, Accumulator):
            if (guide.size.width, guide.size.height) != (self.size.width, self.size.height) or guide.device != self.device:
                raise ValueError("the guide accumulator has another size or device")
            if guide.params.layout != N.LAYOUT_IMAGE or (guide.params.part_index, max(1, guide.params.part_count)) != (0, 1):
                raise ValueError("the guide accumulator does not hold the whole image")
            guide = guide._resolved_device(lib().rtw_accum_resolve)
        elif guide is not None and not hasattr(guide, "data_ptr"):
            guide = torch.from_numpy(np.ascontiguousarray(guide, np.float32)).to(dev)
        if self._denoiser is None:
            self._denoiser = Denoiser(self.size, self.device)
        color = self._resolved_device(lib().rtw_accum_resolve)
        se = self._resolved_device(lib().rtw_accum_resolve_stderr)
        res = self._denoiser.run_device(color, se, guide, color, albedo=albedo, **options)
        torch.cuda.current_stream(dev).synchronize()
        if isinstance(res, tuple):
            return res[0].cpu().numpy(), res[1].cpu().numpy()
        return res.cpu().numpy()

    def noise(self, stream_ptr: int | None = None) -> tuple[float, int]:
        """(mean over the pixels of (se_r + se_g + se_b) / (mean_r + mean_g + mean_b + 0.01), pixels
        counted); pixels whose value is not finite are left out (moments, samples >= 2)."""
        v, n = C.c_double(), C.c_int64()
        check(lib().rtw_accum_noise(self._h, C.c_void_p(stream_ptr or 0), C.byref(v), C.byref(n)))
        return v.value, n.value

    def sample_counts(self) -> np.ndarray:
        """The samples each pixel holds (its tile's count), uint32, laid out as `image()` with one channel;
        padding slots of a tile buffer hold 0."""
        import torch

        return self._resolved(lib().rtw_accum_resolve_samples, 1, torch.int32).view(np.uint32)

    def kept_counts(self) -> np.ndarray:
        """The samples that entered each pixel's sums (finite=True), uint32, laid out as `sample_counts()`."""
        import torch

        return self._resolved(lib().rtw_accum_resolve_kept, 1, torch.int32).view(np.uint32)

    def clamped_counts(self) -> np.ndarray:
        """The samples of each pixel the clamp scaled down (clamp=L), uint32, laid out as `kept_counts()`."""
        import torch

        return self._resolved(lib().rtw_accum_resolve_clamped, 1, torch.int32).view(np.uint32)

    def clamp_loss(self) -> np.ndarray:
        """The mean radiance the clamp removed from each pixel, lost / kept per channel (clamp=L), laid out as
        `image()`: (W*H, 3) f32."""
        return self._resolved(lib().rtw_accum_resolve_clamp_loss)

    def rejected_counts(self) -> np.ndarray:
        """The samples of each pixel that were left out: `sample_counts()` - `kept_counts()` (finite=True)."""
        return self.sample_counts() - self.kept_counts()

    @property
    def tiles(self) -> int:
        """Local tiles of the partition (entries of the stop map)."""
        return self.slots // (self.params.tile_width * self.params.tile_height)

    def adapt(self, target: float, min_samples: int = 16, stream_ptr: int | None = None) -> tuple[int, int]:
        """Stops every active tile whose worst pixel has a relative standard error (the per-pixel value of
        `noise()`) of at most `target`, once the accumulator holds `min_samples` samples.  Returns (active
        tiles, active pixels) after the decision (adaptive, samples >= 2, min_samples >= 2)."""
        t, p = C.c_int64(), C.c_int64()
        check(lib().rtw_accum_adapt(self._h, target, min_samples, C.c_void_p(stream_ptr or 0), C.byref(t), C.byref(p)))
        return t.value, p.value

    def tile_stops(self) -> np.ndarray:
        """The stop map: per local tile 0 (active) or the sample count it stopped at (uint32, shape (tiles,))."""
        stop = np.zeros(self.tiles, np.uint32)
        check(lib().rtw_accum_tile_stops(self._h, _pointer(stop)))
        return stop

    def state(self) -> AccumState:
        i = self.info()
        arrays = _zeros(int(i.flags), i.slots, self.tiles)
        p = {name: _pointer(a) for name, a in arrays.items()}
        if self.clamp is not None:
            check(lib().rtw_accum_export_state_clamp(self._h, p["sums"], p["squares"], p["tile_stop"], p["kept"], p["clamped"],
                                                     p["lost"]))
        elif self.finite:  # the one pair for every flag combination
            check(lib().rtw_accum_export_state(self._h, p["sums"], p["squares"], p["tile_stop"], p["kept"]))
        elif self.adaptive:
            check(lib().rtw_accum_export_adaptive(self._h, p["sums"], p["squares"], p["tile_stop"]))
        else:
            check(lib().rtw_accum_export(self._h, p["sums"], p["squares"]))
        return AccumState(**{n: int(getattr(i, n)) for n in _HEADER}, **arrays)

    def packed_bytes(self) -> int:
        """The bytes of this accumulator's packed record (the same for every part of its part_count)."""
        return N.packed_bytes(self.params, int(self.info().flags), max(1, self.params.part_count))

    def pack_into(self, tensor, stream_ptr: int | None = None) -> None:
        """Writes the accumulator's state as one packed record (include/rtw_parts.h) into the device tensor
        (at least `packed_bytes()` bytes; asynchronous on `stream_ptr`, ordered with the accumulator's calls)."""
        if not tensor.is_cuda or not tensor.is_contiguous() or tensor.numel() * tensor.element_size() < self.packed_bytes():
            raise ValueError("pack_into needs a contiguous device tensor of at least packed_bytes() bytes")
        check(lib().rtw_accum_pack(self._h, C.c_void_p(tensor.data_ptr()), C.c_void_p(stream_ptr or 0)))

    def merge_parts(self, gathered, stride_bytes: int, part_count: int, stream_ptr: int | None = None) -> None:
        """Replaces this whole-image accumulator's state (part (0, 1)) by the merge of `part_count` packed records,
        record r at byte r * stride_bytes of the device tensor `gathered` (rtw_accum_merge_parts).  Raises
        RtwError naming the field for records of another version, flags, order, part_count, geometry or clamp
        level, a bad stride, and unequal samples where not adaptive; nothing is launched then."""
        need = max(0, part_count - 1) * stride_bytes + N.packed_bytes(self.params, int(self.info().flags), max(1, part_count))
        if not gathered.is_cuda or not gathered.is_contiguous():
            raise ValueError("merge_parts needs a contiguous device tensor")
        if stride_bytes > 0 and gathered.numel() * gathered.element_size() < need:
            raise ValueError(f"the gathered tensor holds fewer than the {need} bytes of {part_count} records")
        check(lib().rtw_accum_merge_parts(self._h, C.c_void_p(gathered.data_ptr()), stride_bytes, part_count,
                                          C.c_void_p(stream_ptr or 0)))

    def load_state(self, state: AccumState) -> None:
        """Continue `state`'s frame here.  Raises RtwError naming the field when the state belongs to another
        world, geometry, max_depth, render mode, seed or flags."""
        i = N.AccumInfo()
        for n in _HEADER:
            setattr(i, n, getattr(state, n))
        # the clamp pair refuses what the flags do not call for, and another level by name
        clamp_pair = self.clamp is not None or state.clamped is not None or state.lost is not None
        arr = {}
        for name, _, dtype, shape, _ in _ARRAYS:
            a = getattr(state, name)
            arr[name] = None if a is None else np.ascontiguousarray(a, dtype)
            if arr[name] is None:
                continue
            if name in _CONVERTED:
                if arr[name].size != 3 * state.slots:
                    raise ValueError("state arrays do not hold 3 * slots floats")
            elif arr[name].shape != _dims(shape, state.slots, self.tiles):
                if clamp_pair:
                    raise ValueError(f"state.{name} does not have shape {_dims(shape, state.slots, self.tiles)}")
                raise ValueError(f"state.{name} does not hold one entry per {'tile' if shape[0] == 'tiles' else 'slot'}")
        p = {name: _pointer(a) for name, a in arr.items()}
        if clamp_pair:
            check(lib().rtw_accum_import_state_clamp(self._h, C.byref(i), p["sums"], p["squares"], p["tile_stop"], p["kept"],
                                                     p["clamped"], p["lost"]))
        elif self.finite or state.kept is not None:  # the one pair: it refuses what the flags do not call for
            check(lib().rtw_accum_import_state(self._h, C.byref(i), p["sums"], p["squares"], p["tile_stop"], p["kept"]))
        elif state.tile_stop is not None:
            check(lib().rtw_accum_import_adaptive(self._h, C.byref(i), p["sums"], p["squares"], p["tile_stop"]))
        else:  # (refused by an adaptive accumulator: its state includes the stop map)
            check(lib().rtw_accum_import(self._h, C.byref(i), p["sums"], p["squares"]))


def merge_parts_host(like: AccumState, gathered: np.ndarray, stride_bytes: int, part_count: int) -> AccumState:
    """rtw_accum_merge_parts_host: the whole image's state from `part_count` packed records in the host array
    `gathered` (record r at byte r * stride_bytes), without a GPU.  `like` is any state of the frame (a part's or
    the whole's): its geometry and flags size the arrays, and its other header fields are carried over.  Raises
    RtwError naming the field, as `Accumulator.merge_parts` does."""
    flags = int(like.flags)
    p = render_params(Size2i(int(like.width), int(like.height)), 0, int(like.max_depth), RenderMode(int(like.render_mode)),
                      int(like.seed), tile=(int(like.tile_width), int(like.tile_height)))
    per_tile, n_tiles = int(like.tile_width) * int(like.tile_height), like._frame_tiles()
    slots = n_tiles * per_tile
    buf = np.ascontiguousarray(gathered).view(np.uint8).ravel()
    need = max(0, part_count - 1) * stride_bytes + N.packed_bytes(p, flags, max(1, part_count))
    if stride_bytes > 0 and buf.size < need:
        raise ValueError(f"the gathered array holds fewer than the {need} bytes of {part_count} records")
    arrays = _zeros(flags, slots, n_tiles)
    ptr = [_pointer(arrays[name]) for name, *_ in _ARRAYS]  # (the C calls take them in the record's order)
    samples = C.c_uint32()
    if flags & N.ACCUM_CLAMP:  # (records of another level than `like`'s are refused naming clamp)
        check(lib().rtw_accum_merge_parts_host_clamp(C.byref(p), flags, like.clamp, C.c_void_p(buf.ctypes.data), stride_bytes,
                                                     part_count, *ptr, C.byref(samples)))
    else:
        sums, squares, kept, _, _, stop = ptr
        check(lib().rtw_accum_merge_parts_host(C.byref(p), flags, C.c_void_p(buf.ctypes.data), stride_bytes, part_count,
                                               sums, squares, kept, stop, C.byref(samples)))
    head = like.header()
    head.update(part_index=0, part_count=1, samples=int(samples.value), slots=slots)
    return AccumState(**head, **arrays)


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


def render_finite(size: Size2i, spp: int, max_depth: int, world, **kw):
    """`spp` samples per pixel through a finite accumulator: returns (image, rejected), the mean of each pixel's
    finite samples ((W*H, 3) f32; +0 where none was finite) and the samples left out per pixel ((W*H, 1) uint32)."""
    if spp < 1:
        raise ValueError("spp must be >= 1")
    kw["finite"] = True
    acc = Accumulator(world, size, max_depth, **kw)
    try:
        acc.add(spp)
        return acc.image(), acc.rejected_counts()
    finally:
        acc.release()


def render_clamped(size: Size2i, spp: int, max_depth: int, world, clamp: float, **kw):
    """`spp` samples per pixel through a clamp accumulator of level `clamp`: returns (image, clamped, loss), the mean
    of each pixel's clamped finite samples ((W*H, 3) f32), the samples the clamp scaled per pixel ((W*H, 1) uint32)
    and the mean radiance it removed ((W*H, 3) f32)."""
    if spp < 1:
        raise ValueError("spp must be >= 1")
    kw["clamp"] = clamp
    acc = Accumulator(world, size, max_depth, **kw)
    try:
        acc.add(spp)
        return acc.image(), acc.clamped_counts(), acc.clamp_loss()
    finally:
        acc.release()


def render_to_noise(size: Size2i, max_depth: int, world, target: float, max_samples: int, batch: int = 16, **kw):
    """Adds `batch` samples at a time (the last batch cut to `max_samples`) until noise() <= target or
    samples == max_samples.  Returns (image, samples, noise).  Keyword arguments go to `Accumulator` (finite=True and
    clamp=L among them)."""
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


def render_adaptive(size: Size2i, max_depth: int, world, target: float, max_samples: int, min_samples: int = 16,
                    batch: int = 16, **kw):
    """Adds `batch` samples at a time (the last batch cut to `max_samples`) to the active tiles and, from
    `min_samples` on, stops the tiles whose worst pixel's relative standard error is at most `target`
    (`Accumulator.adapt`), until no tile is active or samples == max_samples.  Returns (image, sample_counts,
    info): info = {"samples": the frontier, "samples_rendered": the sum of the counts over the owned pixels,
    "active_tiles", "noise"}.  Every tile of the image equals `render` at its own count (with finite=True, passed
    on to `Accumulator`: on the pixels without a rejected sample)."""
    if max_samples < 2 or batch < 1 or min_samples < 2:
        raise ValueError("max_samples and min_samples must be >= 2 and batch >= 1")
    kw["adaptive"] = True
    acc = Accumulator(world, size, max_depth, **kw)
    try:
        active = acc.tiles
        while active > 0 and acc.samples < max_samples:
            acc.add(min(batch, max_samples - acc.samples))
            if acc.samples >= min_samples:
                active = acc.adapt(target, min_samples)[0]
        counts = acc.sample_counts()
        info = {"samples": acc.samples, "samples_rendered": int(counts.astype(np.int64).sum()), "active_tiles": active,
                "noise": acc.noise()[0]}
        return acc.image(), counts, info
    finally:
        acc.release()
