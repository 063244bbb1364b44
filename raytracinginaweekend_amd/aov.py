"""First-hit AOVs: albedo, normal and depth of the camera rays (rtw_aov_*, include/rtw.h).

An `AovAccumulator` keeps per-pixel running sums of what the camera rays hit first.  An AOV sample is one camera
ray and one closest hit, no bounce, traced by a small kernel of its own; it draws the (seed, pixel, sample) stream
of the colour sample, so AOV sample s describes the primary ray of colour sample s.  The normal image is
bit-identical to a `RenderMode.Normals` frame of the same seed and sample count; the albedo image is what the
denoiser divides out of a textured image before it filters (`Denoiser.run(..., albedo=)`), and it pays to run it
well past the colour's sample count: a demodulation is only as good as its albedo.  An add costs 0.1-0.3x a colour
add of as many samples on sphere, rect and textured worlds and as much as the colour add on a triangle mesh
(DESIGN.md 5.5f has the times).

Across GPUs (distributed.py has the rank wrapper): `AovAccumulator(..., part=(r, N))` holds the
8 x 8 tiles t = r, r + N, ... of the frame, the colour accumulators' partition; `pack_into` writes its planes as
one record (include/rtw_aov_parts.h), the records are gathered, and `merge_parts` places them into an accumulator
of part (0, 1), which then is, bit for bit, the accumulator one GPU would hold.  `AovState` is the checkpoint of
any part; `AovState.merge` / `AovState.split` do the placement in numpy, so one written by N ranks resumes on M.
`AovState` needs neither a GPU nor librtw.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from . import _parts
from ._native import check, lib
from .rendering import DEFAULT_SEED, DeviceWorld, Size2i, render_params
from .world import World

_CHANNELS = {"albedo": N.AOV_ALBEDO, "normal": N.AOV_NORMAL, "depth": N.AOV_DEPTH}

RECORD_VERSION = _parts.VERSION  # RTW_PARTS_VERSION
RECORD_HEADER_WORDS = _parts.HEADER_WORDS
RECORD_MAGIC = 0x564F4152  # RTW_AOV_PARTS_MAGIC
PER_TILE = 64  # a wave is an 8 x 8 tile

_HEADER = {n: np.dtype(t) for n, t in N.AovStateInfo._fields_}
_PLANES = (("albedo", 3), ("normal", 3), ("depth", 1), ("hits", 1))  # the record's order


def frame_tiles(width: int, height: int) -> int:
    return -(-width // 8) * -(-height // 8)


def record_layout(width: int, height: int, channels: int, part_count: int) -> dict:
    """The packed record of include/rtw_aov_parts.h in numpy's terms: n_tiles, tiles0, slots0, the word offsets
    albedo / normal / depth (None: the channel is not held) / hits, planes and words."""
    held = [(name, name == "hits" or bool(channels & _CHANNELS[name]), count * PER_TILE) for name, count in _PLANES]
    lay = _parts.section_offsets(frame_tiles(width, height), part_count, PER_TILE, held)
    lay["planes"] = sum(words // PER_TILE for _, has, words in held if has)
    return lay


@dataclass
class AovState:
    """One AOV accumulator's exported state: the fields of rtw_aov_state_info and the planes as the device holds
    them -- albedo and normal float32 of shape (3, slots), depth float32 and hits uint32 of shape (slots,); a
    channel the accumulator does not hold is None.  slots = tiles * 64, slot = local tile * 64 + y * 8 + x;
    padding slots of edge tiles hold zeros."""

    version: int
    channels: int
    width: int
    height: int
    samples: int
    part_index: int
    part_count: int
    slots: int
    tiles: int
    reserved: int
    seed: int
    world_fingerprint: int
    hits: np.ndarray
    albedo: np.ndarray | None = None
    normal: np.ndarray | None = None
    depth: np.ndarray | None = None

    def header(self) -> dict:
        return {n: int(getattr(self, n)) for n in _HEADER}

    def _shape(self, name: str) -> tuple:
        return (3, int(self.slots)) if name in ("albedo", "normal") else (int(self.slots),)

    def _check_arrays(self) -> None:
        for name, _ in _PLANES:
            a = getattr(self, name)
            held = name == "hits" or bool(int(self.channels) & _CHANNELS[name])
            if held != (a is not None):
                raise ValueError(f"{name} does not go with the channels")
            if a is not None:
                want = np.uint32 if name == "hits" else np.float32
                if np.asarray(a).dtype != want or np.asarray(a).shape != self._shape(name):
                    raise ValueError(f"{name} is not {np.dtype(want)} of shape {self._shape(name)}")

    def save(self, path) -> None:
        """One .npz of plain arrays (numpy.savez): a 0-d array per header field and the planes held."""
        self._check_arrays()
        arrays = {n: np.asarray(getattr(self, n), dtype=t) for n, t in _HEADER.items()}
        for name, _ in _PLANES:
            if getattr(self, name) is not None:
                arrays[name] = np.ascontiguousarray(getattr(self, name))
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path) -> "AovState":
        """Reads a file written by `save`.  Nothing is unpickled: a file holding anything but the plain arrays
        `save` writes is refused."""
        with np.load(path, allow_pickle=False) as z:
            names = set(z.files)
            known = set(_HEADER) | {n for n, _ in _PLANES}
            if names - known:
                raise ValueError(f"not an AOV checkpoint: unexpected entries {sorted(names - known)}")
            missing = (set(_HEADER) | {"hits"}) - names
            if missing:
                raise ValueError(f"not an AOV checkpoint: missing entries {sorted(missing)}")
            vals = {}
            for n, t in _HEADER.items():
                a = z[n]
                if a.dtype != t or a.shape != ():
                    raise ValueError(f"AOV checkpoint: bad header field {n}")
                vals[n] = int(a)
            state = cls(**vals, **{name: z[name] for name, _ in _PLANES if name in names})
        state._check_arrays()
        return state

    @classmethod
    def merge(cls, states) -> "AovState":
        """The whole image's state (part (0, 1)) from the states of parts (0..N-1, N) of one frame, in any order:
        a placement of tile blocks, bit for bit the state one accumulator would hold.  Raises ValueError naming
        the field when the states differ in version, channels, size, samples, seed or world_fingerprint, when a
        part is missing or comes twice, and when slots, tiles or an array does not fit the part."""
        states = list(states)
        by_part = _parts.parts_in_order(states, ("version", "channels", "width", "height", "part_count", "reserved", "seed",
                                                 "world_fingerprint", "samples"))
        first, count = states[0], len(by_part)
        n_tiles = frame_tiles(int(first.width), int(first.height))
        slots = n_tiles * PER_TILE
        head = first.header()
        head.update(part_index=0, part_count=1, slots=slots, tiles=n_tiles)
        whole = cls(**head, hits=np.zeros(slots, np.uint32))
        for name, _ in _PLANES[:3]:
            if int(first.channels) & _CHANNELS[name]:
                setattr(whole, name, np.zeros(whole._shape(name), np.float32))
        for r in range(count):
            s = by_part[r]
            at = _parts.part_slots(n_tiles, PER_TILE, (r, count))
            if int(s.slots) != at.size:
                raise ValueError(f"part {r}: slots differs from the partition's ({at.size})")
            if int(s.tiles) != at.size // PER_TILE:
                raise ValueError(f"part {r}: tiles differs from the partition's ({at.size // PER_TILE})")
            s._check_arrays()
            for name, _ in _PLANES:
                dst = getattr(whole, name)
                if dst is not None:  # (bit patterns, not values: a NaN's payload travels)
                    dst.view(np.uint32)[..., at] = np.asarray(getattr(s, name)).view(np.uint32)
        return whole

    def split(self, part_count: int) -> list["AovState"]:
        """The inverse of `merge`: the states of parts (0..part_count-1, part_count) of this whole-image state.
        `merge(s.split(M))` is `s` for every M, so `merge` then `split(M)` re-partitions the checkpoints of N ranks
        for M (each loads its part with `AovAccumulator.load_state`).  A part without tiles (M above the frame's
        tile count) holds empty planes and the frame's sample count."""
        if (int(self.part_index), max(1, int(self.part_count))) != (0, 1):
            raise ValueError("split needs the whole image's state: part_index / part_count is not 0 / 1")
        if part_count < 1:
            raise ValueError("part_count must be >= 1")
        n_tiles = frame_tiles(int(self.width), int(self.height))
        if int(self.slots) != n_tiles * PER_TILE or int(self.tiles) != n_tiles:
            raise ValueError("slots or tiles differs from the frame's")
        self._check_arrays()
        out = []
        for r in range(part_count):
            at = _parts.part_slots(n_tiles, PER_TILE, (r, part_count))
            head = self.header()
            head.update(part_index=r, part_count=part_count, slots=int(at.size), tiles=int(at.size) // PER_TILE)
            out.append(AovState(**head, **{name: np.ascontiguousarray(getattr(self, name)[..., at])
                                           for name, _ in _PLANES if getattr(self, name) is not None}))
        return out

    def packed(self, stride_bytes: int | None = None) -> np.ndarray:
        """This state as the record `AovAccumulator.pack_into` writes (uint32 words, include/rtw_aov_parts.h),
        padded with zeros to `stride_bytes`: what a rank without device-aware collectives sends."""
        self._check_arrays()
        count = max(1, int(self.part_count))
        lay = record_layout(int(self.width), int(self.height), int(self.channels), count)
        header = (RECORD_VERSION, int(self.channels), int(self.part_index), count, int(self.samples), int(self.slots),
                  int(self.tiles), RECORD_MAGIC)
        planes = [(lay[name] + k * lay["slots0"], np.asarray(getattr(self, name)).reshape(count_, -1)[k])
                  for name, count_ in _PLANES if getattr(self, name) is not None for k in range(count_)]
        return _parts.pack_record(header, lay["words"], stride_bytes, planes)


assert list(_HEADER) == [f for f in AovState.__dataclass_fields__][:len(_HEADER)]


def _f32p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _u32p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))


def aov_packed_bytes(size: Size2i, channels: int, part_count: int) -> int:
    """rtw_aov_packed_bytes: the bytes of one part's packed AOV record (host only)."""
    n = C.c_int64()
    check(lib().rtw_aov_packed_bytes(C.byref(render_params(size, 0, 0)), channels, part_count, C.byref(n)))
    return n.value


def merge_parts_host(like: AovState, gathered: np.ndarray, stride_bytes: int, part_count: int) -> AovState:
    """rtw_aov_merge_parts_host: the whole image's state from `part_count` packed records in the host array
    `gathered` (record r at byte r * stride_bytes), without a GPU.  `like` is any state of the frame (a part's or
    the whole's): its size and channels size the arrays, and its other header fields are carried over.  Raises
    RtwError naming the field, as `AovAccumulator.merge_parts` does."""
    size, channels = Size2i(int(like.width), int(like.height)), int(like.channels)
    n_tiles = frame_tiles(size.width, size.height)
    slots = n_tiles * PER_TILE
    buf = np.ascontiguousarray(gathered).view(np.uint8).ravel()
    if stride_bytes > 0 and part_count >= 1:
        need = (part_count - 1) * stride_bytes + aov_packed_bytes(size, channels, part_count)
        if buf.size < need:
            raise ValueError(f"the gathered array holds fewer than the {need} bytes of {part_count} records")
    head = like.header()
    head.update(part_index=0, part_count=1, slots=slots, tiles=n_tiles)
    whole = AovState(**head, hits=np.zeros(slots, np.uint32))
    for name, _ in _PLANES[:3]:
        if channels & _CHANNELS[name]:
            setattr(whole, name, np.zeros(whole._shape(name), np.float32))
    samples = C.c_uint32()
    check(lib().rtw_aov_merge_parts_host(C.byref(render_params(size, 0, 0)), channels, C.c_void_p(buf.ctypes.data), stride_bytes,
                                         part_count, _f32p(whole.albedo), _f32p(whole.normal), _f32p(whole.depth),
                                         _u32p(whole.hits), C.byref(samples)))
    whole.samples = int(samples.value)
    return whole


class AovAccumulator:
    """The first-hit AOVs of one World on one GPU, over the whole image (rtw_aov_create) or, with part=(r, N), over
    the frame's 8 x 8 tiles t = r, r + N, ... (rtw_aov_create_part).

    world: a `World` (uploaded here) or a `DeviceWorld` (shared with colour accumulators and one-shot frames,
    which it leaves alone).  channels: which of "albedo", "normal", "depth" to keep.  A part is not resolved: it
    is read through `state()` or, packed and gathered with the others, after `merge_parts` into the whole."""

    def __init__(self, world: World | DeviceWorld, size: Size2i, *, seed: int = DEFAULT_SEED, device: int = 0,
                 channels=("albedo", "normal", "depth"), part: tuple[int, int] = (0, 1)):
        self._h = None
        channels = tuple(channels)
        unknown = [c for c in channels if c not in _CHANNELS]
        if unknown:
            raise ValueError(f"unknown AOV channels {unknown}: choose from {sorted(_CHANNELS)}")
        if not channels:
            raise ValueError("channels is empty: name at least one AOV channel")
        self.channels = channels
        self.dworld = world if isinstance(world, DeviceWorld) else DeviceWorld(world, device)
        self.device = self.dworld.device
        self.size = size
        self.part = (int(part[0]), int(part[1]))
        whole = self.part == (0, 1)
        self.params = render_params(size, 0, 0, seed=seed) if whole else render_params(size, 0, 0, seed=seed, part=self.part,
                                                                                       layout=N.LAYOUT_TILES)
        bits = 0
        for c in channels:
            bits |= _CHANNELS[c]
        self.channel_bits = bits
        h = C.c_void_p()
        create = lib().rtw_aov_create if whole else lib().rtw_aov_create_part
        check(create(self.dworld._h, C.byref(self.params), bits, C.byref(h)))
        self._h = h

    def release(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().rtw_aov_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def info(self) -> N.AovInfo:
        i = N.AovInfo()
        check(lib().rtw_aov_get_info(self._h, C.byref(i)))
        return i

    @property
    def samples(self) -> int:
        """Samples per pixel added so far."""
        return int(self.info().samples)

    def add(self, n: int, stream_ptr: int | None = None) -> None:
        """Traces the next `n` camera samples of every pixel and adds them (asynchronous; default: torch's current
        stream, the one the resolves below run on)."""
        if n < 0 or n > 0xFFFFFFFF:
            raise ValueError("n must be in 0 .. 2^32 - 1")
        if stream_ptr is None:
            stream_ptr = self._stream()
        check(lib().rtw_aov_add(self._h, n, C.c_void_p(stream_ptr or 0)))

    def _stream(self) -> int:
        import torch

        return torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream

    def state_info(self) -> N.AovStateInfo:
        i = N.AovStateInfo()
        check(lib().rtw_aov_get_state_info(self._h, C.byref(i)))
        return i

    @property
    def tiles(self) -> int:
        """The 8 x 8 tiles this accumulator holds (the whole frame's, or the part's own)."""
        return int(self.state_info().tiles)

    def packed_bytes(self) -> int:
        """The bytes of this accumulator's packed record (the same for every part of its part_count)."""
        return aov_packed_bytes(self.size, self.channel_bits, self.part[1])

    def pack_into(self, tensor, stream_ptr: int | None = None) -> None:
        """Writes the accumulator's planes as one packed record (include/rtw_aov_parts.h) into the device tensor
        (at least `packed_bytes()` bytes; asynchronous; default: torch's current stream)."""
        if not tensor.is_cuda or not tensor.is_contiguous() or tensor.numel() * tensor.element_size() < self.packed_bytes():
            raise ValueError("pack_into needs a contiguous device tensor of at least packed_bytes() bytes")
        if stream_ptr is None:
            stream_ptr = self._stream()
        check(lib().rtw_aov_pack(self._h, C.c_void_p(tensor.data_ptr()), C.c_void_p(stream_ptr or 0)))

    def merge_parts(self, gathered, stride_bytes: int, part_count: int, stream_ptr: int | None = None) -> None:
        """Replaces this whole-image accumulator's planes (part (0, 1)) by the merge of `part_count` packed records,
        record r at byte r * stride_bytes of the device tensor `gathered` (rtw_aov_merge_parts).  Raises RtwError
        naming the field for records of another version, kind, channels, order, part_count or geometry, a bad
        stride and unequal samples; nothing is launched then."""
        if not gathered.is_cuda or not gathered.is_contiguous():
            raise ValueError("merge_parts needs a contiguous device tensor")
        if stride_bytes > 0 and part_count >= 1:
            need = (part_count - 1) * stride_bytes + aov_packed_bytes(self.size, self.channel_bits, part_count)
            if gathered.numel() * gathered.element_size() < need:
                raise ValueError(f"the gathered tensor holds fewer than the {need} bytes of {part_count} records")
        if stream_ptr is None:
            stream_ptr = self._stream()
        check(lib().rtw_aov_merge_parts(self._h, C.c_void_p(gathered.data_ptr()), stride_bytes, part_count,
                                        C.c_void_p(stream_ptr or 0)))

    def state(self) -> AovState:
        """The accumulator's planes and header on the host (synchronous)."""
        i = self.state_info()
        st = AovState(**{n: int(getattr(i, n)) for n in _HEADER}, hits=np.zeros(i.slots, np.uint32))
        for name in self.channels:
            setattr(st, name, np.zeros(st._shape(name), np.float32))
        check(lib().rtw_aov_export_state(self._h, _f32p(st.albedo), _f32p(st.normal), _f32p(st.depth), _u32p(st.hits)))
        return st

    def load_state(self, state: AovState) -> None:
        """Continue `state`'s AOVs here.  Raises RtwError naming the field when the state belongs to another
        world, size, part, seed or set of channels, or holds a hit count above its samples or a non-zero
        padding slot."""
        state._check_arrays()
        i = N.AovStateInfo()
        for n in _HEADER:
            setattr(i, n, getattr(state, n))
        planes = {name: None if getattr(state, name) is None else np.ascontiguousarray(getattr(state, name)) for name, _ in _PLANES}
        check(lib().rtw_aov_import_state(self._h, C.byref(i), _f32p(planes["albedo"]), _f32p(planes["normal"]),
                                         _f32p(planes["depth"]), _u32p(planes["hits"])))

    def _resolve_device(self, channel: str):
        import torch

        if self.part != (0, 1):
            raise ValueError(f"this AOV accumulator holds part {self.part} of the image: read it through state() or "
                             "merge the parts into a whole-image accumulator")
        dev = torch.device("cuda", self.device)
        n = self.size.width * self.size.height
        stream = C.c_void_p(self._stream() or 0)
        if channel == "hits":
            out = torch.empty(n, dtype=torch.int32, device=dev)
            check(lib().rtw_aov_hits(self._h, C.c_void_p(out.data_ptr()), stream))
            return out
        if channel not in self.channels:
            raise ValueError(f"this AOV accumulator does not hold the {channel} channel")
        out = torch.empty(n if channel == "depth" else (n, 3), dtype=torch.float32, device=dev)
        check(lib().rtw_aov_resolve(self._h, _CHANNELS[channel], C.c_void_p(out.data_ptr()), stream))
        return out

    def _resolve_host(self, channel: str) -> np.ndarray:
        import torch

        out = self._resolve_device(channel)
        torch.cuda.current_stream(out.device).synchronize()
        return out.cpu().numpy()

    def albedo_device(self):
        """The mean first-hit albedo, a (W*H, 3) f32 tensor on the device: the material's texture at the hit, 1 for
        a dielectric and on a miss (samples >= 1)."""
        return self._resolve_device("albedo")

    def normal_device(self):
        """The mean of (n + 1) / 2 at the first hit and of the background on a miss, (W*H, 3): a
        `RenderMode.Normals` frame, bit for bit."""
        return self._resolve_device("normal")

    def depth_device(self):
        """The mean hit distance over the samples that hit, (W*H,); 0 where none did."""
        return self._resolve_device("depth")

    def hits_device(self):
        """The samples of each pixel that hit something, (W*H,) int32."""
        return self._resolve_device("hits")

    def albedo(self) -> np.ndarray:
        return self._resolve_host("albedo")

    def normal(self) -> np.ndarray:
        return self._resolve_host("normal")

    def depth(self) -> np.ndarray:
        return self._resolve_host("depth")

    def hits(self) -> np.ndarray:
        return self._resolve_host("hits").view(np.uint32)


def render_aov(size: Size2i, spp: int, world, *, seed: int = DEFAULT_SEED, device: int = 0) -> dict:
    """The first-hit AOVs of `world` at `spp` camera samples per pixel: {"albedo": (W*H, 3), "normal": (W*H, 3),
    "depth": (W*H,), "hits": (W*H,) uint32}."""
    if spp < 1:
        raise ValueError("spp must be >= 1")
    aov = AovAccumulator(world, size, seed=seed, device=device)
    try:
        aov.add(spp)
        return {"albedo": aov.albedo(), "normal": aov.normal(), "depth": aov.depth(), "hits": aov.hits()}
    finally:
        aov.release()
