"""First-hit AOVs: albedo, normal and depth of the camera rays (rtw_aov_*, include/rtw.h).

An `AovAccumulator` keeps per-pixel running sums of what the camera rays hit first.  An AOV sample is one camera
ray and one closest hit, no bounce, traced by a small kernel of its own; it draws the (seed, pixel, sample) stream
of the colour sample, so AOV sample s describes the primary ray of colour sample s.  The normal image is
bit-identical to a `RenderMode.Normals` frame of the same seed and sample count; the albedo image is what the
denoiser divides out of a textured image before it filters (`Denoiser.run(..., albedo=)`), and it pays to run it
well past the colour's sample count: a demodulation is only as good as its albedo.  An add costs 0.1-0.3x a colour
add of as many samples on sphere, rect and textured worlds and as much as the colour add on a triangle mesh
(DESIGN.md 5.5f has the times).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._native import check, lib
from .rendering import DEFAULT_SEED, DeviceWorld, Size2i, render_params
from .world import World

_CHANNELS = {"albedo": N.AOV_ALBEDO, "normal": N.AOV_NORMAL, "depth": N.AOV_DEPTH}


class AovAccumulator:
    """The first-hit AOVs of one World on one GPU, over the whole image (rtw_aov_create).

    world: a `World` (uploaded here) or a `DeviceWorld` (shared with colour accumulators and one-shot frames,
    which it leaves alone).  channels: which of "albedo", "normal", "depth" to keep."""

    def __init__(self, world: World | DeviceWorld, size: Size2i, *, seed: int = DEFAULT_SEED, device: int = 0,
                 channels=("albedo", "normal", "depth")):
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
        self.params = render_params(size, 0, 0, seed=seed)
        bits = 0
        for c in channels:
            bits |= _CHANNELS[c]
        h = C.c_void_p()
        check(lib().rtw_aov_create(self.dworld._h, C.byref(self.params), bits, C.byref(h)))
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

    def _resolve_device(self, channel: str):
        import torch

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
