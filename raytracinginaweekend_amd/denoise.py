"""A variance-guided a-trous filter for previews (rtw_denoiser_*, include/rtw.h).

The filter takes a colour image, the standard error of its channels (`Accumulator.stderr()`) and an optional
guide image of up to 4 channels per pixel (a `RenderMode.Normals` frame, say), all in image layout, and smooths
the colour where its neighbours agree within their noise and within the guide.  The arithmetic is a fixed f32
expression (include/rtw_denoise.h): `Denoiser.run` (HIP kernels), `denoise_host` (the host twin, no GPU) and a
numpy restatement give the same bits.  Pixels whose colour, error or guide is not finite are left out: they pass
through bit for bit and no other pixel reads them.

This is a preview filter.  It removes noise at the price of detail the noise hides (an image texture's contrast
at 8 spp); the exact image stays `Accumulator.image()`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._native import check, lib
from .rendering import Size2i


def _params(size: Size2i, gc: int, iterations: int, sigma_l: float, sigma_g: float) -> N.DenoiseParams:
    return N.DenoiseParams(size.width, size.height, int(iterations), int(gc), float(sigma_l), float(sigma_g), 0, 0)


def _shape_check(name: str, a, pixels: int, channels: int | None) -> int:
    """The channel count of an (pixels, channels) array; ValueError for another shape."""
    shape = tuple(a.shape)
    if len(shape) != 2 or shape[0] != pixels or (channels is not None and shape[1] != channels) or shape[1] > 4:
        want = f"({pixels}, {channels})" if channels is not None else f"({pixels}, 0..4)"
        raise ValueError(f"{name} has shape {shape}, not {want}")
    return shape[1]


def _host_array(name: str, a, pixels: int, channels: int | None) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32)
    _shape_check(name, a, pixels, channels)
    return a


def _f32p(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def denoise_host(size: Size2i, color, stderr, guide=None, *, albedo=None, iterations: int = 3, sigma_l: float = 1.5,
                 sigma_g: float = 0.35, variance: bool = False):
    """`Denoiser.run` on the host (rtw_denoise_host_albedo): numpy arrays in, the same bits out, no GPU."""
    n = size.width * size.height
    color = _host_array("color", color, n, 3)
    stderr = _host_array("stderr", stderr, n, 3)
    if guide is not None:
        guide = _host_array("guide", guide, n, None)
    if albedo is not None:
        albedo = _host_array("albedo", albedo, n, 3)
    gc = 0 if guide is None else guide.shape[1]
    out = np.empty((n, 3), np.float32)
    var = np.empty(n, np.float32) if variance else None
    p = _params(size, gc, iterations, sigma_l, sigma_g)
    check(lib().rtw_denoise_host_albedo(C.byref(p), _f32p(color), _f32p(stderr), _f32p(guide if gc else None),
                                        _f32p(albedo), _f32p(out), _f32p(var)))
    return (out, var) if variance else out


class Denoiser:
    """The filter's device scratch for frames of one size (rtw_denoiser_create): 48 bytes per pixel."""

    def __init__(self, size: Size2i, device: int = 0):
        self._h = None
        self.size = size
        self.device = device
        h = C.c_void_p()
        check(lib().rtw_denoiser_create(device, size.width, size.height, C.byref(h)))
        self._h = h

    def release(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().rtw_denoiser_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def run_device(self, color, stderr, guide=None, out=None, *, albedo=None, iterations: int = 3, sigma_l: float = 1.5,
                   sigma_g: float = 0.35, variance: bool = False, stream_ptr: int | None = None):
        """The filter on torch tensors of this device (f32, contiguous; color and stderr (W*H, 3), guide (W*H, gc),
        albedo (W*H, 3) or None); asynchronous on `stream_ptr` (default: torch's current stream).  `out` may be
        `color`.  Returns out, or (out, variance)."""
        import torch

        n = self.size.width * self.size.height
        dev = torch.device("cuda", self.device)
        gc = 0 if guide is None else _shape_check("guide", guide, n, None)
        _shape_check("color", color, n, 3)
        _shape_check("stderr", stderr, n, 3)
        if albedo is not None:
            _shape_check("albedo", albedo, n, 3)
        for name, t in (("color", color), ("stderr", stderr), ("guide", guide), ("albedo", albedo), ("out", out)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev):
                raise ValueError(f"{name} is not a contiguous float32 tensor on {dev}")
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        else:
            _shape_check("out", out, n, 3)
        var = torch.empty(n, dtype=torch.float32, device=dev) if variance else None
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(dev).cuda_stream
        p = _params(self.size, gc, iterations, sigma_l, sigma_g)
        check(lib().rtw_denoiser_run_albedo(
            self._h, C.byref(p), C.c_void_p(color.data_ptr()), C.c_void_p(stderr.data_ptr()),
            C.c_void_p(guide.data_ptr() if gc else 0), C.c_void_p(albedo.data_ptr() if albedo is not None else 0),
            C.c_void_p(out.data_ptr()), C.c_void_p(var.data_ptr() if variance else 0), C.c_void_p(stream_ptr or 0)))
        return (out, var) if variance else out

    def run(self, color, stderr, guide=None, *, albedo=None, iterations: int = 3, sigma_l: float = 1.5,
            sigma_g: float = 0.35, variance: bool = False):
        """Filters `color` ((W*H, 3) f32) by its standard error `stderr` ((W*H, 3)) and, when given, the guide
        ((W*H, gc), gc <= 4).  numpy arrays are copied to the device and the result comes back as numpy; torch
        tensors of this device are filtered where they are, without a copy, and the result is a tensor (`run_device`).
        Returns the (W*H, 3) f32 image, with variance=True also the (W*H,) variance of each pixel's filtered
        luminance estimate (NaN where the pixel was left out).

        albedo ((W*H, 3), an `AovAccumulator.albedo()` say): the filter runs on color / D and stderr / D with
        D = max(albedo, 1/64) per channel and the result is multiplied by D again, so that a texture's contrast is
        not taken for noise; the variance is then that of the demodulated luminance.  Use an albedo that is better
        converged than the colour."""
        import torch

        opts = dict(iterations=iterations, sigma_l=sigma_l, sigma_g=sigma_g, variance=variance)
        if hasattr(color, "data_ptr"):  # a torch tensor
            return self.run_device(color, stderr, guide, albedo=albedo, **opts)
        n = self.size.width * self.size.height
        dev = torch.device("cuda", self.device)
        arrays = [_host_array("color", color, n, 3), _host_array("stderr", stderr, n, 3),
                  None if guide is None else _host_array("guide", guide, n, None),
                  None if albedo is None else _host_array("albedo", albedo, n, 3)]
        if arrays[2] is not None and arrays[2].shape[1] == 0:
            arrays[2] = None
        tensors = [None if a is None else torch.from_numpy(a).to(dev) for a in arrays]
        res = self.run_device(*tensors[:3], albedo=tensors[3], **opts)
        torch.cuda.current_stream(dev).synchronize()
        if variance:
            return res[0].cpu().numpy(), res[1].cpu().numpy()
        return res.cpu().numpy()
