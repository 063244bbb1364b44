"""numpy restatement of finite-sample accumulation (include/rtw_finite.h): the filter, the in-order sums, squares
and kept counts, and the resolves with each pixel's own kept as its n.  Shared by test_finite_host.py (against
the host twins) and test_gpu_finite.py (against the device)."""
import numpy as np

from oracle import pyoracle as O
from raytracinginaweekend_amd.distributed import tile_slots
from tests import adaptive_ref as A

f32 = np.float32
_samples = {}


def finite(colors):
    """True per sample where all three channels satisfy fabsf(x) < inf."""
    with np.errstate(invalid="ignore"):
        return (np.abs(colors) < np.inf).all(axis=-1)


def accumulate(colors, sums=None, squares=None, kept=None, moments=True):
    """colors (n, slots, 3) in sample order onto (sums, squares, kept); fresh zeros when not given.  Returns new
    arrays (squares None without moments)."""
    slots = colors.shape[1]
    sums = np.zeros((slots, 3), f32) if sums is None else sums.copy()
    squares = (np.zeros((slots, 3), f32) if squares is None else squares.copy()) if moments else None
    kept = np.zeros(slots, np.uint32) if kept is None else kept.copy()
    with np.errstate(all="ignore"):
        for c in colors:
            ok = finite(c)
            sums[ok] = sums[ok] + c[ok]
            if moments:
                squares[ok] = squares[ok] + c[ok] * c[ok]
            kept[ok] += np.uint32(1)
    assert sums.dtype == np.float32 and kept.dtype == np.uint32
    return sums, squares, kept


def mean(sums, kept):
    """sum / (float)kept; +0.0 where kept == 0."""
    with np.errstate(all="ignore"):
        m = sums / kept.astype(f32)[:, None]
    return np.where((kept == 0)[:, None], f32(0), m).astype(f32)


def stats(sums, squares, kept):
    """(se, e) per slot: rtw_adapt_se / rtw_adapt_pixel with n = kept (not finite where kept < 2)."""
    se, _, e = A.pixel_stats(sums, squares, kept)
    return se, e


def noise(e, owned):
    """(the f64 mean of the finite e of the owned slots, their number)."""
    ok = owned & np.isfinite(e)
    return (float(e[ok].astype(np.float64).mean()) if ok.any() else 0.0), int(ok.sum())


def tiles_E(sums, squares, kept, size, tile, part):
    owned = tile_slots(size, tile, part) >= 0
    return A.tile_max(stats(sums, squares, kept)[1], owned, tile[0] * tile[1])


def oracle_samples(world, params, n):
    """The oracle's colour of samples 0 .. n-1 of every pixel: (n, W*H, 3) f32, pixels in image order.  Cached
    per (world, geometry, depth, seed): rendering them is the slow part of these tests."""
    w, h = params.width, params.height
    key = (id(world), w, h, params.max_depth, params.seed, n)
    if key not in _samples:
        _samples[key] = np.stack([np.stack([O.sample_color(world, params, i % w, i // w, s) for i in range(w * h)])
                                  for s in range(n)]).astype(f32)
    return _samples[key]


def to_slots(per_pixel, slots):
    """(..., W*H, 3) f32 in image order -> (..., slots, 3) in slot order.  Padding slots hold NaN: as colours the
    filter leaves them out, so their sums, squares and kept stay zero as on the device."""
    out = np.full(per_pixel.shape[:-2] + (len(slots),) + per_pixel.shape[-1:], np.nan, per_pixel.dtype)
    out[..., slots >= 0, :] = per_pixel[..., slots[slots >= 0], :]
    return out
