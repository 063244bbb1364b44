"""numpy restatement of sample clamping at the accumulate step (include/rtw_clamp.h): the per-sample step, the
in-order sums, squares, kept, clamped and lost, and the loss resolve.  The resolves, standard error, noise and the
stop test are finite_ref's on these sums, squares and kept.  Shared by test_clamp_host.py (against the host twin) and
test_gpu_clamp.py (against the device)."""
import numpy as np

from tests import finite_ref as F

f32 = np.float32


def clamp_samples(colors, level):
    """(c', hit) of finite colours (..., 3) f32: c' = c scaled by level / max channel where that channel exceeds
    the level, each channel then cut to the level; hit marks those samples.  Non-finite rows come back unchanged
    and unmarked (the caller filters them)."""
    level = f32(level)
    c = np.asarray(colors, f32)
    with np.errstate(all="ignore"):
        # max(max(r, g), b) with the header's a > b ? a : b
        m = np.where(c[..., 0] > c[..., 1], c[..., 0], c[..., 1])
        m = np.where(m > c[..., 2], m, c[..., 2])
        hit = F.finite(c) & (m > level)
        s = (level / m).astype(f32)
        scaled = (c * s[..., None]).astype(f32)
        cut = np.where(scaled < level, scaled, level).astype(f32)
    return np.where(hit[..., None], cut, c).astype(f32), hit


def accumulate(colors, level, sums=None, squares=None, kept=None, clamped=None, lost=None, moments=True):
    """colors (n, slots, 3) in sample order onto (sums, squares, kept, clamped, lost); fresh zeros when not given.
    Returns new arrays (squares None without moments)."""
    slots = colors.shape[1]
    sums = np.zeros((slots, 3), f32) if sums is None else sums.copy()
    squares = (np.zeros((slots, 3), f32) if squares is None else squares.copy()) if moments else None
    kept = np.zeros(slots, np.uint32) if kept is None else kept.copy()
    clamped = np.zeros(slots, np.uint32) if clamped is None else clamped.copy()
    lost = np.zeros((slots, 3), f32) if lost is None else lost.copy()
    with np.errstate(all="ignore"):
        for c in colors:
            ok = F.finite(c)
            v, hit = clamp_samples(c, level)
            lost[hit] = lost[hit] + (c[hit] - v[hit])
            clamped[hit] += np.uint32(1)
            sums[ok] = sums[ok] + v[ok]
            if moments:
                squares[ok] = squares[ok] + v[ok] * v[ok]
            kept[ok] += np.uint32(1)
    assert sums.dtype == lost.dtype == np.float32 and kept.dtype == clamped.dtype == np.uint32
    return sums, squares, kept, clamped, lost


def loss_mean(lost, kept):
    """lost / (float)kept; +0.0 where kept == 0."""
    return F.mean(lost, kept)
