"""numpy restatement of the adaptive accumulator's arithmetic (include/rtw_adapt.h, rtw.h): the per-pixel
relative error in f32, the per-tile maximum and the stop rule.  Shared by test_adaptive_host.py (against the
host twin) and test_gpu_adaptive.py (the replay)."""
import numpy as np

from raytracinginaweekend_amd.distributed import tile_slots

f32 = np.float32


def pixel_stats(sums, squares, n):
    """(se, mean, e) per slot in f32, the order of rtw.h; n: a count, or one per slot."""
    n = np.broadcast_to(np.asarray(n, np.int64), sums.shape[:1])
    with np.errstate(all="ignore"):
        nf = n.astype(f32)[:, None]
        nm1 = (n - 1).astype(f32)[:, None]
        mean = sums / nf
        d = squares - sums * mean
        var = np.where(d < 0, f32(0), d) / nm1  # a NaN d stays NaN
        se = np.sqrt(var / nf)
        e = ((se[:, 0] + se[:, 1]) + se[:, 2]) / (((mean[:, 0] + mean[:, 1]) + mean[:, 2]) + f32(0.01))
    assert se.dtype == mean.dtype == e.dtype == np.float32
    return se, mean, e


def tile_max(e, owned, per_tile):
    """E per tile: the maximum of the finite e of its owned slots, 0 where there is none."""
    ok = owned & np.isfinite(e)
    E = np.where(ok, e, -np.inf).astype(f32).reshape(-1, per_tile).max(axis=1)
    return np.where(np.isneginf(E), f32(0), E)


def tiles_E(sums, squares, n, size, tile, part):
    owned = tile_slots(size, tile, part) >= 0
    return tile_max(pixel_stats(sums, squares, n)[2], owned, tile[0] * tile[1])


def stop_rule(stop, E, n, target, min_samples):
    """The stop map after an adapt at n samples (stopped tiles stay as they are)."""
    hit = (stop == 0) & (n >= min_samples) & (E <= f32(target))
    return np.where(hit, np.uint32(n), stop).astype(np.uint32)


def expand(per_tile_values, per_tile):
    """One value per tile -> one per slot."""
    return np.repeat(np.asarray(per_tile_values), per_tile)
