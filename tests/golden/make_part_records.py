"""Generates tests/golden/part_records.json: SHA-256 digests of the packed partition records and of their merge
(DESIGN.md 5.5h, 5.5i), and the refusals of the host twins.  CPU only; tests/test_part_records.py recomputes
`compute()` on the current tree and compares it with the committed file, so the record format stays byte for byte
what it was when the file was written.

Every case is a synthetic whole-image state of a 44 x 26 frame from a seeded numpy generator: random u32 patterns as
float planes (NaNs with payloads, -0, +inf among them), non-zero counts, zeros in the padding slots of edge tiles.
A case's digest runs over, for the tight stride and then the stride rounded up to 16 bytes,
  every record `state.split(N)[r].packed(stride)`, r = 0 .. N - 1, then
  every array `merge_parts_host` returns from those records, in record order, then its samples (u32).
Colour: tiles (8, 8) and (5, 3), all 8 flag combinations, N in 1, 2, 3, 7 and one N above the tile count; adaptive
states hold stopped tiles, and every tile of part 1 of 3 has stopped.  AOV: all 7 channel combinations, N in
1, 2, 3, 30 (the frame has 24 tiles).  A refusal is the return code and message of the C host twin for one damaged
gather per reason it knows.

python tests/golden/make_part_records.py
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import raytracinginaweekend_amd as R  # noqa: E402
from raytracinginaweekend_amd import _native as N  # noqa: E402
from raytracinginaweekend_amd import aov as AOV  # noqa: E402
from raytracinginaweekend_amd import progressive as PROG  # noqa: E402
from raytracinginaweekend_amd.distributed import tile_slots  # noqa: E402

PATH = os.path.join(HERE, "part_records.json")
SIZE = (44, 26)
SAMPLES = 24
SPECIAL = (0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000)  # NaNs with payloads, -0, +inf


def _bits(rng, shape, owned, axis):
    a = rng.integers(1, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    a.reshape(-1)[:4] = SPECIAL
    a.reshape(-1)[-4:] = SPECIAL  # (the last part's tail too)
    if axis == 0:
        a[~owned] = 0
    else:
        a[..., ~owned] = 0
    return a.view(np.float32)


def colour_state(tile, flags, seed=19):
    rng = np.random.default_rng(seed)
    owned = tile_slots(R.Size2i(*SIZE), tile, (0, 1)) >= 0
    per_tile = tile[0] * tile[1]
    tiles = owned.size // per_tile
    stop = kept = None
    if flags & N.ACCUM_ADAPTIVE:
        stop = rng.choice(np.array([0, 0, 8, 12, 20], np.uint32), size=tiles)
        stop[:5] = (0, 8, 12, 20, 0)
        stop[1::3] = np.where(stop[1::3] == 0, np.uint32(12), stop[1::3])  # part 1 of 3: every tile has stopped
    if flags & N.ACCUM_FINITE:
        n = np.full(owned.size, SAMPLES, np.int64) if stop is None else np.repeat(np.where(stop != 0, stop, SAMPLES), per_tile).astype(np.int64)
        kept = rng.integers(1, n + 1).astype(np.uint32)
        kept[~owned] = 0
    return PROG.AccumState(version=1, flags=flags, width=SIZE[0], height=SIZE[1], tile_width=tile[0], tile_height=tile[1],
                           part_index=0, part_count=1, max_depth=50, render_mode=0, samples=SAMPLES, reserved=0, seed=77,
                           world_fingerprint=0x1234_5678_9ABC_DEF0, slots=owned.size, sums=_bits(rng, (owned.size, 3), owned, 0),
                           squares=_bits(rng, (owned.size, 3), owned, 0) if flags & N.ACCUM_MOMENTS else None,
                           tile_stop=stop, kept=kept)


def aov_state(channels, seed=23):
    rng = np.random.default_rng(seed)
    owned = tile_slots(R.Size2i(*SIZE), (8, 8), (0, 1)) >= 0
    slots = owned.size
    hits = rng.integers(1, SAMPLES + 1, size=slots).astype(np.uint32)
    hits[~owned] = 0
    return AOV.AovState(version=1, channels=channels, width=SIZE[0], height=SIZE[1], samples=SAMPLES, part_index=0, part_count=1,
                        slots=slots, tiles=slots // 64, reserved=0, seed=77, world_fingerprint=0x1234_5678_9ABC_DEF0, hits=hits,
                        albedo=_bits(rng, (3, slots), owned, 1) if channels & N.AOV_ALBEDO else None,
                        normal=_bits(rng, (3, slots), owned, 1) if channels & N.AOV_NORMAL else None,
                        depth=_bits(rng, (slots,), owned, 1) if channels & N.AOV_DEPTH else None)


def _digest(state, n, merge, names) -> str:
    h = hashlib.sha256()
    parts = state.split(n)
    tight = len(parts[0].packed()) * 4
    for stride in (tight, -(-tight // 16) * 16):
        records = [p.packed(stride) for p in parts]
        for rec in records:
            assert rec.dtype == np.uint32 and rec.size * 4 == stride
            h.update(rec.astype("<u4").tobytes())
        whole = merge(parts[-1], np.concatenate(records), stride, n)
        for name in names:
            a = getattr(whole, name)
            if a is not None:
                h.update(np.ascontiguousarray(a).view(np.uint32).astype("<u4").tobytes())
        h.update(np.uint32(whole.samples).astype("<u4").tobytes())
    return h.hexdigest()


COLOUR_ARRAYS = ("sums", "squares", "kept", "tile_stop")
AOV_ARRAYS = ("albedo", "normal", "depth", "hits")


def digests() -> dict:
    out = {}
    for tile in ((8, 8), (5, 3)):
        n_tiles = -(-SIZE[0] // tile[0]) * -(-SIZE[1] // tile[1])
        for flags in range(8):
            s = colour_state(tile, flags)
            for n in (1, 2, 3, 7, n_tiles + 6):
                out[f"colour tile {tile[0]}x{tile[1]} flags {flags} parts {n}"] = _digest(s, n, PROG.merge_parts_host, COLOUR_ARRAYS)
    for channels in range(1, 8):
        s = aov_state(channels)
        for n in (1, 2, 3, 30):
            out[f"aov channels {channels} parts {n}"] = _digest(s, n, AOV.merge_parts_host, AOV_ARRAYS)
    return out


def _colour_host(gathered, stride, count, flags, tile=(8, 8)):
    """(rc, message) of rtw_accum_merge_parts_host on arrays of the whole image's size."""
    p = R.render_params(R.Size2i(*SIZE), 0, 50, tile=tile)
    slots = tile_slots(R.Size2i(*SIZE), tile, (0, 1)).size
    g = np.ascontiguousarray(gathered, np.uint32)
    sums = np.zeros((slots, 3), np.float32)
    squares = np.zeros((slots, 3), np.float32) if flags & N.ACCUM_MOMENTS else None
    kept = np.zeros(slots, np.uint32) if flags & N.ACCUM_FINITE else None
    stop = np.zeros(slots // (tile[0] * tile[1]), np.uint32) if flags & N.ACCUM_ADAPTIVE else None
    samples = C.c_uint32()

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(C.POINTER(t))

    rc = N.lib().rtw_accum_merge_parts_host(C.byref(p), flags, C.c_void_p(g.ctypes.data), stride, count, ptr(sums, C.c_float),
                                            ptr(squares, C.c_float), ptr(kept, C.c_uint32), ptr(stop, C.c_uint32), C.byref(samples))
    return [int(rc), (N.lib().rtw_last_error() or b"").decode() if rc else ""]


def _aov_host(gathered, stride, count, channels):
    p = R.render_params(R.Size2i(*SIZE), 0, 0)
    slots = tile_slots(R.Size2i(*SIZE), (8, 8), (0, 1)).size
    g = np.ascontiguousarray(gathered, np.uint32)
    albedo = np.zeros((3, slots), np.float32) if channels & N.AOV_ALBEDO else None
    normal = np.zeros((3, slots), np.float32) if channels & N.AOV_NORMAL else None
    depth = np.zeros(slots, np.float32) if channels & N.AOV_DEPTH else None
    hits = np.zeros(slots, np.uint32)
    samples = C.c_uint32()

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(C.POINTER(t))

    rc = N.lib().rtw_aov_merge_parts_host(C.byref(p), channels, C.c_void_p(g.ctypes.data), stride, count, ptr(albedo, C.c_float),
                                          ptr(normal, C.c_float), ptr(depth, C.c_float), ptr(hits, C.c_uint32), C.byref(samples))
    return [int(rc), (N.lib().rtw_last_error() or b"").decode() if rc else ""]


def _damaged(rec, words, record, word, value=None, add=0):
    bad = rec.copy()
    at = record * words + word
    bad[at] = (int(bad[at]) + add) if value is None else value
    return bad


def refusals() -> dict:
    """One refused gather of 3 records per reason; the header's words are version, flags or channels, part_index,
    part_count, samples, slots, tiles, 0 or the AOV magic."""
    out = {}
    n = 3
    flags = N.ACCUM_MOMENTS | N.ACCUM_ADAPTIVE | N.ACCUM_FINITE
    s = colour_state((8, 8), flags)
    parts = s.split(n)
    stride = len(parts[0].packed()) * 4
    words = stride // 4
    rec = np.concatenate([p.packed(stride) for p in parts])
    stop_at = PROG.record_layout(SIZE[0], SIZE[1], (8, 8), flags, n)["stop"]
    plain = colour_state((8, 8), N.ACCUM_MOMENTS)
    plain_stride = len(plain.split(n)[0].packed()) * 4
    plain_rec = np.concatenate([p.packed(plain_stride) for p in plain.split(n)])
    colour = {
        "params": _colour_host(rec, stride, 0, flags),
        "stride_bytes": _colour_host(rec, stride - 4, n, flags),
        "stride_bytes not a multiple of 4": _colour_host(rec, stride + 2, n, flags),
        "version": _colour_host(_damaged(rec, words, 1, 0, 9), stride, n, flags),
        "flags": _colour_host(_damaged(rec, words, 1, 1, N.ACCUM_MOMENTS), stride, n, flags),
        "part_index": _colour_host(np.concatenate([rec[words: 2 * words], rec[:words], rec[2 * words:]]), stride, n, flags),
        "part_count": _colour_host(_damaged(rec, words, 2, 3, 4), stride, n, flags),
        "slots": _colour_host(_damaged(rec, words, 2, 5, add=64), stride, n, flags),
        "tiles": _colour_host(_damaged(rec, words, 2, 6, add=1), stride, n, flags),
        "reserved": _colour_host(_damaged(rec, words, 1, 7, AOV.RECORD_MAGIC), stride, n, flags),
        "samples": _colour_host(_damaged(plain_rec, plain_stride // 4, 2, 4, add=1), plain_stride, n, N.ACCUM_MOMENTS),
        "tile_stop is 1": _colour_host(_damaged(rec, words, 2, stop_at + 1, 1), stride, n, flags),
        "tile_stop above samples": _colour_host(_damaged(rec, words, 1, stop_at + 3, SAMPLES + 1), stride, n, flags),
    }
    out["colour"] = colour
    channels = N.AOV_ALBEDO | N.AOV_NORMAL | N.AOV_DEPTH
    a = aov_state(channels)
    parts = a.split(n)
    stride = len(parts[0].packed()) * 4
    words = stride // 4
    rec = np.concatenate([p.packed(stride) for p in parts])
    out["aov"] = {
        "params": _aov_host(rec, stride, 0, channels),
        "stride_bytes": _aov_host(rec, stride - 4, n, channels),
        "stride_bytes not a multiple of 4": _aov_host(rec, stride + 2, n, channels),
        "version": _aov_host(_damaged(rec, words, 1, 0, 9), stride, n, channels),
        "magic": _aov_host(_damaged(rec, words, 1, 7, 0), stride, n, channels),
        "channels": _aov_host(_damaged(rec, words, 0, 1, N.AOV_NORMAL), stride, n, channels),
        "part_index": _aov_host(np.concatenate([rec[words: 2 * words], rec[:words], rec[2 * words:]]), stride, n, channels),
        "part_count": _aov_host(_damaged(rec, words, 2, 3, 4), stride, n, channels),
        "slots": _aov_host(_damaged(rec, words, 2, 5, add=64), stride, n, channels),
        "tiles": _aov_host(_damaged(rec, words, 2, 6, add=1), stride, n, channels),
        "samples": _aov_host(_damaged(rec, words, 2, 4, add=1), stride, n, channels),
    }
    return out


def compute() -> dict:
    return {"digests": digests(), "refusals": refusals()}


def main():
    with open(PATH, "w") as f:
        json.dump(compute(), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
