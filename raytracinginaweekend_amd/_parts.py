"""Partition records in numpy's terms: what progressive.py (colour) and aov.py (first-hit AOVs) share.

A record is 8 header words and an ordered table of sections, each tile-major with a fixed number of words per tile
(include/rtw_parts.h states the same for C and HIP).  Part (r, N) owns the frame's tiles
r, r + N, ...; the records of all N parts have the size of part 0's, which owns the most tiles.  This module is a
restatement, not a binding: it never asks librtw.so for an offset.
"""
from __future__ import annotations

import numpy as np

HEADER_WORDS = 8
VERSION = 1


def part_tiles(n_tiles: int, part: tuple[int, int]) -> np.ndarray:
    """The frame's tiles part (r, N) owns, in the part's own order."""
    return np.arange(part[0], n_tiles, part[1], dtype=np.int64)


def part_slots(n_tiles: int, per_tile: int, part: tuple[int, int]) -> np.ndarray:
    """The whole image's slots part (r, N) owns, in the part's own slot order."""
    return (part_tiles(n_tiles, part)[:, None] * per_tile + np.arange(per_tile, dtype=np.int64)[None, :]).ravel()


def section_offsets(n_tiles: int, part_count: int, per_tile: int, sections) -> dict:
    """`sections`: (name, held, words per tile) in record order.  Returns n_tiles, tiles0, slots0, every section's
    word offset under its name (None: not held) and the record's words."""
    tiles0 = -(-n_tiles // part_count)
    lay = {"n_tiles": n_tiles, "tiles0": tiles0, "slots0": tiles0 * per_tile}
    at = HEADER_WORDS
    for name, held, words in sections:
        lay[name] = at if held else None
        at += words * tiles0 if held else 0
    lay["words"] = at
    return lay


def parts_in_order(states, same: tuple[str, ...]) -> list:
    """The states of parts (0..N-1, N) of one frame, given in any order, by part_index.  Raises ValueError naming
    the field when they differ in one of `same`, and when a part is missing, comes twice or lies outside 0 .. N - 1."""
    states = list(states)
    if not states:
        raise ValueError("merge needs at least one state")
    first = states[0]
    for s in states[1:]:
        for n in same:
            if int(getattr(s, n)) != int(getattr(first, n)):
                raise ValueError(f"the states are not parts of one frame: {n} differs")
    count = max(1, int(first.part_count))
    by_part = {}
    for s in states:
        if int(s.part_index) in by_part:
            raise ValueError(f"part_index {int(s.part_index)} comes twice")
        by_part[int(s.part_index)] = s
    for r in range(count):
        if r not in by_part:
            raise ValueError(f"part_index {r} of part_count {count} is missing")
    if len(by_part) != count:
        raise ValueError(f"part_index outside 0 .. part_count - 1 ({count})")
    return [by_part[r] for r in range(count)]


def pack_record(header: tuple, words: int, stride_bytes: int | None, sections) -> np.ndarray:
    """A record of `words` uint32 words, padded with zeros to `stride_bytes`: the 8 header words, then every
    (word offset, array) of `sections` as bit patterns; a section's words past the array stay zero."""
    total = words if stride_bytes is None else stride_bytes // 4
    if total < words or (stride_bytes or 0) % 4:
        raise ValueError("stride_bytes must be a multiple of 4 and at least the record's bytes")
    rec = np.zeros(total, np.uint32)
    rec[:HEADER_WORDS] = header
    for at, arr in sections:
        flat = np.ascontiguousarray(arr).view(np.uint32).ravel()
        rec[at: at + flat.size] = flat
    return rec
