"""Partition records on the host (include/rtw_parts.h, progressive.py, distributed.py).

Merging the accumulators of parts (0..N-1, N) is a placement of tile blocks, so everything is checked bit for bit
on synthetic states that hold what a value-level copy would damage: random u32 patterns as sums and squares (NaN
payloads, -0), kept counts, a stop map with active tiles and three distinct stops, zeros in padding slots.  The
numpy pair `AccumState.merge` / `split`, numpy-packed records through the host twin `rtw_accum_merge_parts_host`,
a gloo gather of such records onto rank 0, and the stand-alone program tests/native/parts_check.c (the shared
header alone, built plain and with -fsanitize=address,undefined, run alone) must all reproduce the unsplit state."""
import os
import socket
import struct
import subprocess

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.distributed import tile_slots
from raytracinginaweekend_amd.progressive import AccumState, merge_parts_host, record_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((37, 21), (8, 8)), ((37, 21), (5, 3)), ((20, 12), (8, 8)), ((20, 12), (5, 3))]
PARTS = (1, 2, 3, 4, 8)
ALL_FLAGS = N.ACCUM_MOMENTS | N.ACCUM_ADAPTIVE | N.ACCUM_FINITE
SAMPLES = 24


def synthetic(size, tile, flags=ALL_FLAGS, seed=1):
    """A whole-image state no renderer made: every bit of it must survive."""
    rng = np.random.default_rng(seed)
    sz = R.Size2i(*size)
    slots = tile_slots(sz, tile, (0, 1))
    owned = slots >= 0
    per_tile = tile[0] * tile[1]
    tiles = len(slots) // per_tile

    def bits():
        a = rng.integers(0, 2 ** 32, size=(len(slots), 3), dtype=np.uint64).astype(np.uint32)
        a[:4, 0] = (0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000)  # NaNs with payloads, -0, +inf
        a[~owned] = 0
        return a.view(np.float32)

    stop = None
    if flags & N.ACCUM_ADAPTIVE:
        stop = rng.choice(np.array([0, 0, 8, 12, 20], np.uint32), size=tiles)
        stop[:5] = (0, 8, 12, 20, 0)
    kept = None
    if flags & N.ACCUM_FINITE:
        n = np.full(len(slots), SAMPLES, np.uint32) if stop is None else np.repeat(np.where(stop != 0, stop, SAMPLES), per_tile)
        kept = rng.integers(0, n.astype(np.int64) + 1).astype(np.uint32)
        kept[~owned] = 0
    return AccumState(version=1, flags=flags, width=size[0], height=size[1], tile_width=tile[0], tile_height=tile[1],
                      part_index=0, part_count=1, max_depth=50, render_mode=0, samples=SAMPLES, reserved=0, seed=77,
                      world_fingerprint=0x1234_5678_9ABC_DEF0, slots=len(slots), sums=bits(),
                      squares=bits() if flags & N.ACCUM_MOMENTS else None, tile_stop=stop, kept=kept)


def same(a: AccumState, b: AccumState) -> None:
    assert a.header() == b.header()
    for name in ("sums", "squares", "tile_stop", "kept"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, name
            assert (x.view(np.uint32) == y.view(np.uint32)).all(), name


def gather_numpy(parts, stride_bytes):
    return np.concatenate([p.packed(stride_bytes) for p in parts])


@pytest.mark.parametrize("size,tile", SHAPES)
@pytest.mark.parametrize("flags", [0, N.ACCUM_MOMENTS, N.ACCUM_FINITE, ALL_FLAGS])
def test_merge_of_split_is_the_state(size, tile, flags):
    s = synthetic(size, tile, flags)
    sz = R.Size2i(*size)
    whole_slots = tile_slots(sz, tile, (0, 1))
    image = np.zeros((sz.count(), 3), np.uint32)  # the state as an image, through the frame path's arithmetic
    image[whole_slots[whole_slots >= 0]] = s.sums.view(np.uint32)[whole_slots >= 0]
    for n in PARTS:
        parts = s.split(n)
        assert [(p.part_index, p.part_count) for p in parts] == [(r, n) for r in range(n)]
        same(AccumState.merge(parts), s)
        same(AccumState.merge(parts[::-1]), s)  # in any order
        for r, p in enumerate(parts):
            slots = tile_slots(sz, tile, (r, n))
            assert p.slots == len(slots) and p.sums.shape == (len(slots), 3)
            got = p.sums.view(np.uint32)
            assert (got[slots >= 0] == image[slots[slots >= 0]]).all()
            assert (got[slots < 0] == 0).all()
            if p.kept is not None:
                assert (p.kept[slots < 0] == 0).all()


@pytest.mark.parametrize("size,tile", SHAPES)
def test_split_samples_follow_the_frontier_rule(size, tile):
    s = synthetic(size, tile)
    for n in PARTS:
        for p in s.split(n):
            if (p.tile_stop == 0).any():
                assert p.samples == SAMPLES
            else:
                assert p.samples == (int(p.tile_stop.max()) if p.tile_stop.size else 0) < SAMPLES
            assert (p.tile_stop <= p.samples).all()
    # every tile stopped: the frontier is the largest stop, on the whole and on every part with tiles
    s.tile_stop = np.where(s.tile_stop == 0, np.uint32(20), s.tile_stop).astype(np.uint32)
    s.kept = np.minimum(s.kept, np.repeat(s.tile_stop, tile[0] * tile[1])).astype(np.uint32)
    s.samples = 20
    for n in PARTS:
        same(AccumState.merge(s.split(n)), s)


@pytest.mark.parametrize("size,tile", SHAPES)
@pytest.mark.parametrize("flags", [0, N.ACCUM_MOMENTS | N.ACCUM_FINITE, ALL_FLAGS])
def test_host_twin_merges_numpy_records(size, tile, flags):
    s = synthetic(size, tile, flags, seed=2)
    p = R.render_params(R.Size2i(*size), 0, 50, tile=tile)
    for n in PARTS:
        parts = s.split(n)
        lay = record_layout(size[0], size[1], tile, flags, n)
        assert N.packed_bytes(p, flags, n) == lay["words"] * 4
        assert lay["slots0"] == parts[0].slots and all(len(q.packed()) == lay["words"] for q in parts)
        for stride in (lay["words"] * 4, lay["words"] * 4 + 20):  # a padded stride too
            same(merge_parts_host(parts[-1], gather_numpy(parts, stride), stride, n), s)


def test_more_parts_than_tiles():
    size, tile = (20, 12), (8, 8)  # 3 x 2 tiles
    s = synthetic(size, tile)
    for n in (6, 7, 11):
        parts = s.split(n)
        assert [p.slots for p in parts] == [64] * 6 + [0] * (n - 6)
        assert all(p.samples == 0 and p.tile_stop.size == 0 for p in parts[6:])
        same(AccumState.merge(parts), s)
        stride = len(parts[0].packed()) * 4
        same(merge_parts_host(s, gather_numpy(parts, stride), stride, n), s)
    plain = synthetic(size, tile, N.ACCUM_MOMENTS)
    parts = plain.split(9)
    assert all(p.samples == SAMPLES for p in parts)  # not adaptive: every part counts alike
    same(AccumState.merge(parts), plain)


def _refused(field, call, exc):
    with pytest.raises(exc) as e:
        call()
    assert field in str(e.value), str(e.value)


def test_refusals_name_the_field():
    size, tile, n = (37, 21), (8, 8), 3
    s = synthetic(size, tile)
    plain = synthetic(size, tile, N.ACCUM_MOMENTS)

    def both(field, damage, state=s):
        """`damage` edits the parts; numpy's merge and the host twin both refuse them by `field`."""
        parts = state.split(n)
        damage(parts)
        _refused(field, lambda: AccumState.merge(parts), ValueError)
        stride = len(state.split(n)[0].packed()) * 4
        try:
            gathered = gather_numpy(parts, stride)
        except ValueError:
            return  # (a state whose arrays contradict its flags has no record)
        _refused(field, lambda: merge_parts_host(state, gathered, stride, n), N.RtwError)

    def wrong_flags(parts):
        q = plain.split(n)[1]
        q.sums, q.squares = parts[1].sums, parts[1].squares
        parts[1] = q

    both("flags", wrong_flags)

    def duplicate(parts):
        parts[2] = parts[1]

    both("part_index", duplicate)
    _refused("part_index", lambda: AccumState.merge(s.split(n)[:2]), ValueError)  # a missing part
    stride = len(s.split(n)[0].packed()) * 4
    stride2 = record_layout(size[0], size[1], tile, ALL_FLAGS, 2)["words"] * 4
    two = gather_numpy(s.split(n)[:2], stride2)
    _refused("part_count", lambda: merge_parts_host(s, two, stride2, 2), N.RtwError)  # the host twin sees 2 of 3

    def unequal(parts):
        parts[1].samples -= 1

    both("samples", unequal, plain)

    def stop_one(parts):
        parts[2].tile_stop[1] = 1

    both("tile_stop", stop_one)

    def stop_above(parts):
        parts[0].tile_stop[:] = 20  # its frontier stays 24 ...
        parts[0].samples = 16  # ... until the part says it holds fewer samples than its stops

    both("tile_stop", stop_above)
    for field in ("width", "tile_height", "max_depth", "render_mode", "seed", "world_fingerprint"):
        def other_frame(parts, field=field):
            setattr(parts[1], field, getattr(parts[1], field) + 1)

        parts = s.split(n)
        other_frame(parts)
        _refused(field, lambda: AccumState.merge(parts), ValueError)
    rec = gather_numpy(s.split(n), stride)
    _refused("stride_bytes", lambda: merge_parts_host(s, rec, stride - 4, n), N.RtwError)
    bad = rec.copy()
    bad[stride // 4] = 9  # record 1's version
    _refused("version", lambda: merge_parts_host(s, bad, stride, n), N.RtwError)
    bad = rec.copy()
    bad[2 * (stride // 4) + 5] += 64  # record 2's slots
    _refused("slots", lambda: merge_parts_host(s, bad, stride, n), N.RtwError)
    _refused("part_index", lambda: s.split(2)[1].split(2), ValueError)  # split takes the whole image's state only


def test_split_and_merge_repartition_a_checkpoint(tmp_path):
    """N = 3 ranks' files -> one whole -> M = 2 ranks' states, through save / load."""
    s = synthetic((37, 21), (5, 3))
    for r, p in enumerate(s.split(3)):
        p.save(tmp_path / f"rank{r}.npz")
    merged = AccumState.merge(AccumState.load(tmp_path / f"rank{r}.npz") for r in range(3))
    same(merged, s)
    two = merged.split(2)
    same(AccumState.merge(two), s)
    assert [p.part_count for p in two] == [2, 2] and sum(p.slots for p in two) == s.slots


# ---- the stand-alone program: the shared header alone, plain and under the sanitizers -----------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "parts_check.c")
    d = tmp_path_factory.mktemp("parts")
    plain, san = str(d / "parts_check"), str(d / "parts_check_san")
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-o", plain, src, "-lm"],
                   check=True)
    subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src,
                    "-lm"], check=True)
    return plain, san


def fnv(a) -> int:
    h = 0xCBF29CE484222325
    if a is None:
        return 0
    for b in np.ascontiguousarray(a).view(np.uint32).astype("<u4").tobytes():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_program_on_the_same_cases(programs, tmp_path, sanitized):
    exe = programs[1 if sanitized else 0]

    def run(size, tile, flags, n, stride, gathered):
        path = str(tmp_path / "case.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<5iIQ", *size, *tile, n, flags, stride // 4))
            f.write(np.ascontiguousarray(gathered, np.uint32).tobytes())
        out = subprocess.run([exe, "colour", path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (size, tile, flags, n, out.stdout[-2000:], out.stderr[-2000:])
        return out.stdout.split("\n")

    for size, tile in SHAPES:
        for flags in (0, ALL_FLAGS):
            s = synthetic(size, tile, flags, seed=3)
            want = "fnv " + " ".join(f"{fnv(a):016x}" for a in (s.sums, s.squares, s.kept, s.tile_stop))
            for n in (1, 3, 8, 40):  # (40: more parts than the 15 or 6 tiles of the 8 x 8 shapes)
                parts = s.split(n)
                stride = len(parts[0].packed()) * 4  # the exact record: a word read past it is out of bounds
                lines = run(size, tile, flags, n, stride, gather_numpy(parts, stride))
                assert lines[0] == f"rc 0 samples {SAMPLES}", lines[0]
                assert lines[1] == want, (size, tile, flags, n)
    size, tile = SHAPES[0]
    parts = synthetic(size, tile).split(3)
    parts[2].tile_stop[1] = 1
    stride = len(parts[0].packed()) * 4
    assert run(size, tile, ALL_FLAGS, 3, stride, gather_numpy(parts, stride))[0]== "rc -1 field tile_stop at 2 1"
    assert run(size, tile, ALL_FLAGS, 2, stride, gather_numpy(parts[:2], stride))[0].startswith("rc -1 field stride_bytes at ")


# ---- the wrapper's gather step over gloo ------------------------------------------------------------------
def _free_port() -> int:
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def _worker(rank, world_size, port, out_path, size, tile):
    import sys

    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    from raytracinginaweekend_amd.distributed import gather_records

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world_size)
    try:
        s = synthetic(size, tile)  # (every rank derives the same state and keeps its own part of it)
        mine = s.split(world_size)[rank]
        stride = -(-len(mine.packed()) * 4 // 16) * 16  # the wrapper's stride: whole 16 bytes
        record = torch.from_numpy(mine.packed(stride).view(np.int32))
        gathered = torch.zeros(world_size * stride // 4, dtype=torch.int32) if rank == 0 else None
        gather_records(record, gathered, rank, world_size)
        if rank == 0:
            merge_parts_host(mine, gathered.numpy(), stride, world_size).save(out_path)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world_size,size,tile", [(2, (37, 21), (8, 8)), (3, (20, 12), (5, 3))])
def test_gloo_record_gather_reassembles_the_state(tmp_path, world_size, size, tile):
    import torch.multiprocessing as mp

    out = str(tmp_path / "whole.npz")
    mp.start_processes(_worker, args=(world_size, _free_port(), out, size, tile), nprocs=world_size, start_method="spawn",
                       join=True)
    same(AccumState.load(out), synthetic(size, tile))
