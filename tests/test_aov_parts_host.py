"""AOV partition records on the host (include/rtw_aov_parts.h, aov.py, distributed.py).

Merging the AOV accumulators of parts (0..N-1, N) is a placement of 64-slot tile blocks in every plane, so
everything is checked bit for bit on synthetic states that hold what a value-level copy would damage: random u32
patterns as planes (NaN payloads, -0), hit counts up to the sample count, zeros in padding slots.  The numpy pair
`AovState.merge` / `split`, numpy-packed records through the host twin `rtw_aov_merge_parts_host`, a gloo gather of
such records onto rank 0, and the stand-alone program tests/native/parts_check.c (the shared headers alone,
built plain and with -fsanitize=address,undefined, run alone) must all reproduce the unsplit state.  37 x 19 has
15 tiles with edge tiles on both axes, 16 x 8 has 2; with 16 parts at least one part holds no tiles."""
import ctypes as C
import itertools
import os
import socket
import struct
import subprocess

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd import aov as AOV
from raytracinginaweekend_amd.aov import AovState, merge_parts_host, record_layout
from raytracinginaweekend_amd.distributed import tile_slots
from raytracinginaweekend_amd.progressive import AccumState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(37, 19), (16, 8)]
PARTS = (1, 2, 3, 4, 16)
NAMES = ("albedo", "normal", "depth")
BITS = {"albedo": N.AOV_ALBEDO, "normal": N.AOV_NORMAL, "depth": N.AOV_DEPTH}
SUBSETS = [c for k in (1, 2, 3) for c in itertools.combinations(NAMES, k)]
ALL = N.AOV_ALBEDO | N.AOV_NORMAL | N.AOV_DEPTH
SAMPLES = 24


def bits_of(names) -> int:
    return sum(BITS[n] for n in names)


def synthetic(size, channels=ALL, seed=1):
    """A whole-image AOV state no renderer made: every bit of it must survive."""
    rng = np.random.default_rng(seed)
    owned = tile_slots(R.Size2i(*size), (8, 8), (0, 1)) >= 0
    slots = owned.size

    def plane(k):
        a = rng.integers(0, 2 ** 32, size=(k, slots), dtype=np.uint64).astype(np.uint32)
        a[0, :4] = (0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000)  # NaNs with payloads, -0, +inf
        a[:, ~owned] = 0
        return a.view(np.float32)

    hits = rng.integers(0, SAMPLES + 1, size=slots).astype(np.uint32)
    hits[~owned] = 0
    return AovState(version=1, channels=channels, width=size[0], height=size[1], samples=SAMPLES, part_index=0, part_count=1,
                    slots=slots, tiles=slots // 64, reserved=0, seed=77, world_fingerprint=0x1234_5678_9ABC_DEF0, hits=hits,
                    albedo=plane(3) if channels & N.AOV_ALBEDO else None, normal=plane(3) if channels & N.AOV_NORMAL else None,
                    depth=plane(1)[0] if channels & N.AOV_DEPTH else None)


def same(a: AovState, b: AovState) -> None:
    assert a.header() == b.header()
    for name in ("albedo", "normal", "depth", "hits"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, name
            assert (x.view(np.uint32) == y.view(np.uint32)).all(), name


def gather_numpy(parts, stride_bytes):
    return np.concatenate([p.packed(stride_bytes) for p in parts])


@pytest.mark.parametrize("size", SHAPES)
@pytest.mark.parametrize("names", SUBSETS, ids="+".join)
def test_merge_of_split_is_the_state(size, names):
    s = synthetic(size, bits_of(names))
    sz = R.Size2i(*size)
    n_tiles = AOV.frame_tiles(*size)
    for n in PARTS:
        parts = s.split(n)
        assert [(p.part_index, p.part_count) for p in parts] == [(r, n) for r in range(n)]
        assert [p.tiles for p in parts] == [len(range(r, n_tiles, n)) for r in range(n)]
        assert all(p.samples == SAMPLES for p in parts)
        if n == 16:
            assert parts[-1].tiles == 0 and parts[-1].hits.size == 0  # more parts than tiles
        same(AovState.merge(parts), s)
        same(AovState.merge(parts[::-1]), s)  # in any order
        for r, p in enumerate(parts):  # a part's slots against the frame path's arithmetic
            slots = tile_slots(sz, (8, 8), (r, n))
            whole = tile_slots(sz, (8, 8), (0, 1))
            assert p.slots == len(slots) == p.tiles * 64
            at = {int(pix): i for i, pix in enumerate(whole) if pix >= 0}
            src = np.array([at[int(pix)] for pix in slots[slots >= 0]], np.int64)
            assert (p.hits[slots >= 0] == s.hits[src]).all() and (p.hits[slots < 0] == 0).all()
            for name in names:
                got, want = getattr(p, name).view(np.uint32), getattr(s, name).view(np.uint32)
                assert (got[..., slots >= 0] == want[..., src]).all() and (got[..., slots < 0] == 0).all()


@pytest.mark.parametrize("size", SHAPES)
@pytest.mark.parametrize("names", SUBSETS, ids="+".join)
def test_host_twin_merges_numpy_records(size, names):
    channels = bits_of(names)
    s = synthetic(size, channels, seed=2)
    for n in PARTS:
        parts = s.split(n)
        lay = record_layout(size[0], size[1], channels, n)
        assert AOV.aov_packed_bytes(R.Size2i(*size), channels, n) == lay["words"] * 4
        assert lay["slots0"] == parts[0].slots and all(len(q.packed()) == lay["words"] for q in parts)
        assert lay["words"] == 8 + lay["planes"] * lay["slots0"]
        for stride in (lay["words"] * 4, lay["words"] * 4 + 20):  # an odd stride with padding between the records
            same(merge_parts_host(parts[-1], gather_numpy(parts, stride), stride, n), s)
    rec = s.split(3)[1].packed()
    assert tuple(rec[:8]) == (1, channels, 1, 3, SAMPLES, s.split(3)[1].slots, s.split(3)[1].tiles, AOV.RECORD_MAGIC)


def _refused(field, call, exc=N.RtwError):
    with pytest.raises(exc) as e:
        call()
    assert field in str(e.value), str(e.value)


def test_refusals_name_the_field_and_write_nothing():
    size, n = (37, 19), 3
    s = synthetic(size)
    parts = s.split(n)
    stride = len(parts[0].packed()) * 4
    rec = gather_numpy(parts, stride)
    words = stride // 4
    lib = N.lib()
    p = R.render_params(R.Size2i(*size), 0, 0)

    def host(gathered, stride_bytes, count, channels=ALL):
        """The C entry point on arrays filled with a pattern: refused, and the pattern is still there."""
        out = {k: np.full((3, s.slots) if k in ("albedo", "normal") else s.slots, 0xABABABAB, np.uint32)
               for k in ("albedo", "normal", "depth", "hits") if k == "hits" or channels & BITS[k]}
        samples = C.c_uint32(0xABABABAB)
        g = np.ascontiguousarray(gathered, np.uint32)

        def ptr(k, t):
            return out[k].ctypes.data_as(C.POINTER(t)) if k in out else None

        rc = lib.rtw_aov_merge_parts_host(C.byref(p), channels, C.c_void_p(g.ctypes.data), stride_bytes, count,
                                          ptr("albedo", C.c_float), ptr("normal", C.c_float), ptr("depth", C.c_float),
                                          ptr("hits", C.c_uint32), C.byref(samples))
        assert rc == N.RTW_ERR_INVALID_ARGUMENT
        assert samples.value == 0xABABABAB and all((a == 0xABABABAB).all() for a in out.values())
        return (lib.rtw_last_error() or b"").decode()

    assert "stride_bytes" in host(rec, stride - 4, n)  # a stride below the record's size
    bad = rec.copy()
    bad[words] = 9  # record 1's version
    assert "version" in host(bad, stride, n)
    # a colour record given to the AOV merge: it holds 0 where an AOV record holds its magic
    colour = AccumState(version=1, flags=0, width=size[0], height=size[1], tile_width=8, tile_height=8, part_index=0,
                        part_count=1, max_depth=50, render_mode=0, samples=SAMPLES, reserved=0, seed=77, world_fingerprint=1,
                        slots=s.slots, sums=np.zeros((s.slots, 3), np.float32))
    colour_rec = np.concatenate([q.packed(stride) for q in colour.split(n)])
    assert colour_rec[0] == 1 and colour_rec[7] == 0
    assert "magic" in host(colour_rec, stride, n)
    swapped = np.concatenate([rec[words: 2 * words], rec[:words], rec[2 * words:]])
    assert "part_index" in host(swapped, stride, n)
    stride2 = record_layout(size[0], size[1], ALL, 2)["words"] * 4
    assert "part_count" in host(gather_numpy(parts[:2], stride2), stride2, 2)  # two of three parts
    bad = rec.copy()
    bad[words + 4] += 1  # record 1's samples
    assert "samples" in host(bad, stride, n)
    assert "channels" in host(rec, stride, n, channels=N.AOV_ALBEDO | N.AOV_DEPTH)  # channels that differ from whole's
    bad = rec.copy()
    bad[2 * words + 5] += 64
    assert "slots" in host(bad, stride, n)
    bad = rec.copy()
    bad[2 * words + 6] += 1
    assert "tiles" in host(bad, stride, n)
    # the same through the wrapper, and numpy's merge by the same names
    _refused("stride_bytes", lambda: merge_parts_host(s, rec, stride - 4, n))
    _refused("magic", lambda: merge_parts_host(s, colour_rec, stride, n))
    _refused("part_index", lambda: AovState.merge(parts[:2]), ValueError)
    _refused("part_index", lambda: AovState.merge([parts[0], parts[1], parts[1]]), ValueError)
    for field in ("channels", "width", "seed", "world_fingerprint", "samples"):
        other = s.split(n)
        setattr(other[1], field, getattr(other[1], field) + (2 if field == "channels" else 1))
        _refused(field, lambda: AovState.merge(other), ValueError)
    _refused("part_index", lambda: parts[1].split(2), ValueError)  # split takes the whole image's state only
    # the AOV record in turn is refused by the colour merge
    from raytracinginaweekend_amd.progressive import merge_parts_host as colour_merge

    # (one whose channels word reads as the colour accumulator's flags, so that the check reaches the last word)
    colour.flags, colour.squares = N.ACCUM_MOMENTS, np.zeros((s.slots, 3), np.float32)
    wide = len(colour.split(n)[0].packed()) * 4
    albedo_rec = gather_numpy(synthetic(size, N.AOV_ALBEDO).split(n), wide)
    _refused("reserved", lambda: colour_merge(colour, albedo_rec, wide, n))
    _refused("flags", lambda: colour_merge(colour, rec, stride, n))  # (any other: its channels are not the flags)


def _create_part(channels=ALL, **kw):
    p = R.render_params(R.Size2i(37, 19), 0, 0, seed=1)
    for k, v in kw.items():
        setattr(p, k, v)
    h = C.c_void_p(0xDEAD)
    rc = N.lib().rtw_aov_create_part(None, C.byref(p), channels, C.byref(h))
    return rc, (N.lib().rtw_last_error() or b"").decode(), h


def test_create_part_refusals():
    # rtw_aov_create_part checks the params before the world: refused without a device, nothing allocated
    for field, code, kw in (("tile_width", N.RTW_ERR_UNSUPPORTED, dict(tile_width=5, tile_height=3)),
                            ("tile_height", N.RTW_ERR_UNSUPPORTED, dict(tile_width=8, tile_height=3)),
                            ("thread_count", N.RTW_ERR_UNSUPPORTED, dict(thread_count=2)),
                            ("part_index", N.RTW_ERR_INVALID_ARGUMENT, dict(part_index=3, part_count=3)),
                            ("part_index", N.RTW_ERR_INVALID_ARGUMENT, dict(part_index=-1, part_count=3)),
                            ("layout", N.RTW_ERR_INVALID_ARGUMENT, dict(layout=7)),
                            ("reserved0", N.RTW_ERR_INVALID_ARGUMENT, dict(reserved0=1))):
        rc, msg, h = _create_part(**kw)
        assert rc == code and field in msg and not h.value, (field, rc, msg)
    for channels in (0, 8):
        rc, msg, h = _create_part(channels)
        assert rc == N.RTW_ERR_INVALID_ARGUMENT and "channels" in msg and not h.value
    # valid part params reach the world
    for kw in (dict(part_index=2, part_count=3, layout=N.LAYOUT_TILES), dict(part_index=0, part_count=1),
               dict(part_index=15, part_count=16, tile_width=0, tile_height=0), dict(part_index=1, part_count=2, tile_width=8)):
        rc, msg, h = _create_part(**kw)
        assert rc == N.RTW_ERR_INVALID_ARGUMENT and "null world" in msg and not h.value, (kw, msg)
    # and rtw_aov_create still refuses what it refused
    p = R.render_params(R.Size2i(37, 19), 0, 0, seed=1, part=(1, 2))
    h = C.c_void_p()
    assert N.lib().rtw_aov_create(None, C.byref(p), ALL, C.byref(h)) == N.RTW_ERR_UNSUPPORTED
    assert b"part_count" in N.lib().rtw_last_error()


def test_state_checkpoint_roundtrip_and_repartition(tmp_path):
    """N = 3 ranks' files -> one whole -> M = 2 ranks' states, through save / load."""
    s = synthetic((37, 19), N.AOV_ALBEDO | N.AOV_DEPTH)
    for r, p in enumerate(s.split(3)):
        p.save(tmp_path / f"rank{r}.npz")
    merged = AovState.merge(AovState.load(tmp_path / f"rank{r}.npz") for r in range(3))
    same(merged, s)
    two = merged.split(2)
    same(AovState.merge(two), s)
    assert [p.part_count for p in two] == [2, 2] and sum(p.slots for p in two) == s.slots
    np.savez(tmp_path / "odd.npz", **{**{k: np.asarray(v) for k, v in s.header().items()}, "hits": s.hits})
    with pytest.raises(ValueError, match="header field"):
        AovState.load(tmp_path / "odd.npz")  # (plain ints: not the dtypes save writes)


def test_header_compiles_as_c99():
    src = ('#include "rtw_aov_parts.h"\n'
           "int main(void){rtw_aov* a = 0; rtw_aov_state_info i; rtw_render_params p = {0}; rtw_parts_layout L; int64_t b;\n"
           "uint32_t n; const char* f; int32_t at[2]; uint32_t* dst[RTW_PARTS_MAX_SECTIONS] = {0};\n"
           "return rtw_aov_create_part(0, &p, RTW_AOV_ALBEDO, &a) + rtw_aov_packed_bytes(&p, 7u, 2, &b) + rtw_aov_pack(a, 0, 0)\n"
           "+ rtw_aov_merge_parts(a, 0, 0, 1, 0) + rtw_aov_merge_parts_host(&p, 7u, 0, 0, 1, 0, 0, 0, 0, &n)\n"
           "+ rtw_aov_get_state_info(a, &i) + rtw_aov_export_state(a, 0, 0, 0, 0) + rtw_aov_import_state(a, &i, 0, 0, 0, 0)\n"
           "+ rtw_aov_parts_layout_of(&p, 7u, 2, &L) + rtw_parts_merge(&L, 0, 0, dst, &n, &f, at)\n"
           "+ (int)sizeof(rtw_aov_state_info);}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)
    assert C.sizeof(N.AovStateInfo) == 56  # fixed-width fields, no padding


# ---- the stand-alone program: the shared header alone, plain and under the sanitizers -----------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "parts_check.c")
    d = tmp_path_factory.mktemp("aov_parts")
    plain, san = str(d / "aov_parts_check"), str(d / "aov_parts_check_san")
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

    def run(size, channels, n, stride, gathered):
        path = str(tmp_path / "case.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<3iIQ", *size, n, channels, stride // 4))
            f.write(np.ascontiguousarray(gathered, np.uint32).tobytes())
        out = subprocess.run([exe, "aov", path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (size, channels, n, out.stdout[-2000:], out.stderr[-2000:])
        return out.stdout.split("\n")

    for size in SHAPES:
        for channels in (ALL, N.AOV_NORMAL, N.AOV_ALBEDO | N.AOV_DEPTH):
            s = synthetic(size, channels, seed=3)
            want = "fnv " + " ".join(f"{fnv(a):016x}" for a in (s.albedo, s.normal, s.depth, s.hits))
            for n in PARTS:
                parts = s.split(n)
                stride = len(parts[0].packed()) * 4  # the exact record: a word read past it is out of bounds
                lines = run(size, channels, n, stride, gather_numpy(parts, stride))
                assert lines[0] == f"rc 0 samples {SAMPLES}", lines[0]
                assert lines[1] == want, (size, channels, n)
    size = SHAPES[0]
    parts = synthetic(size).split(3)
    stride = len(parts[0].packed()) * 4
    parts[2].samples -= 1
    assert run(size, ALL, 3, stride, gather_numpy(parts, stride))[0] == "rc -1 field samples at 2"
    assert run(size, ALL, 2, stride, gather_numpy(parts[:2], stride))[0] == "rc -1 field stride_bytes at 0"
    assert run(size, N.AOV_NORMAL, 3, stride, gather_numpy(parts, stride))[0] == "rc -1 field channels at 0"


# ---- the wrapper's gather step over gloo ------------------------------------------------------------------
def _free_port() -> int:
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def _worker(rank, world_size, port, out_path, size):
    import sys

    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    from raytracinginaweekend_amd.distributed import gather_records

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world_size)
    try:
        s = synthetic(size)  # (every rank derives the same state and keeps its own part of it)
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


@pytest.mark.parametrize("world_size,size", [(2, (37, 19)), (3, (16, 8))])
def test_gloo_record_gather_reassembles_the_state(tmp_path, world_size, size):
    import torch.multiprocessing as mp

    out = str(tmp_path / "whole.npz")
    mp.start_processes(_worker, args=(world_size, _free_port(), out, size), nprocs=world_size, start_method="spawn", join=True)
    same(AovState.load(out), synthetic(size))
