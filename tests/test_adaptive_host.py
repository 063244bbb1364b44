"""Adaptive sampling, the parts that need no GPU: the checkpoint file with a stop map, the host twin of the
tile test (rtw_adapt_tiles_host, include/rtw_adapt.h) against a numpy restatement, the C declarations, and
the stand-alone program tests/native/adapt_check.c, which runs the same header function on the same cases --
built once plain and once with -fsanitize=address,undefined, and run alone."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.distributed import tile_slots
from raytracinginaweekend_amd.progressive import AccumState
from tests import adaptive_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "adapt_check.c")
FLAGS = ["-std=c11", "-ffp-contract=off", "-fno-fast-math"]
SIZE = R.Size2i(50, 37)
HEADER_FIELDS = [n for n, _ in N.AccumInfo._fields_]
f32 = np.float32


# ---- the checkpoint file --------------------------------------------------------------------------
def _state(tile_stop) -> AccumState:
    rng = np.random.default_rng(5)
    tiles, per_tile = 7, 15
    slots = tiles * per_tile
    sums = rng.integers(0, 2**32, (slots, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    squares = rng.random((slots, 3), dtype=np.float32)
    return AccumState(version=1, flags=3 if tile_stop is not None else 1, width=50, height=30, tile_width=5, tile_height=3,
                      part_index=1, part_count=3, max_depth=9, render_mode=0, samples=4000000000, reserved=0,
                      seed=0xFEDCBA9876543210, world_fingerprint=0x8000000000000001, slots=slots, sums=sums,
                      squares=squares, tile_stop=tile_stop)


def test_checkpoint_with_a_stop_map_round_trips_every_bit(tmp_path):
    stop = np.array([0, 2, 4000000000, 0, 17, 0xFFFFFFFF, 8], np.uint32)
    s = _state(stop)
    assert s.tiles == 7
    path = tmp_path / "adaptive.npz"
    s.save(path)
    t = AccumState.load(path)
    for n in HEADER_FIELDS:
        assert getattr(t, n) == getattr(s, n), n
    assert (t.sums.view(np.uint32) == s.sums.view(np.uint32)).all()
    assert (t.squares.view(np.uint32) == s.squares.view(np.uint32)).all()
    assert t.tile_stop.dtype == np.uint32 and t.tile_stop.shape == (7,) and (t.tile_stop == stop).all()
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(HEADER_FIELDS) | {"sums", "squares", "tile_stop"}


def test_checkpoint_without_a_stop_map_keeps_its_entry_set(tmp_path):
    s = _state(None)
    path = tmp_path / "plain.npz"
    s.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(HEADER_FIELDS) | {"sums", "squares"}
    assert AccumState.load(path).tile_stop is None


@pytest.mark.parametrize("bad", [np.zeros(7, np.int32), np.zeros(7, np.uint64), np.zeros(7, np.float32),
                                 np.zeros(6, np.uint32), np.zeros(8, np.uint32), np.zeros((7, 1), np.uint32)],
                         ids=["int32", "uint64", "float32", "short", "long", "2d"])
def test_checkpoint_refuses_a_bad_stop_map(tmp_path, bad):
    with pytest.raises(ValueError):
        _state(bad).save(tmp_path / "refused.npz")  # save does not write one it would not load
    good = tmp_path / "good.npz"
    _state(np.zeros(7, np.uint32)).save(good)
    with np.load(good, allow_pickle=False) as z:
        arrays = {n: z[n] for n in z.files}
    arrays["tile_stop"] = bad
    np.savez(tmp_path / "bad.npz", **arrays)
    with pytest.raises(ValueError, match="tile_stop"):
        AccumState.load(tmp_path / "bad.npz")


# ---- the tile test on the host ----------------------------------------------------------------------
SHAPES = [((8, 8), (0, 1)), ((5, 3), (0, 1)), ((16, 8), (0, 1)), ((8, 8), (1, 3)), ((5, 3), (1, 3))]


def _case(tile, part, samples=12):
    """Synthetic sums and squares of `samples` samples: per tile a noise level spanning four decades, then the
    special pixels.  Padding slots hold values that would win every maximum if they were read as pixels."""
    rng = np.random.default_rng(tile[0] * 100 + tile[1] * 10 + part[0])
    slots = tile_slots(SIZE, tile, part)
    owned = slots >= 0
    per_tile = tile[0] * tile[1]
    tiles = len(slots) // per_tile
    assert tiles >= 6
    mean = rng.random((len(slots), 3), dtype=np.float32) + f32(0.05)
    sums = (mean * f32(samples)).astype(f32)
    spread = np.repeat(f32(10.0) ** rng.uniform(-4, 0, tiles).astype(f32), per_tile)[:, None]
    squares = (sums * sums / f32(samples) * (f32(1) + spread * rng.random((len(slots), 3), dtype=np.float32))).astype(f32)
    sums[~owned] = f32(1e-3)
    squares[~owned] = f32(1e30)
    first = [int(np.flatnonzero(owned[t * per_tile:(t + 1) * per_tile])[0]) + t * per_tile for t in range(tiles)]
    sums[first[0], 1] = np.nan  # a NaN e beside finite ones: left out
    squares[first[1], 2] = np.inf  # an infinite e: left out
    t2 = slice(2 * per_tile, 3 * per_tile)  # a tile with no finite pixel: E = 0
    sums[t2][owned[t2]] = np.nan
    squares[first[3]] = f32(0)  # d < 0 clamps to 0: e = 0
    return sums, squares, owned, tiles, per_tile


def _host(sums, squares, tile, part, samples, target, min_samples, stop):
    p = R.render_params(SIZE, 1, 1, tile=tile, part=part)
    out = stop.copy()
    rc = N.lib().rtw_adapt_tiles_host(sums.ctypes.data_as(C.POINTER(C.c_float)), squares.ctypes.data_as(C.POINTER(C.c_float)),
                                      C.byref(p), samples, target, min_samples, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return rc, out


def _targets(E):
    """Targets that split the tiles, one of them exactly a tile's E (<= stops it, the next tile up stays)."""
    finite = np.sort(np.unique(E[E > 0]))
    return [float(finite[len(finite) // 2]), float(finite[0]) * 0.5, 0.0, 1e30, float("nan")]


@pytest.mark.parametrize("tile,part", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_host_twin_against_numpy(tile, part):
    samples = 12
    sums, squares, owned, tiles, per_tile = _case(tile, part, samples)
    E = A.tiles_E(sums, squares, samples, SIZE, tile, part)
    assert E.shape == (tiles,) and E[2] == 0 and np.isfinite(E).all() and len(np.unique(E)) > tiles // 2
    before = np.zeros(tiles, np.uint32)
    before[4] = 5  # already stopped: left alone, whatever its E
    for target in _targets(E):
        want = A.stop_rule(before, E, samples, target, 8)
        rc, got = _host(sums, squares, tile, part, samples, target, 8, before)
        assert rc == N.RTW_OK
        assert (got == want).all(), (target, got, want)
        assert got[4] == 5
        if target == target and 0 < target < 1e30:
            assert (got == samples).any() and (got == 0).any()  # the target splits the tiles
            exact = np.flatnonzero(E == f32(target))
            if len(exact):
                assert (got[exact[exact != 4]] == samples).all()  # E == target stops
        # samples < min_samples: nothing stops
        rc, got = _host(sums, squares, tile, part, samples, target, 13, before)
        assert rc == N.RTW_OK and (got == before).all()
    rc, got = _host(sums, squares, tile, part, samples, 1e30, 8, before)
    assert (got[np.arange(tiles) != 4] == samples).all()  # the tile with no finite pixel too (E = 0)
    assert _host(sums, squares, tile, part, 1, 1.0, 8, before)[0] == N.RTW_ERR_INVALID_ARGUMENT
    assert _host(sums, squares, tile, part, samples, 1.0, 1, before)[0] == N.RTW_ERR_INVALID_ARGUMENT


def test_header_compiles_as_c11():
    src = ('#include "rtw.h"\n#include "rtw_adapt.h"\n'
           '_Static_assert(RTW_ACCUM_ADAPTIVE == 2, "RTW_ACCUM_ADAPTIVE");\n'
           '_Static_assert(RTW_ACCUM_MOMENTS == 1, "RTW_ACCUM_MOMENTS");\n'
           "int main(void){rtw_accum* a = 0; uint32_t s = 0; int64_t n = 0;\n"
           "return rtw_accum_adapt(a, 0.5f, 2u, 0, &n, &n) + rtw_accum_tile_stops(a, &s) + rtw_accum_resolve_samples(a, &s, 0)\n"
           "+ rtw_accum_export_adaptive(a, 0, 0, &s) + rtw_accum_import_adaptive(a, 0, 0, 0, &s)\n"
           "+ rtw_adapt_tiles_host(0, 0, 0, 2u, 0.5f, 2u, &s) + (int)rtw_adapt_stop(0.0f, 2u, 0.5f, 2u);}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)
    assert N.ACCUM_ADAPTIVE == 2


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("adapt")
    plain, san = str(d / "adapt_check"), str(d / "adapt_check_san")
    subprocess.run(["gcc", "-O2", *FLAGS, "-o", plain, SRC, "-lm"], check=True)
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *FLAGS, "-o", san,
                    SRC, "-lm"], check=True)
    return plain, san


def _run_program(exe, path, tile, part, samples, min_samples, target, sums, squares, stop):
    with open(path, "wb") as f:
        f.write(struct.pack("<6i2Ifi", SIZE.width, SIZE.height, *tile, *part, samples, min_samples, target, len(stop)))
        f.write(sums.tobytes())
        f.write(squares.tobytes())
        f.write(stop.tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    lines = out.stdout.split("\n")
    assert lines[0] == f"rc 0 tiles {len(stop)}", lines[0]
    return np.array([int(x) for x in lines[1:] if x], np.uint32)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_program_on_the_same_cases(programs, tmp_path, sanitized):
    exe = programs[1 if sanitized else 0]
    for tile, part in SHAPES:
        sums, squares, owned, tiles, per_tile = _case(tile, part)
        E = A.tiles_E(sums, squares, 12, SIZE, tile, part)
        before = np.zeros(tiles, np.uint32)
        before[4] = 5
        for target in _targets(E):
            for min_samples in (8, 13):
                want = A.stop_rule(before, E, 12, target, min_samples)
                got = _run_program(exe, str(tmp_path / "case.bin"), tile, part, 12, min_samples, target, sums, squares, before)
                assert (got == want).all(), (tile, part, target, min_samples)
