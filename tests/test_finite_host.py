"""Finite-sample accumulation, the parts that need no GPU (include/rtw_finite.h): the oracle's
per-sample colours as the definition, the host twins (rtw_finite_accumulate_host, rtw_adapt_tiles_finite_host)
against a numpy restatement bit for bit, the checkpoint file with kept counts, the C declarations, and the
stand-alone program tests/native/finite_check.c -- built once plain and once with -fsanitize=address,undefined,
and run alone."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.distributed import tile_slots
from raytracinginaweekend_amd.progressive import AccumState
from tests import adaptive_ref as A
from tests import finite_ref as F
from tests.parity import assert_bit_identical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "finite_check.c")
FLAGS = ["-std=c11", "-ffp-contract=off", "-fno-fast-math"]
HEADER_FIELDS = [n for n, _ in N.AccumInfo._fields_]
f32 = np.float32
f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def host_accumulate(colors, sums, squares, kept):
    """rtw_finite_accumulate_host on copies: colors (n, slots, 3)."""
    colors = np.ascontiguousarray(colors, f32)
    sums, kept = sums.copy(), kept.copy()
    squares = None if squares is None else squares.copy()
    rc = N.lib().rtw_finite_accumulate_host(colors.ctypes.data_as(f32p), colors.shape[0], colors.shape[1],
                                            sums.ctypes.data_as(f32p), squares.ctypes.data_as(f32p) if squares is not None else None,
                                            kept.ctypes.data_as(u32p))
    assert rc == N.RTW_OK
    return sums, squares, kept


def host_adapt(sums, squares, kept, size, tile, part, samples, target, min_samples, stop):
    p = R.render_params(size, 1, 1, tile=tile, part=part)
    out = stop.copy()
    rc = N.lib().rtw_adapt_tiles_finite_host(sums.ctypes.data_as(f32p), squares.ctypes.data_as(f32p), kept.ctypes.data_as(u32p),
                                             C.byref(p), samples, target, min_samples, out.ctypes.data_as(u32p))
    return rc, out


# ---- 1. the oracle is the definition ---------------------------------------------------------------------
def test_the_oracle_is_the_definition(worlds):
    world, size, n = worlds("suzanne"), R.Size2i(37, 19), 16
    p = R.render_params(size, n, 10, seed=31)
    colors = F.oracle_samples(world, p, n)
    bad = ~F.finite(colors)
    rejected = bad.sum(axis=0)
    first = np.where(rejected > 0, bad.argmax(axis=0), n)
    print("non-finite samples", int(bad.sum()), "pixels", int((rejected > 0).sum()), "most in a pixel", int(rejected.max()),
          "first below 8", int((first < 8).sum()))
    assert (rejected > 0).sum() >= 10 and (first < 8).sum() >= 4, "the input must exercise the filter on both sides of a split"
    sums, squares, kept = F.accumulate(colors)
    assert (kept == n - rejected).all()
    zero = np.zeros((size.count(), 3), f32)
    got = host_accumulate(colors, zero, zero, np.zeros(size.count(), np.uint32))
    assert_bit_identical(got[0], sums, "sums")
    assert_bit_identical(got[1], squares, "squares")
    assert (got[2] == kept).all()
    assert np.isfinite(got[0]).all()  # no NaN entered a sum
    # split at 8, with rejected samples on both sides, and without moments
    half = host_accumulate(colors[:8], zero, None, np.zeros(size.count(), np.uint32))
    assert half[1] is None
    both = host_accumulate(colors[8:], half[0], None, half[2])
    assert_bit_identical(both[0], sums, "sums of a split add")
    assert (both[2] == kept).all()
    # where nothing was rejected the mean is the reference's pixel
    ref = O.render(world, p)
    clean = rejected == 0
    assert_bit_identical(F.mean(sums, kept)[clean], ref[clean], "the mean on pixels without a rejected sample")
    assert np.isnan(ref[~clean]).any(axis=1).all() and np.isfinite(F.mean(sums, kept)).all()


# ---- 2. synthetic colours: the twins against numpy ---------------------------------------------------------
SHAPES = [((2, 2), (8, 8), (0, 1)), ((7, 5), (4, 4), (0, 1)), ((7, 5), (4, 4), (1, 3)), ((37, 23), (8, 8), (0, 1)),
          ((37, 23), (8, 8), (1, 3))]
SAMPLES, BATCH, MIN = 12, 4, 4


def bits(u):
    return np.array(u, np.uint32).view(f32)


def _case(size, tile, part):
    """12 samples per slot: per tile a noise level spanning three decades, then the special values on the owned
    slots in turn.  Padding slots hold NaN colours (finite_ref.to_slots)."""
    sz = R.Size2i(*size)
    rng = np.random.default_rng(size[0] * 100 + tile[0] * 10 + part[0])
    slots = tile_slots(sz, tile, part)
    owned = slots >= 0
    per_tile = tile[0] * tile[1]
    tiles = len(slots) // per_tile
    base = rng.random((len(slots), 3), dtype=f32) + f32(0.05)
    spread = np.repeat(f32(10.0) ** rng.uniform(-3, 0, tiles).astype(f32), per_tile)[None, :, None]
    colors = (base[None] * (f32(1) + spread * (rng.random((SAMPLES, len(slots), 3), dtype=f32) - f32(0.5)))).astype(f32)
    own = np.flatnonzero(owned)
    assert len(own) >= 4
    nan = bits([0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF])  # quiet, payloads, signalling, negative
    colors[:, own[0]] = nan[np.arange(SAMPLES) % 5][:, None]  # every sample bad: kept = 0
    colors[:, own[1]] = np.nan
    colors[1, own[1]] = (0.25, 0.5, 0.75)  # one sample left, in the first batch (a stopped tile is frozen): kept = 1
    specials = [(np.inf, 1, 1), (1, -np.inf, 1), (1, 1, np.nan), (np.nan, 2, 3), (-0.0, -0.0, -0.0), (1e-40, 3e-45, 0.0),
                (1e30, 1.0, 1e-30), (-1e30, 1e19, 1e20), (3.4e38, 3.4e38, 3.4e38), bits([0x7FC00001, 0x3F800000, 0xFF800000])]
    for i, c in enumerate(specials):  # each on an owned slot of its own, at a sample that moves through the batches
        colors[(3 * i) % SAMPLES, own[(2 + i) % len(own)]] = np.array(c, f32)
    if len(own) > 20:
        colors[:, own[17]] = 0.0
        colors[0, own[17]] = -0.0  # sums of -0 and +0
        colors[2:, own[19]] = np.inf  # two samples left: the smallest kept with a finite e
    colors[:, ~owned] = np.nan
    return sz, colors, slots, owned, tiles, per_tile


def _replay(case, size, tile, part, accumulate, adapt):
    """An adaptive finite accumulator's run in batches of 4: a stopped tile's state is frozen.  The target is the
    median positive tile E of the numpy restatement at the first batch."""
    sz, colors, slots, owned, tiles, per_tile = case
    sums = np.zeros((len(slots), 3), f32)
    squares, kept, stop = sums.copy(), np.zeros(len(slots), np.uint32), np.zeros(tiles, np.uint32)
    first = F.accumulate(colors[:BATCH])
    E0 = F.tiles_E(*first, sz, tile, part)
    target = float(np.median(E0[E0 > 0])) if (E0 > 0).any() else 0.5
    stops = []
    for s0 in range(0, SAMPLES, BATCH):
        new = accumulate(colors[s0:s0 + BATCH], sums, squares, kept)
        frozen = A.expand(stop != 0, per_tile)
        sums = np.where(frozen[:, None], sums, new[0])
        squares = np.where(frozen[:, None], squares, new[1])
        kept = np.where(frozen, kept, new[2])
        stop = adapt(sums, squares, kept, s0 + BATCH, target, stop)
        stops.append(stop)
    return sums, squares, kept, stops, target


@pytest.mark.parametrize("size,tile,part", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_host_twins_against_numpy(size, tile, part):
    case = _case(size, tile, part)
    sz, colors, slots, owned, tiles, per_tile = case

    def np_adapt(sums, squares, kept, n, target, stop):
        return A.stop_rule(stop, F.tiles_E(sums, squares, kept, sz, tile, part), n, target, MIN)

    def c_adapt(sums, squares, kept, n, target, stop):
        rc, out = host_adapt(sums, squares, kept, sz, tile, part, n, target, MIN, stop)
        assert rc == N.RTW_OK
        return out

    want = _replay(case, size, tile, part, F.accumulate, np_adapt)
    got = _replay(case, size, tile, part, host_accumulate, c_adapt)
    assert_bit_identical(got[0], want[0], "sums")
    assert_bit_identical(got[1], want[1], "squares")
    assert (got[2] == want[2]).all()
    for r, (g, w) in enumerate(zip(got[3], want[3])):
        assert (g == w).all(), (r, g, w)
    sums, squares, kept, stops, target = want
    assert (kept[~owned] == 0).all() and (sums.view(np.uint32)[~owned] == 0).all() and (squares.view(np.uint32)[~owned] == 0).all()
    own = np.flatnonzero(owned)
    assert kept[own[0]] == 0 and kept[own[1]] == 1 and np.isfinite(sums).all()
    assert np.isinf(squares).any()  # 1e30: kept, its square overflows
    # kept < 2 has no finite e, whatever the sums: confirmed, not assumed
    se, e = F.stats(sums, squares, kept)
    low = owned & (kept < 2)
    assert low.sum() >= 2 and not np.isfinite(e[low]).any() and not np.isfinite(se[low]).any()
    assert (F.mean(sums, kept)[own[0]].view(np.uint32) == 0).all()  # kept 0 resolves to +0.0
    if len(own) > 20:
        assert kept[own[19]] == 2 and np.isfinite(e[own[19]])
        assert (stops[0] != 0).any() and (stops[0] == 0).any(), "the target must split the tiles"
        if tiles >= 10:
            assert len({tuple(s) for s in stops}) > 1, "tiles must stop in more than one round"
    # the preconditions stay on the frontier
    zero = np.zeros(tiles, np.uint32)
    assert host_adapt(sums, squares, kept, sz, tile, part, 1, 1.0, 2, zero)[0] == N.RTW_ERR_INVALID_ARGUMENT
    assert host_adapt(sums, squares, kept, sz, tile, part, SAMPLES, 1.0, 1, zero)[0] == N.RTW_ERR_INVALID_ARGUMENT
    rc, none = host_adapt(sums, squares, kept, sz, tile, part, SAMPLES, 1e30, SAMPLES + 1, zero)
    assert rc == N.RTW_OK and (none == 0).all()  # the frontier below min_samples: nothing stops


def test_kept_equal_to_samples_is_the_plain_accumulator():
    """Without a non-finite colour the finite sums and squares are the plain in-order ones, and the tile test
    with kept = n everywhere takes rtw_adapt_tiles_host's decisions."""
    sz, tile, part = R.Size2i(37, 23), (8, 8), (0, 1)
    rng = np.random.default_rng(3)
    slots = tile_slots(sz, tile, part)
    owned = slots >= 0
    colors = rng.random((SAMPLES, len(slots), 3), dtype=f32)
    colors[:, ~owned] = np.nan
    zero = np.zeros((len(slots), 3), f32)
    sums, squares, kept = host_accumulate(colors, zero, zero, np.zeros(len(slots), np.uint32))
    plain_s, plain_q = zero.copy(), zero.copy()
    for c in np.where(owned[None, :, None], colors, f32(0)):
        plain_s = plain_s + c
        plain_q = plain_q + c * c
    assert_bit_identical(sums, plain_s, "sums")
    assert_bit_identical(squares, plain_q, "squares")
    assert (kept[owned] == SAMPLES).all()
    E = A.tiles_E(sums, squares, SAMPLES, sz, tile, part)
    target = float(np.median(E))
    stop = np.zeros(len(slots) // 64, np.uint32)
    p = R.render_params(sz, 1, 1, tile=tile, part=part)
    plain = stop.copy()
    assert N.lib().rtw_adapt_tiles_host(sums.ctypes.data_as(f32p), squares.ctypes.data_as(f32p), C.byref(p), SAMPLES, target,
                                        MIN, plain.ctypes.data_as(u32p)) == N.RTW_OK
    rc, fin = host_adapt(sums, squares, kept, sz, tile, part, SAMPLES, target, MIN, stop)
    assert rc == N.RTW_OK and (fin == plain).all() and (fin != 0).any() and (fin == 0).any()


# ---- 3. the checkpoint file -----------------------------------------------------------------------------
def _state(kept, tile_stop=None) -> AccumState:
    rng = np.random.default_rng(5)
    tiles, per_tile = 7, 15
    slots = tiles * per_tile
    sums = rng.random((slots, 3), dtype=np.float32)
    flags = 4 | 1 | (2 if tile_stop is not None else 0)
    return AccumState(version=1, flags=flags if kept is not None else 1, width=50, height=30, tile_width=5, tile_height=3,
                      part_index=1, part_count=3, max_depth=9, render_mode=0, samples=4000000000, reserved=0,
                      seed=0xFEDCBA9876543210, world_fingerprint=0x8000000000000001, slots=slots, sums=sums,
                      squares=sums * sums, tile_stop=tile_stop, kept=kept)


def test_checkpoint_with_kept_round_trips_every_bit(tmp_path):
    kept = np.random.default_rng(1).integers(0, 2**32, 105, dtype=np.uint64).astype(np.uint32)
    for stop in (None, np.array([0, 2, 4000000000, 0, 17, 0xFFFFFFFF, 8], np.uint32)):
        s = _state(kept, stop)
        path = tmp_path / "finite.npz"
        s.save(path)
        t = AccumState.load(path)
        for n in HEADER_FIELDS:
            assert getattr(t, n) == getattr(s, n), n
        assert (t.sums.view(np.uint32) == s.sums.view(np.uint32)).all()
        assert t.kept.dtype == np.uint32 and t.kept.shape == (105,) and (t.kept == kept).all()
        assert (t.tile_stop is None) if stop is None else (t.tile_stop == stop).all()
        with np.load(path, allow_pickle=False) as z:
            assert set(z.files) == set(HEADER_FIELDS) | {"sums", "squares", "kept"} | ({"tile_stop"} if stop is not None else set())


def test_checkpoint_without_kept_loads_as_before(tmp_path):
    s = _state(None)
    path = tmp_path / "plain.npz"
    s.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(HEADER_FIELDS) | {"sums", "squares"}
    t = AccumState.load(path)
    assert t.kept is None and t.tile_stop is None and t.flags == 1


@pytest.mark.parametrize("bad", [np.zeros(105, np.int32), np.zeros(105, np.uint64), np.zeros(105, np.float32),
                                 np.zeros(104, np.uint32), np.zeros(106, np.uint32), np.zeros((105, 1), np.uint32),
                                 np.zeros(7, np.uint32)], ids=["int32", "uint64", "float32", "short", "long", "2d", "per_tile"])
def test_checkpoint_refuses_a_bad_kept(tmp_path, bad):
    with pytest.raises(ValueError, match="kept"):
        _state(bad).save(tmp_path / "refused.npz")  # save does not write one it would not load
    good = tmp_path / "good.npz"
    _state(np.zeros(105, np.uint32)).save(good)
    with np.load(good, allow_pickle=False) as z:
        arrays = {n: z[n] for n in z.files}
    arrays["kept"] = bad
    np.savez(tmp_path / "bad.npz", **arrays)
    with pytest.raises(ValueError, match="kept"):
        AccumState.load(tmp_path / "bad.npz")


# ---- the header --------------------------------------------------------------------------------------------
def test_header_compiles_as_c99():
    src = ('#include "rtw.h"\n#include "rtw_finite.h"\n'
           "typedef char flag_is_4[RTW_ACCUM_FINITE == 4 ? 1 : -1];\n"
           "int main(void){rtw_accum* a = 0; uint32_t k = 0; float s[3] = {0, 0, 0};\n"
           "rtw_finite_accumulate(s, 1u, 1u, s, 0, &k);\n"
           "return rtw_accum_resolve_kept(a, &k, 0) + rtw_accum_export_state(a, s, 0, 0, &k)\n"
           "+ rtw_accum_import_state(a, 0, s, 0, 0, &k) + rtw_finite_accumulate_host(s, 1u, 1u, s, 0, &k)\n"
           "+ rtw_adapt_tiles_finite_host(s, s, &k, 0, 2u, 0.5f, 2u, &k) + rtw_finite_sample(s[0], s[1], s[2])\n"
           "+ (int)rtw_finite_mean(s[0], k);}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)
    assert N.ACCUM_FINITE == 4
    assert set(N.declared_symbols(os.path.join(ROOT, "include", "rtw_finite.h"))) == {"rtw_finite_accumulate_host",
                                                                                     "rtw_adapt_tiles_finite_host"}


# ---- 4. the stand-alone program ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("finite")
    plain, san = str(d / "finite_check"), str(d / "finite_check_san")
    subprocess.run(["gcc", "-O2", *FLAGS, "-o", plain, SRC, "-lm"], check=True)
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *FLAGS, "-o", san,
                    SRC, "-lm"], check=True)
    return plain, san


def fnv(a: np.ndarray) -> int:
    u = a if a.dtype == np.uint32 else np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
    h = 0xCBF29CE484222325
    for b in np.ascontiguousarray(u).astype("<u4").tobytes():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_program_on_the_same_cases(programs, tmp_path, sanitized):
    exe = programs[1 if sanitized else 0]
    for size, tile, part in SHAPES:
        case = _case(size, tile, part)
        sz, colors, slots, owned, tiles, per_tile = case
        for moments in (1, 0):
            if moments:
                sums, squares, kept, stops, target = _replay(
                    case, size, tile, part, F.accumulate,
                    lambda s, q, k, n, t, stop: A.stop_rule(stop, F.tiles_E(s, q, k, sz, tile, part), n, t, MIN))
                se, e = F.stats(sums, squares, kept)
                want = [fnv(sums.ravel()), fnv(squares.ravel()), fnv(kept), fnv(F.mean(sums, kept).ravel()), fnv(se.ravel()), fnv(e)]
                low = owned & (kept < 2)
            else:
                sums, _, kept = F.accumulate(colors, moments=False)
                want = [fnv(sums.ravel()), 0, fnv(kept), fnv(F.mean(sums, kept).ravel()), 0, 0]
                stops, target = [], 0.0
            path = str(tmp_path / "case.bin")
            with open(path, "wb") as f:
                f.write(struct.pack("<6i4If", *size, *tile, *part, SAMPLES, BATCH, moments, MIN, target))
                f.write(colors.tobytes())
            out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, (size, tile, part, out.stdout[-2000:], out.stderr[-2000:])
            lines = out.stdout.split("\n")
            assert lines[0] == f"rc 0 slots {len(slots)}", lines[0]
            assert lines[1] == "sum " + " ".join(f"{v:016x}" for v in want), (size, tile, part, moments)
            assert lines[2] == (f"low {int(low.sum())} finite 0" if moments else "low 0 finite 0"), lines[2]
            assert [ln for ln in lines[3:] if ln] == ["stop " + " ".join(str(int(v)) for v in s) for s in stops]
