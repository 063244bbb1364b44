"""Sample clamping, the parts that need no GPU (include/rtw_clamp.h, include/rtw_parts.h, progressive.py; DESIGN.md
5.5j): the host twin rtw_clamp_accumulate_host against the numpy restatement (tests/clamp_ref.py) bit for bit on
synthetic colours, the partition record's layout for every flag combination, the host merge of records that carry
clamped and lost, and `AccumState` through save / load / merge / split."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.distributed import tile_slots
from raytracinginaweekend_amd.progressive import AccumState, merge_parts_host, record_layout
from tests import clamp_ref as K
from tests import finite_ref as F
from tests.parity import assert_bit_identical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
CLAMP_FLAGS = N.ACCUM_FINITE | N.ACCUM_CLAMP


def bits(u):
    return np.array(u, np.uint32).view(f32)


def level_bits(level) -> int:
    return int(np.array(level, f32).view(np.uint32))


def host_accumulate(colors, level, sums, squares, kept, clamped, lost):
    """rtw_clamp_accumulate_host on copies: colors (n, slots, 3)."""
    colors = np.ascontiguousarray(colors, f32)
    sums, kept, clamped, lost = sums.copy(), kept.copy(), clamped.copy(), lost.copy()
    squares = None if squares is None else squares.copy()
    rc = N.lib().rtw_clamp_accumulate_host(colors.ctypes.data_as(f32p), colors.shape[0], colors.shape[1], f32(level),
                                           sums.ctypes.data_as(f32p), squares.ctypes.data_as(f32p) if squares is not None else None,
                                           kept.ctypes.data_as(u32p), clamped.ctypes.data_as(u32p), lost.ctypes.data_as(f32p))
    assert rc == N.RTW_OK, N.lib().rtw_last_error()
    return sums, squares, kept, clamped, lost


def fresh(slots, moments=True):
    z = np.zeros((slots, 3), f32)
    return z, (z if moments else None), np.zeros(slots, np.uint32), np.zeros(slots, np.uint32), z


def same(got, want, what):
    for name, g, w in zip(("sums", "squares", "kept", "clamped", "lost"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            assert g.dtype == w.dtype
            assert_bit_identical(g.view(f32) if g.dtype == np.uint32 else g, w.view(f32) if w.dtype == np.uint32 else w,
                                 f"{what}: {name}")


# ---- 1. the twin against numpy on synthetic colours ------------------------------------------------------------
def rounds_above(level, rng, want=4):
    """Finite colours whose largest channel m exceeds `level` and for which mul(m, div(level, m)) rounds above the
    level: the samples that need the definition's final min."""
    level = f32(level)
    m = (level * (f32(1) + rng.random(1 << 16, dtype=f32) * f32(30))).astype(f32)
    m = m[m > level]
    s = (level / m).astype(f32)
    found = m[(m * s).astype(f32) > level]
    # (a level that is a power of two has none: m * fl(L / m) never rounds above it; 2 L stands in there)
    return np.concatenate([found[:want], np.full(max(0, want - found.size), 2 * level)]).astype(f32)


def synthetic(level, slots=96, samples=12, seed=5):
    """(samples, slots, 3): noise around the level (about a third of the samples above it), then the special values
    each on a slot of its own."""
    rng = np.random.default_rng(seed)
    level = f32(level)
    colors = (level * f32(1.6) * rng.random((samples, slots, 3), dtype=f32)).astype(f32)
    colors[:, :8] *= f32(0.3)  # slots without a clamped sample
    above = rounds_above(level, rng)
    specials = [(np.nan, 1, 1), (np.inf, 0.1, 0.1), (0.1, -np.inf, 0.1), bits([0x7FC00001, 0x3F800000, 0xFF800000]),
                (level, level, level),  # m == L exactly: not clamped
                (level, 0.0, -0.0), (np.nextafter(level, f32(np.inf)), level, 0.0),  # one ulp above: clamped
                (-5.0 * level, 27.5 * level, 0.25 * level),  # a negative channel beside a large one
                (-1e30, 1e20, 1e19), (3.4e38, 3.4e38, 1.0), (1e-40, 2.0 * level, 3e-45), (-1.0, -2.0, -3.0),
                (above[0], above[0], 0.5 * level), (0.0, above[1], above[1]), (above[2], 0.0, above[2]), (above[3],) * 3]
    for i, c in enumerate(specials):
        colors[(5 * i) % samples, 8 + i] = np.array(c, f32)
    colors[:, 30] = np.nan  # kept = 0
    colors[:, 31] = 30.0 * level  # every sample clamped
    colors[:, -4:] = np.nan  # padding slots
    return colors, above


MIN_LEVELS = (0.3, 0.7, 1e-3)  # levels at which mul(m, div(L, m)) can round above L


@pytest.mark.parametrize("level", [1.0, 0.5, 4.0] + list(MIN_LEVELS), ids=lambda v: f"L{v:g}")
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no_moments"])
def test_twin_against_numpy(level, moments):
    colors, above = synthetic(level)
    n, slots = colors.shape[:2]
    L = f32(level)
    # the inputs hold what the test is about
    v, hit = K.clamp_samples(colors, L)
    fin = F.finite(colors)
    assert (~fin).sum() >= 5 and hit.sum() >= 50 and not (hit & ~fin).any()
    with np.errstate(all="ignore"):
        raw = (colors * (L / colors.max(axis=-1)).astype(f32)[..., None]).astype(f32)
    if level in MIN_LEVELS:
        assert (hit[..., None] & (raw > L)).sum() >= 4, "no sample exercises the final min"
        assert ((above * (L / above).astype(f32)).astype(f32) > L).all()
    at = colors[5 * 4 % n, 8 + 4]
    assert (at == L).all() and not hit[5 * 4 % n, 8 + 4]  # m == L is not clamped
    assert hit[5 * 6 % n, 8 + 6] and hit[5 * 7 % n, 8 + 7]
    neg = v[5 * 7 % n, 8 + 7]  # the negative channel is scaled with the rest (27.5 L -> L up to a rounding)
    assert neg[0] < 0 and abs(neg[0] / L + f32(5 / 27.5)) < 1e-6 and L * f32(1 - 2e-7) <= neg[1] <= L
    assert (v[fin] <= L).all(), "an accumulated channel exceeds the level"
    want = K.accumulate(colors, L, moments=moments)
    got = host_accumulate(colors, L, *fresh(slots, moments))
    same(got, want, "one call")
    assert (got[2][30] == 0) and (got[3][31] == n) and (got[2][-4:] == 0).all() and (got[4][-4:].view(np.uint32) == 0).all()
    assert (got[3] <= got[2]).all()
    # split 5 + 7: the state carries
    a = host_accumulate(colors[:5], L, *fresh(slots, moments))
    b = host_accumulate(colors[5:], L, *a)
    same(b, want, "split add")
    same(K.accumulate(colors[5:], L, *K.accumulate(colors[:5], L, moments=moments), moments=moments), want, "numpy split")
    # no clamped sample: the finite accumulator's bits
    quiet = got[3] == 0
    fs, fq, fk = F.accumulate(colors, moments=moments)
    assert quiet.sum() >= 8
    assert_bit_identical(got[0][quiet], fs[quiet], "sums where nothing was clamped")
    assert (got[2] == fk).all() and (got[4][quiet].view(np.uint32) == 0).all()
    if moments:
        assert_bit_identical(got[1][quiet], fq[quiet], "squares where nothing was clamped")
    # the loss: what was removed, as a mean over kept
    loss = K.loss_mean(got[4], got[2])
    assert loss.dtype == f32 and (loss[got[2] == 0] == 0).all() and (loss[quiet] == 0).all()


def test_twin_refuses_a_bad_level():
    colors = np.zeros((1, 4, 3), f32)
    z, q, k, c, l = fresh(4)
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        rc = N.lib().rtw_clamp_accumulate_host(colors.ctypes.data_as(f32p), 1, 4, bad, z.copy().ctypes.data_as(f32p), None,
                                               k.ctypes.data_as(u32p), c.ctypes.data_as(u32p), l.copy().ctypes.data_as(f32p))
        assert rc == N.RTW_ERR_INVALID_ARGUMENT and b"clamp" in N.lib().rtw_last_error()


def test_header_is_c99_and_declares_the_twin():
    src = ('#include "rtw.h"\n#include "rtw_clamp.h"\n'
           "int main(void){float v[3]; return rtw_clamp_sample(1.f, 2.f, 3.f, 1.f, v) + (int)rtw_clamp_loss_mean(1.f, 0u)"
           " + rtw_clamp_level_ok(1.f) + rtw_clamp_accumulate_host(0, 0, 0, 1.f, 0, 0, 0, 0, 0);}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)
    assert set(N.declared_symbols(os.path.join(ROOT, "include", "rtw_clamp.h"))) == {"rtw_clamp_accumulate_host"}
    assert N.ACCUM_CLAMP == 8


# ---- 2. the record's layout for every flag combination ---------------------------------------------------------
@pytest.mark.parametrize("size,tile,n", [((50, 37), (8, 8), 3), ((50, 37), (5, 3), 3), ((20, 12), (8, 8), 1), ((9, 9), (4, 4), 7)])
def test_layout_offsets_for_every_flag_combination(size, tile, n):
    p = R.render_params(R.Size2i(*size), 0, 5, tile=tile)
    per_tile = tile[0] * tile[1]
    tiles0 = -(-(-(-size[0] // tile[0]) * -(-size[1] // tile[1])) // n)
    for flags in range(16):
        nbytes = C.c_int64()
        rc = N.lib().rtw_accum_packed_bytes(C.byref(p), flags, n, C.byref(nbytes))
        if (flags & N.ACCUM_CLAMP) and not (flags & N.ACCUM_FINITE):  # no such accumulator
            assert rc == N.RTW_ERR_INVALID_ARGUMENT
            continue
        assert rc == N.RTW_OK
        lay = record_layout(size[0], size[1], tile, flags, n)
        # the sections in the record's order, each after the one before: sums, squares, kept, clamped, lost, tile_stop
        at, order = 8, []
        for name, bit, per in (("sums", 0, 3 * per_tile), ("squares", N.ACCUM_MOMENTS, 3 * per_tile), ("kept", N.ACCUM_FINITE, per_tile),
                               ("clamped", N.ACCUM_CLAMP, per_tile), ("lost", N.ACCUM_CLAMP, 3 * per_tile),
                               ("stop", N.ACCUM_ADAPTIVE, 1)):
            if bit and not flags & bit:
                assert lay[name] is None
                continue
            assert lay[name] == at, (flags, name)
            order.append(name)
            at += per * tiles0
        assert lay["words"] == at and nbytes.value == 4 * at, (flags, order)
        assert len(order) <= 6
    assert N.lib().rtw_accum_packed_bytes(C.byref(p), 16, n, C.byref(nbytes)) == N.RTW_ERR_INVALID_ARGUMENT


# ---- 3. AccumState and the host merge ------------------------------------------------------------------------------
def whole_state(size, tile, flags, level, samples=12, seed=3):
    """A whole-image state of a clamp accumulator from the restatement on synthetic colours (padding slots zero)."""
    sz = R.Size2i(*size)
    slots = tile_slots(sz, tile, (0, 1))
    rng = np.random.default_rng(seed)
    colors = (f32(2.5) * f32(level) * rng.random((samples, len(slots), 3), dtype=f32) ** 3).astype(f32)
    colors[rng.random((samples, len(slots))) < 0.02] = np.nan
    colors[:, slots < 0] = np.nan
    moments = bool(flags & N.ACCUM_MOMENTS)
    sums, squares, kept, clamped, lost = K.accumulate(colors, f32(level), moments=moments)
    assert (clamped > 0).sum() > len(slots) // 4 and (kept < samples)[slots >= 0].any()
    n_tiles = len(slots) // (tile[0] * tile[1])
    stop = None
    if flags & N.ACCUM_ADAPTIVE:
        stop = np.where(np.arange(n_tiles) % 3 == 1, 8, 0).astype(np.uint32)
    return AccumState(version=1, flags=flags, width=size[0], height=size[1], tile_width=tile[0], tile_height=tile[1],
                      part_index=0, part_count=1, max_depth=50, render_mode=0, samples=samples, reserved=level_bits(level),
                      seed=77, world_fingerprint=0x1234_5678_9ABC_DEF0, slots=len(slots), sums=sums, squares=squares,
                      tile_stop=stop, kept=kept, clamped=clamped, lost=lost)


def same_state(a: AccumState, b: AccumState, what=""):
    assert a.header() == b.header(), what
    for name in ("sums", "squares", "tile_stop", "kept", "clamped", "lost"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and (x.view(np.uint32) == y.view(np.uint32)).all(), (what, name)


FLAG_SETS = [CLAMP_FLAGS, CLAMP_FLAGS | N.ACCUM_MOMENTS, CLAMP_FLAGS | N.ACCUM_MOMENTS | N.ACCUM_ADAPTIVE]


@pytest.mark.parametrize("flags", FLAG_SETS, ids=["clamp", "moments", "adaptive"])
@pytest.mark.parametrize("tile", [(8, 8), (5, 3)], ids=["tile8x8", "tile5x3"])
def test_state_round_trips(flags, tile, tmp_path):
    whole = whole_state((50, 37), tile, flags, 0.75)
    assert whole.clamp == 0.75
    whole.save(tmp_path / "whole.npz")
    same_state(AccumState.load(tmp_path / "whole.npz"), whole, "save / load")
    for m in (1, 2, 3, 7):
        parts = whole.split(m)
        assert all(p.clamp == 0.75 and p.clamped.shape == (p.slots,) and p.lost.shape == (p.slots, 3) for p in parts)
        same_state(AccumState.merge(reversed(parts)), whole, f"merge(split({m}))")
        # the records: numpy's packing, merged by the library's host twin (odd stride: nothing depends on 16 bytes)
        for pad in (0, 4):
            stride = 4 * record_layout(50, 37, tile, flags, m)["words"] + pad
            gathered = np.concatenate([p.packed(stride) for p in parts])
            assert all(int(p.packed()[7]) == level_bits(0.75) for p in parts)
            same_state(merge_parts_host(parts[-1], gathered, stride, m), whole, f"host merge of {m} records")
    # re-partition 3 -> 2 through merge
    same_state(AccumState.merge(AccumState.merge(whole.split(3)).split(2)), whole, "3 -> 2")


def test_states_of_different_levels_do_not_merge():
    flags = CLAMP_FLAGS | N.ACCUM_MOMENTS
    a, b = whole_state((50, 37), (8, 8), flags, 0.75).split(2), whole_state((50, 37), (8, 8), flags, 0.5).split(2)
    with pytest.raises(ValueError, match="clamp"):
        AccumState.merge([a[0], b[1]])
    # ... nor their records
    stride = 4 * record_layout(50, 37, (8, 8), flags, 2)["words"]
    with pytest.raises(N.RtwError) as e:
        merge_parts_host(a[0], np.concatenate([a[0].packed(stride), b[1].packed(stride)]), stride, 2)
    assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT and "clamp" in str(e.value) and "record 1" in str(e.value)
    # the older entry point names the flag; a record without the flag still names `reserved` for a non-zero last word
    p = R.render_params(R.Size2i(50, 37), 0, 50, seed=77)
    gathered = np.concatenate([s.packed(stride) for s in a])
    z3, z1, n = np.zeros((7 * 5 * 64, 3), f32), np.zeros(7 * 5 * 64, np.uint32), C.c_uint32()
    rc = N.lib().rtw_accum_merge_parts_host(C.byref(p), flags, C.c_void_p(gathered.ctypes.data), stride, 2, z3.ctypes.data_as(f32p),
                                            z3.copy().ctypes.data_as(f32p), z1.ctypes.data_as(u32p), None, C.byref(n))
    assert rc == N.RTW_ERR_INVALID_ARGUMENT and b"RTW_ACCUM_CLAMP" in N.lib().rtw_last_error()
    plain = AccumState.merge(a)
    plain = AccumState(**{**plain.header(), "flags": N.ACCUM_FINITE | N.ACCUM_MOMENTS, "reserved": 0}, sums=plain.sums,
                       squares=plain.squares, kept=plain.kept)
    rec = plain.packed()
    rec[7] = level_bits(0.75)
    with pytest.raises(N.RtwError) as e:
        merge_parts_host(plain, rec, 4 * rec.size, 1)
    assert "reserved" in str(e.value)


def test_state_file_refusals(tmp_path):
    st = whole_state((20, 12), (8, 8), CLAMP_FLAGS, 1.0)
    st.lost = None
    with pytest.raises(ValueError, match="clamped and lost"):
        st.save(tmp_path / "bad.npz")
    st = whole_state((20, 12), (8, 8), CLAMP_FLAGS, 1.0)
    st.clamped = st.clamped.astype(np.int64)
    with pytest.raises(ValueError, match="clamped"):
        st.save(tmp_path / "bad.npz")
    assert AccumState(**{**st.header(), "flags": N.ACCUM_FINITE}, sums=st.sums).clamp is None
