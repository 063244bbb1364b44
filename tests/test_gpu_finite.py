"""Finite-sample accumulation on the device (RTW_ACCUM_FINITE, progressive.py).

The contract is per pixel: the sums, squares and kept counts are the in-order accumulation of the pixel's finite
samples, and a sample's colour is a fixed function of (seed, pixel, sample), so the oracle's per-sample colours and
a numpy restatement (tests/finite_ref.py) give every bit.  The shapes are the smallest that split an add, cross a
tile edge and meet a NaN sample."""
import ctypes as C

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.distributed import tile_slots
from raytracinginaweekend_amd.progressive import AccumState
from tests import adaptive_ref as A
from tests import finite_ref as F
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

DEPTH, SEED, TILE = 10, 31, (8, 8)
SIZE = R.Size2i(37, 19)
f32 = np.float32
f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def by_slot(image, slots, layout):
    """An image() / stderr() / *_counts() result on the owned slots, in slot order."""
    owned = slots >= 0
    return image[owned] if layout == N.LAYOUT_TILES else image[slots[owned]]


def check_against_numpy(acc, colors, slots, layout, moments):
    """Everything the accumulator shows after acc.samples samples, against the restatement on the first
    acc.samples of `colors` ((n, slots, 3), slot order, padding NaN)."""
    n, owned = acc.samples, slots >= 0
    sums, squares, kept = F.accumulate(colors[:n], moments=moments)
    st = acc.state()
    assert st.flags == (5 if moments else 4) and st.samples == n and st.tile_stop is None
    assert_bit_identical(st.sums, sums, f"sums at {n}")
    assert (st.kept == kept).all(), f"kept at {n}"
    assert (st.kept[~owned] == 0).all() and (st.sums.view(np.uint32)[~owned] == 0).all()
    assert np.isfinite(st.sums).all()
    assert_bit_identical(by_slot(acc.image(), slots, layout), F.mean(sums, kept)[owned], f"image at {n}")
    counts, got_kept, rejected = acc.sample_counts(), acc.kept_counts(), acc.rejected_counts()
    assert got_kept.dtype == rejected.dtype == np.uint32 and got_kept.shape == counts.shape == rejected.shape
    assert (by_slot(got_kept, slots, layout)[:, 0] == kept[owned]).all()
    assert (by_slot(rejected, slots, layout)[:, 0] == n - kept[owned]).all()
    if layout == N.LAYOUT_TILES:
        assert (got_kept[~owned] == 0).all() and (rejected[~owned] == 0).all()
    if not moments:
        assert st.squares is None
        return kept
    assert_bit_identical(st.squares, squares, f"squares at {n}")
    assert (st.squares.view(np.uint32)[~owned] == 0).all()
    if n >= 2:
        se, e = F.stats(sums, squares, kept)
        assert_bit_identical(by_slot(acc.stderr(), slots, layout), se[owned], f"standard error at {n}")
        want, pixels = F.noise(e, owned)
        noise, counted = acc.noise()
        print(f"samples {n}: noise {noise!r} numpy {want!r} pixels {counted} of {int(owned.sum())}")
        assert counted == pixels
        assert abs(noise - want) <= 1e-9 * abs(want)  # test_moments' tolerance for the f64 mean
    return kept


# ---- 5. suzanne against the oracle's samples -----------------------------------------------------------------
@pytest.mark.parametrize("moments,part,layout,split", [(True, (0, 1), N.LAYOUT_IMAGE, False), (False, (0, 1), N.LAYOUT_IMAGE, False),
                                                        (True, (1, 3), N.LAYOUT_TILES, False), (True, (0, 1), N.LAYOUT_IMAGE, True)],
                         ids=["moments", "finite_alone", "part1of3_tiles", "several_launches"])
def test_suzanne_against_the_oracle_samples(worlds, monkeypatch, moments, part, layout, split):
    world = worlds("suzanne")
    slots = tile_slots(SIZE, TILE, part)
    colors = F.to_slots(F.oracle_samples(world, R.render_params(SIZE, 16, DEPTH, seed=SEED), 16), slots)
    if split:  # 960 slots x 12 B: 4 samples fit, so 3 (one chunk) per launch
        monkeypatch.setenv("RTW_SAMPLE_BUFFER_BYTES", "50000")
        monkeypatch.setenv("RTW_CHUNK", "3")
    acc = R.Accumulator(world, SIZE, DEPTH, seed=SEED, tile=TILE, part=part, layout=layout, moments=moments, finite=True)
    assert acc.finite and acc.moments is moments and (acc.state().kept == 0).all()
    for n in (4, 4, 8):
        acc.add(n)
        frame = acc.dworld.last_frame()
        assert frame["whole_pixel"] is False  # a finite accumulator filters in the accumulate pass
        assert (frame["launches"] > 1) is split
        kept = check_against_numpy(acc, colors, slots, layout, moments)
    owned = slots >= 0
    bad = ~F.finite(colors[:, owned])
    rejected = bad.sum(axis=0)
    first = np.where(rejected > 0, bad.argmax(axis=0), 16)
    assert (kept[owned] == 16 - rejected).all()
    if part == (0, 1):  # rejected samples on both sides of every add's boundary
        assert (rejected > 0).sum() >= 10 and (first < 8).sum() >= 4 and (kept[owned] > 0).all()
    else:
        assert (rejected > 0).any()
    acc.release()


# ---- 6. a world without non-finite samples ----------------------------------------------------------------
def test_no_rejected_sample_equals_the_plain_accumulator(worlds):
    world = worlds("final_scene1")
    dw = R.DeviceWorld(world, 0)
    plain = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, moments=True)
    fin = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, moments=True, finite=True)
    alone = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, finite=True)
    owned = tile_slots(SIZE, TILE, (0, 1)) >= 0
    for n in (3, 5):
        for acc in (plain, fin, alone):
            acc.add(n)
        a, b, c = fin.state(), plain.state(), alone.state()
        assert a.samples == b.samples == c.samples and b.kept is None
        assert_bit_identical(a.sums, b.sums, f"sums after {a.samples}")
        assert_bit_identical(a.squares, b.squares, f"squares after {a.samples}")
        assert_bit_identical(c.sums, b.sums, f"sums without moments after {a.samples}")
        assert (a.kept[owned] == a.samples).all() and (a.kept[~owned] == 0).all() and (c.kept == a.kept).all()
        assert_bit_identical(fin.image(), plain.image(), f"image after {a.samples}")
        assert_bit_identical(alone.image(), plain.image(), f"image without moments after {a.samples}")
    assert_bit_identical(fin.stderr(), plain.stderr(), "standard error")
    assert fin.noise() == plain.noise()
    assert (fin.kept_counts() == 8).all() and (fin.rejected_counts() == 0).all()
    image, rejected = R.render_finite(SIZE, 8, DEPTH, world, seed=SEED)
    assert_bit_identical(image, plain.image(), "render_finite")
    assert rejected.shape == (SIZE.count(), 1) and (rejected == 0).all()


# ---- 7. adaptive + finite -----------------------------------------------------------------------------------
def test_adaptive_finite_replays_on_the_host(worlds):
    world, size, MIN, BATCH, MAX = worlds("suzanne"), R.Size2i(64, 36), 8, 4, 32
    slots = tile_slots(size, TILE, (0, 1))
    owned, per_tile = slots >= 0, TILE[0] * TILE[1]
    p = R.render_params(size, 1, DEPTH, seed=SEED, tile=TILE)
    dw = R.DeviceWorld(world, 0)
    ref = R.Accumulator(dw, size, DEPTH, seed=SEED, moments=True, finite=True)  # (pinned to the oracle by test 5)
    acc = R.Accumulator(dw, size, DEPTH, seed=SEED, adaptive=True, finite=True)
    states, target, stop_maps = {}, None, []
    while acc.samples < MAX and (acc.tile_stops() == 0).any():
        acc.add(BATCH)
        ref.add(BATCH)
        n = acc.samples
        r = ref.state()
        states[n] = r
        if n < MIN:
            continue
        if target is None:  # the median tile E at 8 samples
            bad = owned & (r.kept < n)
            print("at 8 samples:", int((n - r.kept[owned]).sum()), "rejected samples in", int(bad.sum()), "pixels")
            assert bad.sum() >= 10, "the frame must hold rejected samples"
            target = float(f32(np.median(F.tiles_E(r.sums, r.squares, r.kept, size, TILE, (0, 1)))))
        st = acc.state()
        assert st.flags == 7
        want = st.tile_stop.copy()
        assert N.lib().rtw_adapt_tiles_finite_host(st.sums.ctypes.data_as(f32p), st.squares.ctypes.data_as(f32p),
                                                   st.kept.ctypes.data_as(u32p), C.byref(p), n, target, MIN,
                                                   want.ctypes.data_as(u32p)) == N.RTW_OK
        numpy_stop = A.stop_rule(st.tile_stop, F.tiles_E(st.sums, st.squares, st.kept, size, TILE, (0, 1)), n, target, MIN)
        assert (want == numpy_stop).all()
        active_tiles, _ = acc.adapt(target, MIN)
        got = acc.tile_stops()
        assert (got == want).all(), (n, got, want)
        assert active_tiles == int((want == 0).sum())
        stop_maps.append((n, got, acc.state()))
    stopped_at = np.unique(stop_maps[-1][1])
    print("target", target, "stops", dict(zip(*np.unique(stop_maps[-1][1], return_counts=True))))
    assert len(stopped_at[stopped_at != 0]) >= 2, "tiles must stop at more than one count"
    final = acc.state()
    slot_n = A.expand(np.where(final.tile_stop != 0, final.tile_stop, acc.samples), per_tile)
    for n in np.unique(slot_n):  # every tile holds the non-adaptive finite accumulator's state at its own count
        sel = slot_n == n
        assert_bit_identical(final.sums[sel], states[int(n)].sums[sel], f"sums of the tiles at {n}")
        assert_bit_identical(final.squares[sel], states[int(n)].squares[sel], f"squares of the tiles at {n}")
        assert (final.kept[sel] == states[int(n)].kept[sel]).all()
    for n, stop, st in stop_maps:  # a stopped tile's state did not change in any later add
        sel = A.expand(stop != 0, per_tile)
        assert_bit_identical(final.sums[sel], st.sums[sel], f"sums of the tiles stopped by {n}")
        assert_bit_identical(final.squares[sel], st.squares[sel], f"squares of the tiles stopped by {n}")
        assert (final.kept[sel] == st.kept[sel]).all()
    counts, kept = acc.sample_counts(), acc.kept_counts()
    assert (counts[slots[owned], 0] == slot_n[owned]).all() and (kept[slots[owned], 0] == final.kept[owned]).all()
    assert (acc.rejected_counts()[slots[owned], 0] == slot_n[owned] - final.kept[owned]).all()
    assert_bit_identical(acc.image()[slots[owned]], F.mean(final.sums, final.kept)[owned], "image with per-pixel kept")
    se, e = F.stats(final.sums, final.squares, final.kept)
    assert_bit_identical(acc.stderr()[slots[owned]], se[owned], "standard error with per-pixel kept")
    want_noise, pixels = F.noise(e, owned)
    noise, counted = acc.noise()
    assert counted == pixels and abs(noise - want_noise) <= 1e-9 * abs(want_noise)


# ---- 8. checkpoint and refusals -------------------------------------------------------------------------------
def test_checkpoint_resume(worlds, tmp_path):
    world = worlds("suzanne")
    whole = R.Accumulator(world, SIZE, DEPTH, seed=SEED, moments=True, finite=True)
    whole.add(8)
    path = tmp_path / "finite.npz"
    whole.state().save(path)
    whole.add(8)
    state = AccumState.load(path)
    assert state.flags == 5 and state.samples == 8 and state.kept is not None and (state.kept < 8).any()
    fresh = R.Accumulator(R.DeviceWorld(world, 0), SIZE, DEPTH, seed=SEED, moments=True, finite=True)
    fresh.load_state(state)
    assert fresh.samples == 8 and (fresh.state().kept == state.kept).all()
    fresh.add(8)
    a, b = fresh.state(), whole.state()
    assert_bit_identical(a.sums, b.sums, "resumed sums")
    assert_bit_identical(a.squares, b.squares, "resumed squares")
    assert (a.kept == b.kept).all() and (b.kept < 16).any()
    assert_bit_identical(fresh.image(), whole.image(), "resumed image")


def test_refusals(worlds):
    world = worlds("simple_plane")
    size = R.Size2i(20, 12)  # 3 x 2 tiles, padded in both axes
    dw = R.DeviceWorld(world, 0)
    L = N.lib()
    p = R.render_params(size, 0, DEPTH, seed=SEED)
    h = C.c_void_p()
    assert L.rtw_accum_create(dw._h, C.byref(p), 8, C.byref(h)) == N.RTW_ERR_INVALID_ARGUMENT  # an unknown flag bit
    assert b"unknown" in L.rtw_last_error()
    assert L.rtw_accum_create(dw._h, C.byref(p), N.ACCUM_FINITE | N.ACCUM_ADAPTIVE, C.byref(h)) == N.RTW_ERR_INVALID_ARGUMENT
    with pytest.raises(N.RtwError) as e:
        R.Accumulator(dw, size, DEPTH, seed=SEED, finite=True, thread_count=2)
    assert e.value.code == N.RTW_ERR_UNSUPPORTED

    def refused(rc, word):
        assert rc == N.RTW_ERR_INVALID_ARGUMENT
        assert word in L.rtw_last_error().decode(), L.rtw_last_error()

    fin = R.Accumulator(dw, size, DEPTH, seed=SEED, moments=True, finite=True)
    plain = R.Accumulator(dw, size, DEPTH, seed=SEED, moments=True)
    alone = R.Accumulator(dw, size, DEPTH, seed=SEED, finite=True)
    for acc in (fin, plain, alone):
        acc.add(4)
    st = fin.state()
    info = fin.info()
    s, q, k = st.sums.ctypes.data_as(f32p), st.squares.ctypes.data_as(f32p), st.kept.ctypes.data_as(u32p)
    stop = np.zeros(fin.tiles, np.uint32)
    t = stop.ctypes.data_as(u32p)
    # the two older pairs refuse a finite accumulator by name
    refused(L.rtw_accum_export(fin._h, s, q), "RTW_ACCUM_FINITE")
    refused(L.rtw_accum_import(fin._h, C.byref(info), s, q), "RTW_ACCUM_FINITE")
    refused(L.rtw_accum_export_adaptive(fin._h, s, q, t), "RTW_ACCUM_FINITE")
    refused(L.rtw_accum_import_adaptive(fin._h, C.byref(info), s, q, t), "RTW_ACCUM_FINITE")
    # the new pair: a pointer the flags call for is non-null, any other is null
    refused(L.rtw_accum_export_state(fin._h, s, q, None, None), "kept")
    refused(L.rtw_accum_export_state(fin._h, s, None, None, k), "squares")
    refused(L.rtw_accum_export_state(fin._h, s, q, t, k), "tile_stop")
    refused(L.rtw_accum_export_state(alone._h, s, q, None, k), "squares")
    refused(L.rtw_accum_export_state(plain._h, s, q, None, k), "kept")
    refused(L.rtw_accum_import_state(fin._h, C.byref(info), s, q, None, None), "kept")
    refused(L.rtw_accum_import_state(fin._h, C.byref(info), s, q, t, k), "tile_stop")
    refused(L.rtw_accum_import_state(plain._h, C.byref(plain.info()), s, q, None, k), "kept")
    assert L.rtw_accum_export_state(plain._h, s, q, None, None) == N.RTW_OK  # ... one pair for every combination
    assert_bit_identical(st.sums, plain.state().sums, "a plain accumulator through the new pair")
    assert L.rtw_accum_import_state(plain._h, C.byref(plain.info()), s, q, None, None) == N.RTW_OK
    with pytest.raises(N.RtwError) as e:
        plain.kept_counts()
    assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT and "RTW_ACCUM_FINITE" in str(e.value)
    # kept above the slot's count, and in a padding slot
    slots = tile_slots(size, TILE, (0, 1))
    for slot, bad in ((int(np.flatnonzero(slots >= 0)[5]), 5), (int(np.flatnonzero(slots < 0)[0]), 1)):
        st = fin.state()
        st.kept[slot] = bad
        with pytest.raises(N.RtwError) as e:
            fin.load_state(st)
        assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT and "kept" in str(e.value), str(e.value)
    st = fin.state()
    st.kept[int(np.flatnonzero(slots >= 0)[5])] = 3  # below the count: taken
    fin.load_state(st)
    assert (fin.state().kept == st.kept).all() and fin.samples == 4
    st.kept = None  # a state without kept into a finite accumulator
    with pytest.raises(N.RtwError) as e:
        fin.load_state(st)
    assert "kept" in str(e.value)


# ---- 9. the denoised preview ------------------------------------------------------------------------------
def test_denoised_preview_is_finite(worlds):
    world, size = worlds("suzanne"), R.Size2i(64, 36)
    dw = R.DeviceWorld(world, 0)
    fin = R.Accumulator(dw, size, DEPTH, seed=SEED, moments=True, finite=True)
    plain = R.Accumulator(dw, size, DEPTH, seed=SEED, moments=True)
    fin.add(8)
    plain.add(8)
    assert (fin.rejected_counts() > 0).sum() >= 10
    preview = fin.denoised()
    assert np.isfinite(preview).all()
    assert_bit_identical(preview, R.denoise_host(size, fin.image(), fin.stderr()), "the preview against the host filter")
    holes = np.isnan(plain.image()).any(axis=1)
    assert holes.sum() >= 10 and ((fin.rejected_counts()[:, 0] > 0) == holes).all()
    assert np.isnan(plain.denoised()[holes]).any(axis=1).all()  # the plain preview still holds its NaN pixels
