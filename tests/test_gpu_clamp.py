"""Sample clamping on the device (RTW_ACCUM_CLAMP, progressive.py; include/rtw_clamp.h).

The contract is per pixel: sums, squares, kept, clamped and lost are the in-order accumulation of the pixel's
samples under the definition, and a sample's colour is a fixed function of (seed, pixel, sample), so the oracle's
per-sample colours (finite_ref.oracle_samples) and the numpy restatement (tests/clamp_ref.py) give every bit.  The
shapes are the smallest that split an add, cross a tile edge and meet clamped and non-finite samples."""
import ctypes as C
import os
import socket
import time

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.distributed import tile_slots
from raytracinginaweekend_amd.progressive import AccumState, merge_parts_host
from tests import adaptive_ref as A
from tests import clamp_ref as K
from tests import finite_ref as F
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH, SEED, TILE = 10, 31, (8, 8)
SIZE = R.Size2i(37, 19)
f32 = np.float32
f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def by_slot(image, slots, layout):
    """An image() / stderr() / clamp_loss() / *_counts() result on the owned slots, in slot order."""
    owned = slots >= 0
    return image[owned] if layout == N.LAYOUT_TILES else image[slots[owned]]


def same_state(a: AccumState, b: AccumState, what="") -> None:
    assert a.header() == b.header(), what
    for name in ("sums", "squares", "tile_stop", "kept", "clamped", "lost"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.shape == y.shape and (x.view(np.uint32) == y.view(np.uint32)).all(), (what, name)


def check_against_numpy(acc, colors, level, slots, layout, moments):
    """Everything the accumulator shows after acc.samples samples, against the restatement on the first acc.samples
    of `colors` ((n, slots, 3), slot order, padding NaN)."""
    n, owned = acc.samples, slots >= 0
    sums, squares, kept, clamped, lost = K.accumulate(colors[:n], f32(level), moments=moments)
    st = acc.state()
    assert st.flags == (13 if moments else 12) and st.samples == n and st.tile_stop is None and st.clamp == level
    assert_bit_identical(st.sums, sums, f"sums at {n}")
    assert_bit_identical(st.lost, lost, f"lost at {n}")
    assert (st.kept == kept).all() and (st.clamped == clamped).all(), f"kept / clamped at {n}"
    for plane in (st.sums, st.lost, st.kept, st.clamped):
        assert (plane.view(np.uint32)[~owned] == 0).all()
    assert np.isfinite(st.sums).all() and (st.clamped <= st.kept).all()
    assert_bit_identical(by_slot(acc.image(), slots, layout), F.mean(sums, kept)[owned], f"image at {n}")
    assert_bit_identical(by_slot(acc.clamp_loss(), slots, layout), K.loss_mean(lost, kept)[owned], f"clamp loss at {n}")
    got = acc.clamped_counts()
    assert got.dtype == np.uint32 and got.shape == acc.kept_counts().shape
    assert (by_slot(got, slots, layout)[:, 0] == clamped[owned]).all()
    assert (by_slot(acc.kept_counts(), slots, layout)[:, 0] == kept[owned]).all()
    if layout == N.LAYOUT_TILES:
        assert (got[~owned] == 0).all() and (acc.clamp_loss().view(np.uint32)[~owned] == 0).all()
    if not moments:
        assert st.squares is None
        return
    assert_bit_identical(st.squares, squares, f"squares at {n}")
    assert (st.squares.view(np.uint32)[~owned] == 0).all()
    if n >= 2:
        se, e = F.stats(sums, squares, kept)
        assert_bit_identical(by_slot(acc.stderr(), slots, layout), se[owned], f"standard error at {n}")
        want, pixels = F.noise(e, owned)
        noise, counted = acc.noise()
        print(f"samples {n}: noise {noise!r} numpy {want!r} pixels {counted} of {int(owned.sum())}")
        assert counted == pixels and abs(noise - want) <= 1e-9 * abs(want)


CASES = [(True, (0, 1), N.LAYOUT_IMAGE, False), (False, (0, 1), N.LAYOUT_IMAGE, False), (True, (1, 3), N.LAYOUT_TILES, False),
         (True, (0, 1), N.LAYOUT_IMAGE, True)]
IDS = ["moments", "clamp_alone", "part1of3_tiles", "several_launches"]


def run_against_the_oracle(worlds, monkeypatch, name, level, moments, part, layout, split):
    world = worlds(name)
    slots = tile_slots(SIZE, TILE, part)
    per_pixel = F.oracle_samples(world, R.render_params(SIZE, 16, DEPTH, seed=SEED), 16)
    colors = F.to_slots(per_pixel, slots)
    if split:  # 960 slots x 12 B: 4 samples fit, so 3 (one chunk) per launch
        monkeypatch.setenv("RTW_SAMPLE_BUFFER_BYTES", "50000")
        monkeypatch.setenv("RTW_CHUNK", "3")
    acc = R.Accumulator(world, SIZE, DEPTH, seed=SEED, tile=TILE, part=part, layout=layout, moments=moments, clamp=level)
    assert acc.finite and acc.clamp == level and acc.moments is moments
    st = acc.state()
    assert (st.clamped == 0).all() and (st.lost.view(np.uint32) == 0).all() and acc.info().reserved == f32(level).view(np.uint32)
    for n in (4, 4, 8):
        acc.add(n)
        frame = acc.dworld.last_frame()
        assert frame["whole_pixel"] is False  # a clamp accumulator sees the samples in the accumulate pass
        assert (frame["launches"] > 1) is split
        check_against_numpy(acc, colors, level, slots, layout, moments)
    acc.release()
    return per_pixel


# ---- 1. cornell_box, L = 1.0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments,part,layout,split", CASES, ids=IDS)
def test_cornell_box_against_the_oracle_samples(worlds, monkeypatch, moments, part, layout, split):
    per_pixel = F.oracle_samples(worlds("cornell_box"), R.render_params(SIZE, 16, DEPTH, seed=SEED), 16)
    _, hit = K.clamp_samples(per_pixel, 1.0)
    print("clamped samples", int(hit.sum()), "pixels", int(hit.any(axis=0).sum()), "first 8", int(hit[:8].any(axis=0).sum()),
          "last 8", int(hit[8:].any(axis=0).sum()), "largest", float(np.nanmax(per_pixel)))
    assert hit.any(axis=0).sum() >= 50 and hit[:8].any(axis=0).sum() >= 20 and hit[8:].any(axis=0).sum() >= 20
    run_against_the_oracle(worlds, monkeypatch, "cornell_box", 1.0, moments, part, layout, split)


# ---- 2. suzanne, L = 0.5: clamping and rejection together ------------------------------------------------------
@pytest.mark.parametrize("moments,part,layout,split", CASES, ids=IDS)
def test_suzanne_clamps_and_rejects(worlds, monkeypatch, moments, part, layout, split):
    per_pixel = F.oracle_samples(worlds("suzanne"), R.render_params(SIZE, 16, DEPTH, seed=SEED), 16)
    _, hit = K.clamp_samples(per_pixel, 0.5)
    bad = ~F.finite(per_pixel)
    both = hit.any(axis=0) & bad.any(axis=0)
    print("pixels with both", int(both.sum()), "clamped samples", int(hit.sum()), "non-finite", int(bad.sum()))
    assert both.sum() >= 5
    run_against_the_oracle(worlds, monkeypatch, "suzanne", 0.5, moments, part, layout, split)


# ---- 3. a level nothing reaches -------------------------------------------------------------------------------
def test_a_level_nothing_reaches_equals_the_finite_accumulator(worlds):
    world = worlds("final_scene1")
    dw = R.DeviceWorld(world, 0)
    fin = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, moments=True, finite=True)
    cl = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, moments=True, clamp=3e38)
    alone = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, clamp=3e38)
    for n in (3, 5):
        for acc in (fin, cl, alone):
            acc.add(n)
        a, b, c = cl.state(), fin.state(), alone.state()
        assert a.samples == b.samples == c.samples and b.clamped is None
        assert_bit_identical(a.sums, b.sums, f"sums after {a.samples}")
        assert_bit_identical(a.squares, b.squares, f"squares after {a.samples}")
        assert_bit_identical(c.sums, b.sums, f"sums without moments after {a.samples}")
        assert (a.kept == b.kept).all() and (c.kept == b.kept).all()
        for st in (a, c):
            assert (st.clamped == 0).all() and (st.lost.view(np.uint32) == 0).all()
        assert_bit_identical(cl.image(), fin.image(), f"image after {a.samples}")
        assert_bit_identical(alone.image(), fin.image(), f"image without moments after {a.samples}")
    assert_bit_identical(cl.stderr(), fin.stderr(), "standard error")
    assert cl.noise() == fin.noise()
    assert (cl.clamped_counts() == 0).all() and (cl.clamp_loss().view(np.uint32) == 0).all()
    image, clamped, loss = R.render_clamped(SIZE, 8, DEPTH, world, 3e38, seed=SEED)
    assert_bit_identical(image, fin.image(), "render_clamped")
    assert clamped.shape == (SIZE.count(), 1) and (clamped == 0).all() and loss.shape == (SIZE.count(), 3) and (loss == 0).all()
    dw.release()


# ---- 4. adaptive + clamp --------------------------------------------------------------------------------------
def test_adaptive_clamp_replays_from_the_restatement(worlds):
    world, level, MIN, BATCH, MAX = worlds("cornell_box"), 1.0, 8, 4, 16
    slots = tile_slots(SIZE, TILE, (0, 1))
    owned, per_tile = slots >= 0, TILE[0] * TILE[1]
    colors = F.to_slots(F.oracle_samples(world, R.render_params(SIZE, 16, DEPTH, seed=SEED), 16), slots)
    ref = {n: K.accumulate(colors[:n], f32(level)) for n in range(BATCH, MAX + 1, BATCH)}
    target = float(f32(np.median(F.tiles_E(*ref[MIN][:3], SIZE, TILE, (0, 1)))))
    acc = R.Accumulator(world, SIZE, DEPTH, seed=SEED, adaptive=True, clamp=level)
    stop = np.zeros(acc.tiles, np.uint32)
    while acc.samples < MAX and (stop == 0).any():
        acc.add(BATCH)
        n = acc.samples
        if n < MIN:
            continue
        # the replay: active tiles hold the restatement's state at n, so its sums, squares and kept decide
        stop = A.stop_rule(stop, F.tiles_E(*ref[n][:3], SIZE, TILE, (0, 1)), n, target, MIN)
        active, _ = acc.adapt(target, MIN)
        assert (acc.tile_stops() == stop).all(), (n, acc.tile_stops(), stop)
        assert active == int((stop == 0).sum())
    print("target", target, "stops", dict(zip(*np.unique(stop, return_counts=True))))
    assert len(np.unique(stop[stop != 0])) >= 1 and (stop == MIN).any()
    final = acc.state()
    assert final.flags == 15 and (final.tile_stop == stop).all()
    slot_n = A.expand(np.where(stop != 0, stop, acc.samples), per_tile)
    for n in np.unique(slot_n):  # every tile holds the restatement's state at its own count
        sel = slot_n == n
        for name, want in zip(("sums", "squares", "kept", "clamped", "lost"), ref[int(n)]):
            got = getattr(final, name)
            assert (got.view(np.uint32)[sel] == want.view(np.uint32)[sel]).all(), (name, int(n))
    assert (acc.sample_counts()[slots[owned], 0] == slot_n[owned]).all()
    assert_bit_identical(acc.image()[slots[owned]], F.mean(final.sums, final.kept)[owned], "image with per-pixel kept")
    assert_bit_identical(acc.clamp_loss()[slots[owned]], K.loss_mean(final.lost, final.kept)[owned], "loss")
    acc.release()


# ---- 5. checkpoint and refusals ---------------------------------------------------------------------------------
def test_checkpoint_resume(worlds, tmp_path):
    world = worlds("cornell_box")
    whole = R.Accumulator(world, SIZE, DEPTH, seed=SEED, moments=True, clamp=1.0)
    whole.add(8)
    path = tmp_path / "clamp.npz"
    whole.state().save(path)
    whole.add(8)
    state = AccumState.load(path)
    assert state.flags == 13 and state.samples == 8 and state.clamp == 1.0 and (state.clamped > 0).sum() >= 20
    fresh = R.Accumulator(R.DeviceWorld(world, 0), SIZE, DEPTH, seed=SEED, moments=True, clamp=1.0)
    fresh.load_state(state)
    same_state(fresh.state(), state, "loaded")
    fresh.add(8)
    same_state(fresh.state(), whole.state(), "resumed")
    assert_bit_identical(fresh.image(), whole.image(), "resumed image")
    assert_bit_identical(fresh.clamp_loss(), whole.clamp_loss(), "resumed loss")
    other = R.Accumulator(fresh.dworld, SIZE, DEPTH, seed=SEED, moments=True, clamp=0.5)
    with pytest.raises(N.RtwError) as e:  # a different level
        other.load_state(state)
    assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT and "clamp" in str(e.value)


def test_refusals(worlds):
    world = worlds("simple_plane")
    size = R.Size2i(20, 12)  # 3 x 2 tiles, padded in both axes
    dw = R.DeviceWorld(world, 0)
    L = N.lib()
    p = R.render_params(size, 0, DEPTH, seed=SEED)
    h = C.c_void_p()

    def refused(rc, word):
        assert rc == N.RTW_ERR_INVALID_ARGUMENT
        assert word in L.rtw_last_error().decode(), L.rtw_last_error()

    # rtw_accum_create given the flag; a bad level; the flag without FINITE
    refused(L.rtw_accum_create(dw._h, C.byref(p), N.ACCUM_FINITE | N.ACCUM_CLAMP, C.byref(h)), "RTW_ACCUM_CLAMP")
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        refused(L.rtw_accum_create_clamp(dw._h, C.byref(p), N.ACCUM_FINITE | N.ACCUM_CLAMP, bad, C.byref(h)), "clamp")
    refused(L.rtw_accum_create_clamp(dw._h, C.byref(p), N.ACCUM_CLAMP | N.ACCUM_MOMENTS, 1.0, C.byref(h)), "RTW_ACCUM_FINITE")
    assert "RTW_ACCUM_CLAMP" in L.rtw_last_error().decode()
    refused(L.rtw_accum_create_clamp(dw._h, C.byref(p), N.ACCUM_FINITE, 1.0, C.byref(h)), "RTW_ACCUM_CLAMP")
    cl = R.Accumulator(dw, size, DEPTH, seed=SEED, moments=True, clamp=0.25)
    fin = R.Accumulator(dw, size, DEPTH, seed=SEED, moments=True, finite=True)
    for acc in (cl, fin):
        acc.add(4)
    st, info = cl.state(), cl.info()
    s, q, k = st.sums.ctypes.data_as(f32p), st.squares.ctypes.data_as(f32p), st.kept.ctypes.data_as(u32p)
    c, l = st.clamped.ctypes.data_as(u32p), st.lost.ctypes.data_as(f32p)
    t = np.zeros(cl.tiles, np.uint32).ctypes.data_as(u32p)
    # the three older pairs refuse a clamp accumulator by name
    refused(L.rtw_accum_export(cl._h, s, q), "RTW_ACCUM_CLAMP")
    refused(L.rtw_accum_import(cl._h, C.byref(info), s, q), "RTW_ACCUM_CLAMP")
    refused(L.rtw_accum_export_adaptive(cl._h, s, q, t), "RTW_ACCUM_CLAMP")
    refused(L.rtw_accum_import_adaptive(cl._h, C.byref(info), s, q, t), "RTW_ACCUM_CLAMP")
    refused(L.rtw_accum_export_state(cl._h, s, q, None, k), "RTW_ACCUM_CLAMP")
    refused(L.rtw_accum_import_state(cl._h, C.byref(info), s, q, None, k), "RTW_ACCUM_CLAMP")
    # the clamp pair: the same pointer rule, and its own two arrays
    refused(L.rtw_accum_export_state_clamp(cl._h, s, q, None, k, None, l), "clamped")
    refused(L.rtw_accum_export_state_clamp(cl._h, s, q, None, k, c, None), "lost")
    refused(L.rtw_accum_export_state_clamp(cl._h, s, q, t, k, c, l), "tile_stop")
    refused(L.rtw_accum_export_state_clamp(cl._h, s, None, None, k, c, l), "squares")
    refused(L.rtw_accum_import_state_clamp(cl._h, C.byref(info), s, q, None, None, c, l), "kept")
    refused(L.rtw_accum_export_state_clamp(fin._h, s, q, None, k, c, l), "RTW_ACCUM_CLAMP")
    for fn in (fin.clamped_counts, fin.clamp_loss):
        with pytest.raises(N.RtwError) as e:
            fn()
        assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT and "RTW_ACCUM_CLAMP" in str(e.value)
    # clamped above kept, and something in a padding slot of clamped or lost
    slots = tile_slots(size, TILE, (0, 1))
    inside, pad = int(np.flatnonzero(slots >= 0)[5]), int(np.flatnonzero(slots < 0)[0])
    for name, slot, value in (("clamped", inside, 5), ("clamped", pad, 1), ("lost", pad, f32(1e-30))):
        bad = cl.state()
        getattr(bad, name)[slot] = value
        with pytest.raises(N.RtwError) as e:
            cl.load_state(bad)
        assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT and name in str(e.value), str(e.value)
    same_state(cl.state(), st, "a refused import changes nothing")
    ok = cl.state()
    ok.clamped[inside] = ok.kept[inside]  # at kept: taken
    cl.load_state(ok)
    assert (cl.state().clamped == ok.clamped).all() and cl.samples == 4
    dw.release()


# ---- 6. partitions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [(8, 8), (5, 3)], ids=["tile8x8", "tile5x3"])
def test_parts_packed_and_merged_equal_the_single_accumulator(worlds, tile):
    import torch

    world, size, n, level = worlds("cornell_box"), R.Size2i(50, 37), 3, 1.0
    dw = R.DeviceWorld(world, 0)
    kw = dict(seed=SEED, tile=tile, moments=True, clamp=level)
    single, whole = R.Accumulator(dw, size, DEPTH, **kw), R.Accumulator(dw, size, DEPTH, **kw)
    parts = [R.Accumulator(dw, size, DEPTH, part=(r, n), layout=N.LAYOUT_TILES, **kw) for r in range(n)]
    for acc in parts + [single]:
        acc.add(8)
    want = single.state()
    assert (want.clamped > 0).sum() >= 50
    for pad in (0, 4):  # 8 x 8 and an aligned stride: the 16-byte path; 5 x 3 or an odd stride: the dword path
        stride = parts[0].packed_bytes() + pad
        gathered = torch.full((n * stride // 4,), -1, dtype=torch.int32, device="cuda:0")
        for r, p in enumerate(parts):
            p.pack_into(gathered[r * stride // 4: (r + 1) * stride // 4])
        whole.merge_parts(gathered, stride, n)
        host = gathered.cpu().numpy().view(np.uint32).reshape(n, -1)
        for r, p in enumerate(parts):  # the records word for word, the level in the last header word
            assert (host[r][:stride // 4 - pad // 4] == p.state().packed()).all(), f"record {r}"
            assert host[r][7] == f32(level).view(np.uint32)
        same_state(whole.state(), want, f"merged state, pad {pad}")
        same_state(merge_parts_host(want, host, stride, n), want, f"the host twin, pad {pad}")
    assert (whole.clamped_counts() == single.clamped_counts()).all()
    assert_bit_identical(whole.clamp_loss(), single.clamp_loss(), "loss through the merge")
    assert_bit_identical(whole.image(), single.image(), "image through the merge")
    # a record of another level is refused, and nothing changes
    other = R.Accumulator(dw, size, DEPTH, part=(1, n), layout=N.LAYOUT_TILES, seed=SEED, tile=tile, moments=True, clamp=0.5)
    other.add(8)
    other.pack_into(gathered[stride // 4: 2 * stride // 4])
    with pytest.raises(N.RtwError) as e:
        whole.merge_parts(gathered, stride, n)
    assert "clamp" in str(e.value) and "record 1" in str(e.value)
    same_state(whole.state(), want, "after the refusal")
    dw.release()


SCENE7, SIZE7, LEVEL7 = "cornell_box", (40, 40), 1.0


def _free_port() -> int:
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def _rank(rank, world_size, port, out_dir):
    import sys

    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import torch.distributed as dist

    from raytracinginaweekend_amd.distributed import DistributedAccumulator

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world_size)
    try:
        acc = DistributedAccumulator(R.demo_world(SCENE7), R.Size2i(*SIZE7), DEPTH, rank, world_size, 0, seed=SEED,
                                     moments=True, clamp=LEVEL7)
        acc.add(4)
        acc.add(4)
        whole = acc.sync()
        assert (whole is None) == (rank != 0)
        if whole is not None:
            whole.state().save(os.path.join(out_dir, "whole.npz"))
            np.save(os.path.join(out_dir, "loss.npy"), whole.clamp_loss())
        dist.barrier()
        acc.release()
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu(worlds, tmp_path):
    import torch.multiprocessing as mp

    single = R.Accumulator(worlds(SCENE7), R.Size2i(*SIZE7), DEPTH, seed=SEED, moments=True, clamp=LEVEL7)
    single.add(8)
    want, want_loss = single.state(), single.clamp_loss()
    assert (want.clamped > 0).sum() >= 20
    ctx = mp.start_processes(_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn", join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):  # (raises when a child exits non-zero: no retry)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish in 120 s")
    same_state(AccumState.load(tmp_path / "whole.npz"), want, "the two ranks' merged state")
    assert_bit_identical(np.load(tmp_path / "loss.npy"), want_loss, "the two ranks' loss")
