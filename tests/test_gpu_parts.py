"""Accumulators across partitions on the device (rtw_accum_pack, rtw_accum_merge_parts, distributed.py;
DESIGN.md 5.5h).

The contract: N partition accumulators, packed, gathered and merged, are bit for bit the accumulator one GPU
holds after the same calls -- sums, squares, kept, stop map, header and the zeros of the padding slots -- so
everything read from the merged accumulator (image, standard error, noise, counts, denoised preview, checkpoint)
and every later add is the single accumulator's.  The shapes are the smallest with edge tiles in both axes, several
tiles per part and both copy paths: the (8, 8) tile takes the 16-byte path, (5, 3) and an odd stride the dword
path."""
import functools
import os
import socket
import time

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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 31
f32 = np.float32


def same_state(a: AccumState, b: AccumState, what="") -> None:
    assert a.header() == b.header(), what
    for name in ("sums", "squares", "tile_stop", "kept"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.shape == y.shape and (x.view(np.uint32) == y.view(np.uint32)).all(), (what, name)


def make_parts(dw, size, depth, n, tile, **flags):
    return [R.Accumulator(dw, size, depth, seed=SEED, tile=tile, part=(r, n), layout=N.LAYOUT_TILES, **flags) for r in range(n)]


def pack_and_merge(parts, whole, pad_bytes=0, side_stream=False):
    """Packs every part into one gathered device buffer and merges it into `whole`; returns (gathered, stride).
    side_stream: the packs run on a stream of their own and the merge, on the current one, is not told."""
    import torch

    n = len(parts)
    stride = parts[0].packed_bytes() + pad_bytes
    assert all(p.packed_bytes() == parts[0].packed_bytes() for p in parts) and stride % 4 == 0
    gathered = torch.full((n * stride // 4,), -1, dtype=torch.int32, device=torch.device("cuda", whole.device))
    pack_stream = None
    if side_stream:
        side = torch.cuda.Stream(device=whole.device)
        side.wait_stream(torch.cuda.current_stream(whole.device))  # (the buffer's fill)
        pack_stream = side.cuda_stream
    for r, p in enumerate(parts):
        p.pack_into(gathered[r * stride // 4: (r + 1) * stride // 4], pack_stream)
    whole.merge_parts(gathered, stride, n)
    return gathered, stride


@functools.lru_cache(maxsize=None)
def oracle_frame(getter, name, w, h, spp, depth):
    return O.render(getter(name), R.render_params(R.Size2i(w, h), spp, depth, seed=SEED))


# ---- 1. merge equals single -------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [(8, 8), (5, 3)], ids=["tile8x8", "tile5x3"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_merge_equals_the_single_accumulator(worlds, moments, n, tile):
    world, size, depth = worlds("final_scene1"), R.Size2i(44, 26), 50  # 5.5 x 3.25 tiles of 8 x 8
    dw = R.DeviceWorld(world, 0)
    single = R.Accumulator(dw, size, depth, seed=SEED, tile=tile, moments=moments)
    whole = R.Accumulator(dw, size, depth, seed=SEED, tile=tile, moments=moments)
    parts = make_parts(dw, size, depth, n, tile, moments=moments)
    for k in (3, 5):
        for acc in parts + [single]:
            acc.add(k)
    gathered, stride = pack_and_merge(parts, whole)
    # the records themselves: numpy's packing of the parts' exported states, word for word
    host = gathered.cpu().numpy().view(np.uint32).reshape(n, -1)
    for r, p in enumerate(parts):
        assert (host[r] == p.state().packed(stride)).all(), f"record {r}"
    st = whole.state()
    same_state(st, single.state(), "merged state")
    owned = tile_slots(size, tile, (0, 1)) >= 0
    assert (~owned).any() and (st.sums.view(np.uint32)[~owned] == 0).all()
    assert whole.samples == 8
    assert_bit_identical(whole.image(), oracle_frame(worlds, "final_scene1", 44, 26, 8, 50), "merged image")
    if moments:
        assert (st.squares.view(np.uint32)[~owned] == 0).all()
        assert_bit_identical(whole.stderr(), single.stderr(), "standard error")
        assert whole.noise() == single.noise()
    if tile == (8, 8) and n == 3:  # an odd stride: the dword path on the 8 x 8 tile, the same bits
        again = R.Accumulator(dw, size, depth, seed=SEED, tile=tile, moments=moments)
        pack_and_merge(parts, again, pad_bytes=4)
        same_state(again.state(), st, "odd stride")
        # packs on another stream: the merge waits for them through the world's event, as every accumulator call
        pack_and_merge(parts, again, side_stream=True)
        same_state(again.state(), st, "packs on a side stream")
    dw.release()


# ---- 2. finite --------------------------------------------------------------------------------------------
def test_merge_carries_the_kept_counts(worlds):
    world, size, depth, n = worlds("suzanne"), R.Size2i(64, 36), 10, 3
    dw = R.DeviceWorld(world, 0)
    kw = dict(moments=True, finite=True)
    single = R.Accumulator(dw, size, depth, seed=SEED, **kw)
    whole = R.Accumulator(dw, size, depth, seed=SEED, **kw)
    parts = make_parts(dw, size, depth, n, (8, 8), **kw)
    for acc in parts + [single]:
        acc.add(8)
    pack_and_merge(parts, whole)
    rejected = single.rejected_counts()
    print("pixels with a rejected sample:", int((rejected > 0).sum()))
    assert (rejected > 0).sum() >= 10
    same_state(whole.state(), single.state(), "finite state")
    assert (whole.kept_counts() == single.kept_counts()).all() and (whole.rejected_counts() == rejected).all()
    assert_bit_identical(whole.image(), single.image(), "finite image")
    assert whole.noise() == single.noise()
    dw.release()


# ---- 3. adaptive ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("huge_target", [False, True], ids=["median_target", "target_1e30"])
def test_adaptive_parts_take_the_single_decisions(worlds, huge_target):
    world, size, depth, n, tile = worlds("final_scene1"), R.Size2i(50, 37), 10, 3, (8, 8)
    MIN, BATCH, MAX = 8, 4, 32
    dw = R.DeviceWorld(world, 0)
    if huge_target:
        target = 1e30
    else:  # the median tile error at 8 samples, as test_gpu_adaptive.py derives it
        probe = R.Accumulator(dw, size, depth, seed=SEED, moments=True)
        probe.add(MIN)
        st = probe.state()
        target = float(f32(np.median(A.tiles_E(st.sums, st.squares, MIN, size, tile, (0, 1)))))
        probe.release()
    single = R.Accumulator(dw, size, depth, seed=SEED, adaptive=True)
    parts = make_parts(dw, size, depth, n, tile, adaptive=True)
    frame_tiles = single.tiles
    active_seen, frontier, group_active = [], 0, frame_tiles
    for _ in range(MAX // BATCH):
        single.add(BATCH)
        if group_active > 0:  # (the wrapper's rule: a group without an active tile no longer counts)
            frontier += BATCH
        for p in parts:
            p.add(BATCH)
        assert single.samples == frontier
        if frontier < MIN:
            continue
        want_active = single.adapt(target, MIN)
        got = [p.adapt(target, MIN) for p in parts]
        group_active = sum(t for t, _ in got)
        assert (group_active, sum(px for _, px in got)) == want_active
        stops = np.zeros(frame_tiles, np.uint32)
        for r, p in enumerate(parts):
            stops[r::n] = p.tile_stops()
        assert (stops == single.tile_stops()).all(), frontier
        active_seen.append(want_active[0])
    final = single.tile_stops()
    print("target", target, "stops", dict(zip(*np.unique(final, return_counts=True))), "active", active_seen)
    if huge_target:
        assert (final == MIN).all() and single.samples == MIN and all(p.samples == MIN for p in parts)
    else:  # else the frontier rule is not exercised
        assert len(np.unique(final[final != 0])) >= 2 and max(active_seen) >= 1
    whole = R.Accumulator(dw, size, depth, seed=SEED, adaptive=True)
    pack_and_merge(parts, whole)
    assert whole.samples == single.samples
    assert (whole.tile_stops() == final).all()
    assert (whole.sample_counts() == single.sample_counts()).all()
    same_state(whole.state(), single.state(), "adaptive state")
    # the merged accumulator goes on as the single one does (its host copy of the stop map is current)
    assert whole.adapt(target, MIN) == single.adapt(target, MIN)
    whole.add(BATCH)
    single.add(BATCH)
    same_state(whole.state(), single.state(), "after one more add")
    dw.release()


# ---- 3b. every section of the colour record in one launch -----------------------------------------------------
def test_mixed_section_widths_and_an_unaligned_gather(worlds):
    """moments + finite + adaptive on the 8 x 8 tile, N = 3: sums, squares and kept go as 16-byte units beside the
    dword stop map in one pack and one merge launch.  The same parts packed into a view one word off 16 bytes and
    merged at a stride of 4 mod 16 take the dword path for every section: the same bits."""
    import torch

    world, size, depth, n, tile = worlds("final_scene1"), R.Size2i(44, 26), 10, 3, (8, 8)
    kw = dict(moments=True, finite=True, adaptive=True)
    dw = R.DeviceWorld(world, 0)
    single = R.Accumulator(dw, size, depth, seed=SEED, **kw)
    parts = make_parts(dw, size, depth, n, tile, **kw)
    for acc in parts + [single]:
        acc.add(8)
    st = single.state()
    target = float(f32(np.median(F.tiles_E(st.sums, st.squares, st.kept, size, tile, (0, 1)))))
    for acc in parts + [single]:
        acc.adapt(target, 8)
        acc.add(4)
    want = single.state()
    assert (want.tile_stop == 8).any() and (want.tile_stop == 0).any()  # stopped and active tiles cross the merge
    whole = R.Accumulator(dw, size, depth, seed=SEED, **kw)
    pack_and_merge(parts, whole)
    aligned = whole.state()
    same_state(aligned, want, "16-byte sections beside the dword stop map")
    assert (whole.kept_counts() == single.kept_counts()).all() and whole.samples == single.samples
    # one word off, and a stride that is a multiple of 4 but not of 16
    stride = parts[0].packed_bytes() + 4
    assert parts[0].packed_bytes() % 16 == 0 and stride % 16 == 4
    buf = torch.full((1 + n * stride // 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    gathered = buf[1:]
    assert gathered.data_ptr() % 16 == 4
    for r, p in enumerate(parts):
        p.pack_into(gathered[r * stride // 4: (r + 1) * stride // 4])
    again = R.Accumulator(dw, size, depth, seed=SEED, **kw)
    again.merge_parts(gathered, stride, n)
    same_state(again.state(), aligned, "unaligned gather")
    host = buf.cpu().numpy().view(np.uint32)
    assert host[0] == 0x5A5A5A5A
    for r, p in enumerate(parts):  # the records word for word, and the word between them untouched
        assert (host[1 + r * stride // 4: 1 + (r + 1) * stride // 4] == np.append(p.state().packed(), np.uint32(0x5A5A5A5A))).all(), r
    dw.release()


def test_more_parts_than_tiles(worlds):
    """26 parts of the 24 tiles of 44 x 26: parts 24 and 25 pack a header and zeros, and the merge is the single
    accumulator."""
    world, size, depth, n, tile = worlds("final_scene1"), R.Size2i(44, 26), 5, 26, (8, 8)
    kw = dict(moments=True, finite=True, adaptive=True)
    dw = R.DeviceWorld(world, 0)
    single = R.Accumulator(dw, size, depth, seed=SEED, **kw)
    parts = make_parts(dw, size, depth, n, tile, **kw)
    assert [p.tiles for p in parts] == [1] * 24 + [0] * 2
    for acc in parts + [single]:
        acc.add(3)
    whole = R.Accumulator(dw, size, depth, seed=SEED, **kw)
    gathered, stride = pack_and_merge(parts, whole)
    host = gathered.cpu().numpy().view(np.uint32).reshape(n, -1)
    for r in (24, 25):
        assert tuple(host[r][:4]) == (1, single.state().flags, r, n) and tuple(host[r][5:8]) == (0, 0, 0)
        assert (host[r][8:] == 0).all()
    same_state(whole.state(), single.state(), "26 parts of 24 tiles")
    dw.release()


# ---- 4. continue and re-partition; 5. denoise through the merge ---------------------------------------------
def test_continue_repartition_and_denoise(worlds):
    world, size, depth, tile = worlds("final_scene1"), R.Size2i(44, 26), 50, (8, 8)
    dw = R.DeviceWorld(world, 0)
    single = R.Accumulator(dw, size, depth, seed=SEED, moments=True)
    whole = R.Accumulator(dw, size, depth, seed=SEED, moments=True)
    three = make_parts(dw, size, depth, 3, tile, moments=True)
    for k in (3, 5):
        for acc in three + [single]:
            acc.add(k)
    pack_and_merge(three, whole)
    at8 = whole.state()
    same_state(at8, single.state(), "at 8")
    whole.add(4)
    single.add(4)
    want = single.state()
    same_state(whole.state(), want, "the merged accumulator continues the frame")
    # N = 3 -> M = 2: the checkpoint at 8 samples, split for two ranks, loaded, continued, merged again
    two = make_parts(dw, size, depth, 2, tile, moments=True)
    for acc, st in zip(two, at8.split(2)):
        acc.load_state(st)
        acc.add(4)
    again = R.Accumulator(dw, size, depth, seed=SEED, moments=True)
    pack_and_merge(two, again)
    same_state(again.state(), want, "re-partitioned 3 -> 2")
    assert_bit_identical(again.image(), oracle_frame(worlds, "final_scene1", 44, 26, 12, 50), "12 spp")
    # 5. the preview of the merged accumulator at 12 spp
    assert_bit_identical(whole.denoised(), single.denoised(), "denoised through the merge")
    dw.release()


# ---- 6. refusals -------------------------------------------------------------------------------------------
def test_device_path_refusals_launch_nothing(worlds):
    import torch

    world, size, depth, tile, n = worlds("final_scene1"), R.Size2i(44, 26), 5, (8, 8), 2
    dw = R.DeviceWorld(world, 0)
    whole = R.Accumulator(dw, size, depth, seed=SEED, moments=True)
    whole.add(2)
    before = whole.state()
    parts = make_parts(dw, size, depth, n, tile, moments=True)
    plain = make_parts(dw, size, depth, n, tile)
    for acc in parts + plain:
        acc.add(3)
    stride = parts[0].packed_bytes()
    words = stride // 4
    good = torch.zeros(n * words, dtype=torch.int32, device="cuda:0")
    other_flags = torch.zeros(n * words, dtype=torch.int32, device="cuda:0")
    for r in range(n):
        parts[r].pack_into(good[r * words: (r + 1) * words])
        plain[r].pack_into(other_flags[r * words: (r + 1) * words])  # (a smaller record inside the same stride)
    swapped = torch.cat([good[words:], good[:words]])

    def refused(field, call):
        with pytest.raises(N.RtwError) as e:
            call()
        assert field in str(e.value), str(e.value)
        same_state(whole.state(), before, f"after the refusal of {field}")

    refused("part_index", lambda: parts[1].merge_parts(good, stride, n))  # a whole with part != (0, 1)
    refused("flags", lambda: whole.merge_parts(other_flags, stride, n))
    refused("stride_bytes", lambda: whole.merge_parts(good, stride - 4, n))
    twice = torch.cat([good, good])
    refused("stride_bytes", lambda: whole.merge_parts(twice, stride + 2, n))
    refused("part_index", lambda: whole.merge_parts(swapped, stride, n))  # records in the wrong order
    refused("part_count", lambda: whole.merge_parts(twice, stride, 2 * n))
    uneven = good.clone()
    uneven[words + 4] += 1  # record 1's samples
    refused("samples", lambda: whole.merge_parts(uneven, stride, n))
    with pytest.raises(ValueError):
        whole.merge_parts(good[:-8], stride, n)  # fewer bytes than the records
    whole.merge_parts(good, stride, n)  # and the good buffer is taken
    assert whole.samples == 3
    dw.release()  # a released world: the device state is gone, nothing may be launched
    for call in (lambda: whole.merge_parts(good, stride, n), lambda: parts[0].pack_into(good[:words])):
        with pytest.raises(N.RtwError) as e:
            call()
        assert "world was released" in str(e.value)


# ---- 7. two ranks, one GPU ------------------------------------------------------------------------------------
SCENE7, SIZE7, DEPTH7, MIN7, BATCH7, MAX7 = "cornell_box", (40, 40), 10, 8, 4, 16


def _free_port() -> int:
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def _rank(rank, world_size, port, out_dir, target):
    import sys

    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import torch.distributed as dist

    from raytracinginaweekend_amd.distributed import DistributedAccumulator

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world_size)
    try:
        acc = DistributedAccumulator(R.demo_world(SCENE7), R.Size2i(*SIZE7), DEPTH7, rank, world_size, 0, seed=SEED,
                                     adaptive=True, finite=True)
        while acc.samples < MAX7 and acc.active_tiles > 0:
            acc.add(BATCH7)
            if acc.samples >= MIN7:
                acc.adapt(target, MIN7)
        whole = acc.sync()
        assert (whole is None) == (rank != 0)
        if whole is not None:
            whole.state().save(os.path.join(out_dir, "whole.npz"))
            np.save(os.path.join(out_dir, "image.npy"), whole.image())
        dist.barrier()
        acc.release()
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu(worlds, tmp_path):
    import torch.multiprocessing as mp

    world, size = worlds(SCENE7), R.Size2i(*SIZE7)
    single = R.Accumulator(world, size, DEPTH7, seed=SEED, adaptive=True, finite=True)
    target, stops_seen = None, []
    while single.samples < MAX7 and (single.tile_stops() == 0).any():
        single.add(BATCH7)
        if single.samples < MIN7:
            continue
        if target is None:  # the median tile error at 8 samples
            st = single.state()
            target = float(f32(np.median(F.tiles_E(st.sums, st.squares, st.kept, size, (8, 8), (0, 1)))))
        stops_seen.append(single.adapt(target, MIN7)[0])
    want, want_image = single.state(), single.image()
    print("target", target, "active tiles after each adapt", stops_seen, "samples", want.samples)
    assert (want.tile_stop != 0).any()  # stopped tiles cross the gather
    ctx = mp.start_processes(_rank, args=(2, _free_port(), str(tmp_path), target), nprocs=2, start_method="spawn", join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):  # (raises when a child exits non-zero: no retry)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish in 120 s")
    same_state(AccumState.load(tmp_path / "whole.npz"), want, "the two ranks' merged state")
    assert_bit_identical(np.load(tmp_path / "image.npy"), want_image, "the two ranks' image")
