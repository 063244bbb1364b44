"""The leaf-list kernel's camera batch (render_kernel_pl<.., true>): a wave prepares the camera
rays of 64 consecutive work items at once and its lanes pick the records up.  Every image stays bit-identical
to the oracle, to the same library with RTW_CAMERA_BATCH=0 and to RTW_PRIMARY_LISTS=0, and the park's counters
show every sample prepared once and picked up once (an item traced twice would not show in the image)."""
import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.distributed import pack_tiles
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

DEPTH = 50
SEED = 31


def _frame(dw, p):
    """One frame of `dw` with params `p` (image layout, or one partition's tile buffer)."""
    import torch

    n = R.rendering.partition_floats(p) if p.layout == N.LAYOUT_TILES else p.width * p.height * 3
    out = torch.zeros(n, dtype=torch.float32, device="cuda:0")
    dw.render_into(p, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def refs(worlds):
    """Oracle frames, computed once per (world, size, spp, thread_count)."""
    cache = {}

    def get(name, size, spp, threads=1):
        key = (name, size, spp, threads)
        if key not in cache:
            cache[key] = O.render(worlds(name), R.render_params(R.Size2i(*size), spp, DEPTH, seed=SEED, thread_count=threads))
        return cache[key]

    return get


def _real_pixels(size, tile, part):
    """Pixels of the frame that lie in the partition's tiles (tile t belongs to part t mod count)."""
    (w, h), (tw, th), (index, count) = size, tile, part
    tiles_x, tiles_y = -(-w // tw), -(-h // th)
    n = 0
    for t in range(index, tiles_x * tiles_y, count):
        tx, ty = t % tiles_x, t // tiles_x
        n += min(tw, w - tx * tw) * min(th, h - ty * th)
    return n


def _batched(monkeypatch, dw, p, samples):
    """A frame with the camera batch on: its name ends in `true>`, and the park stored and handed out exactly
    `samples` valid records.  Returns (frame, fills)."""
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    monkeypatch.delenv("RTW_CAMERA_BATCH", raising=False)
    dw.park_counts()
    on = _frame(dw, p)
    name = dw.kernel_variant()["name"]
    fills, stored, picked = dw.park_counts()
    print(name, "fills", fills, "stored", stored, "picked", picked, "samples", samples)
    assert name.startswith("render_kernel_pl<false, 1, 0, ") and name.endswith(", true>")
    assert stored == samples and picked == samples
    assert fills >= -(-samples // 64)
    return on, fills


def _three_ways(monkeypatch, dw, p, samples, lf=None):
    """(batched frame, the frame with RTW_CAMERA_BATCH=0, the frame with RTW_PRIMARY_LISTS=0); `lf`, when given,
    receives the batched frame's last_frame()."""
    on, _ = _batched(monkeypatch, dw, p, samples)
    if lf is not None:
        lf.update(dw.last_frame())
    monkeypatch.setenv("RTW_CAMERA_BATCH", "0")
    off = _frame(dw, p)
    name = dw.kernel_variant()["name"]
    assert name.startswith("render_kernel_pl<false, 1, 0, ") and name.endswith(", false>")
    assert dw.park_counts() == (0, 0, 0)
    monkeypatch.delenv("RTW_CAMERA_BATCH")
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "0")
    walk = _frame(dw, p)
    assert dw.kernel_variant()["name"].startswith("render_kernel<")
    assert dw.park_counts() == (0, 0, 0)
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    return on, off, walk


@pytest.mark.parametrize("cap", [None, 4], ids=["cap16", "cap4"])
@pytest.mark.parametrize("name", ["final_scene1", "defocus_blur"])
def test_whole_frames(worlds, refs, monkeypatch, name, cap):
    if cap is not None:  # "walk" tiles' PH_TRACE records beside resolved ones
        monkeypatch.setenv("RTW_PRIMARY_LIST_CAP", str(cap))
    dw = R.DeviceWorld(worlds(name), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED)
    lf = {}
    on, off, walk = _three_ways(monkeypatch, dw, p, 160 * 90 * 8, lf)
    if cap == 4 and name == "final_scene1":
        assert lf["tiles_walked"] > 0
    assert_bit_identical(on.reshape(-1, 3), refs(name, (160, 90), 8), f"{name} against the oracle")
    assert_bit_identical(on, off, f"{name} batch on / off")
    assert_bit_identical(on, walk, f"{name} batch / no lists")
    dw.release()


@pytest.mark.parametrize("tile", [(8, 8), (16, 4)], ids=["8x8", "16x4"])
@pytest.mark.parametrize("name", ["final_scene1", "defocus_blur"])
def test_edge_tiles_and_partitions(worlds, refs, monkeypatch, name, tile):
    """Padding slots fall inside fills, and the partition's runs are not 64-aligned."""
    dw = R.DeviceWorld(worlds(name), 0)
    size = R.Size2i(50, 37)
    p = R.render_params(size, 8, DEPTH, seed=SEED, tile=tile, part=(1, 3), layout=N.LAYOUT_TILES)
    on, off, walk = _three_ways(monkeypatch, dw, p, _real_pixels((50, 37), tile, (1, 3)) * 8)
    assert_bit_identical(on, pack_tiles(refs(name, (50, 37), 8), size, tile, (1, 3), len(on)), f"{name} partition 1 of 3")
    assert_bit_identical(on, off, f"{name} partition, batch on / off")
    assert_bit_identical(on, walk, f"{name} partition, batch / no lists")
    dw.release()


@pytest.mark.parametrize("shape", [(9, 5, 1, (8, 8)), (8, 8, 3, (2, 2))], ids=["9x5x1", "8x8x3"])
def test_small_frames(worlds, refs, monkeypatch, shape):
    """9x5x1 is 45 samples in padded tiles: partial fills, and most waves get none.  (A tile of so small a frame
    sees most of the scene: the cap is lifted to the leaf count, or every tile would walk and the frame would
    take the kernel without lists.  8x8x3 in 2x2 tiles: one 8x8 tile spans the whole field of view, too wide a
    beam for a list, and a fill then holds 16 tiles.)"""
    monkeypatch.setenv("RTW_PRIMARY_LIST_CAP", "65536")
    w, h, spp, tile = shape
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(w, h), spp, DEPTH, seed=SEED, tile=tile)
    on, off, walk = _three_ways(monkeypatch, dw, p, w * h * spp)
    assert_bit_identical(on.reshape(-1, 3), refs("final_scene1", (w, h), spp), "small frame against the oracle")
    assert_bit_identical(on, off, "small frame, batch on / off")
    assert_bit_identical(on, walk, "small frame, batch / no lists")
    dw.release()


def test_several_launches_per_frame(worlds, refs, monkeypatch):
    """A colour buffer of 3 samples: 3 launches, each starting on an empty park; the counters hold summed."""
    slots = 20 * 12 * 64
    monkeypatch.setenv("RTW_SAMPLE_BUFFER_BYTES", str(slots * 3 * 4 * 3))
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED)
    lf = {}
    on, off, walk = _three_ways(monkeypatch, dw, p, 160 * 90 * 8, lf)
    assert lf["launches"] == 3
    assert_bit_identical(on.reshape(-1, 3), refs("final_scene1", (160, 90), 8), "3 launches against the oracle")
    assert_bit_identical(on, off, "3 launches, batch on / off")
    assert_bit_identical(on, walk, "3 launches, batch / no lists")
    dw.release()


def test_both_work_orders(worlds, refs, monkeypatch):
    """The first frame of a shape runs chunk-major, the second in cost order (tile_perm)."""
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED)
    ref = refs("final_scene1", (160, 90), 8)
    first, _ = _batched(monkeypatch, dw, p, 160 * 90 * 8)
    second, _ = _batched(monkeypatch, dw, p, 160 * 90 * 8)
    assert_bit_identical(first.reshape(-1, 3), ref, "chunk-major order")
    assert_bit_identical(second.reshape(-1, 3), ref, "cost order")
    dw.release()


@pytest.mark.parametrize("name", ["final_scene1", "defocus_blur"])
def test_accumulator_adds(worlds, refs, monkeypatch, name):
    """add(3) then add(5): the second launch starts at sample 3; the counters hold per launch."""
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    acc = R.Accumulator(worlds(name), R.Size2i(160, 90), DEPTH, seed=SEED)
    acc.dworld.park_counts()
    for n in (3, 5):
        acc.add(n)
        _, stored, picked = acc.dworld.park_counts()
        assert stored == picked == 160 * 90 * n
        assert acc.dworld.kernel_variant()["name"].endswith(", true>")
    assert_bit_identical(acc.image(), refs(name, (160, 90), 8), f"{name} 3 + 5 samples")
    acc.release()


def test_thread_count_three(worlds, refs, monkeypatch):
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED, thread_count=3)
    on, off, walk = _three_ways(monkeypatch, dw, p, 160 * 90 * 8)
    assert_bit_identical(on.reshape(-1, 3), refs("final_scene1", (160, 90), 8, 3), "thread_count 3")
    assert_bit_identical(on, off, "thread_count 3, batch on / off")
    assert_bit_identical(on, walk, "thread_count 3, batch / no lists")
    dw.release()


def test_tuner_keeps_the_kernel_without_the_batch(worlds, refs, monkeypatch):
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    monkeypatch.setenv("RTW_TUNE_SPHERES", "1")
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED)
    dw.park_counts()
    img = _frame(dw, p)
    name = dw.kernel_variant()["name"]
    assert name.startswith("render_kernel_pl<false, 1, 0, ") and name.endswith(", false>")
    assert dw.park_counts() == (0, 0, 0)
    assert_bit_identical(img.reshape(-1, 3), refs("final_scene1", (160, 90), 8), "tuner fallback")
    dw.release()


def test_world_out_of_scope(worlds, monkeypatch):
    """A mesh world runs render_kernel<...> under its six-place name, and the park is never touched."""
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    dw = R.DeviceWorld(worlds("cornell_cube"), 0)
    p = R.render_params(R.Size2i(64, 64), 4, DEPTH, seed=SEED)
    dw.park_counts()
    _frame(dw, p)
    name = dw.kernel_variant()["name"]
    assert name.startswith("render_kernel<false, ") and name.count(",") == 5
    assert dw.park_counts() == (0, 0, 0)
    dw.release()
