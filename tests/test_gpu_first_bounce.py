"""The camera batch's first bounce (render_kernel_pl<.., true, true>): the fill shades the listed
camera hits with all its lanes, finishes the samples that end there and parks the others' bounce rays.  Every
frame stays bit-identical to the oracle, to the same library with RTW_FIRST_BOUNCE=0 and with
RTW_CAMERA_BATCH=0, and the counters show every sample prepared once and leaving the fill once:
finished + bounce + unsolved == stored == picked == samples."""
import ctypes as C

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.distributed import pack_tiles
from tests import variant_worlds as V
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

DEPTH = 50
SEED = 31
FB_NAME = "render_kernel_pl<false, 1, 0, 0, false, false, true, true>"
CB_NAME = "render_kernel_pl<false, 1, 0, 0, false, false, true>"


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
    """Oracle frames, computed once per (world, size, spp, depth, mode)."""
    cache = {}

    def get(name, size, spp, depth=DEPTH, mode=R.RenderMode.Default):
        key = (name, size, spp, depth, int(mode))
        if key not in cache:
            cache[key] = O.render(worlds(name), R.render_params(R.Size2i(*size), spp, depth, mode, seed=SEED))
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


def _on(monkeypatch, dw, p, samples, name=FB_NAME):
    """A frame with the first bounce on: the kernel's name first, then the counters.  Returns (frame,
    (finished, bounce, unsolved))."""
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    monkeypatch.delenv("RTW_CAMERA_BATCH", raising=False)
    monkeypatch.delenv("RTW_FIRST_BOUNCE", raising=False)
    dw.park_counts()
    dw.fill_counts()
    on = _frame(dw, p)
    assert dw.kernel_variant()["name"] == name
    fills, stored, picked = dw.park_counts()
    finished, bounce, unsolved = dw.fill_counts()
    print(name, "fills", fills, "stored", stored, "picked", picked, "finished", finished, "bounce", bounce, "unsolved",
          unsolved, "samples", samples)
    assert stored == samples and picked == samples
    if name == FB_NAME:
        assert finished + bounce + unsolved == samples
    else:
        assert (finished, bounce, unsolved) == (0, 0, 0)
    return on, (finished, bounce, unsolved)


def _three_ways(monkeypatch, dw, p, samples, name=FB_NAME):
    """(first-bounce frame, its fill counts, the frame with RTW_FIRST_BOUNCE=0, the frame with
    RTW_CAMERA_BATCH=0)."""
    on, counts = _on(monkeypatch, dw, p, samples, name)
    monkeypatch.setenv("RTW_FIRST_BOUNCE", "0")
    r14 = _frame(dw, p)
    kname = dw.kernel_variant()["name"]
    assert kname.startswith("render_kernel_pl<false, 1, 0, ") and kname.endswith(", false, true>") and kname.count(",") == 6
    _, stored, picked = dw.park_counts()
    assert stored == samples and picked == samples
    assert dw.fill_counts() == (0, 0, 0)
    monkeypatch.delenv("RTW_FIRST_BOUNCE")
    monkeypatch.setenv("RTW_CAMERA_BATCH", "0")
    off = _frame(dw, p)
    kname = dw.kernel_variant()["name"]
    assert kname.startswith("render_kernel_pl<false, 1, 0, ") and kname.endswith(", false>")
    assert dw.park_counts() == (0, 0, 0) and dw.fill_counts() == (0, 0, 0)
    monkeypatch.delenv("RTW_CAMERA_BATCH")
    return on, counts, r14, off


def _same(on, r14, off, ref, what):
    assert_bit_identical(on.reshape(ref.shape), ref, f"{what} against the oracle")
    assert_bit_identical(on, r14, f"{what}, first bounce on / off")
    assert_bit_identical(on, off, f"{what}, first bounce / no batch")


@pytest.mark.parametrize("cap", [None, 4], ids=["cap16", "cap4"])
@pytest.mark.parametrize("name", ["final_scene1", "defocus_blur"])
def test_whole_frames(worlds, refs, monkeypatch, name, cap):
    """Sky samples finish in the fill, hits park bounce records; under a cap of 4 the "walk" tiles' camera rays
    are parked unsolved."""
    if cap is not None:
        monkeypatch.setenv("RTW_PRIMARY_LIST_CAP", str(cap))
    dw = R.DeviceWorld(worlds(name), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED)
    on, (finished, bounce, unsolved), r14, off = _three_ways(monkeypatch, dw, p, 160 * 90 * 8)
    assert finished > 0 and bounce > 0
    if cap == 4 and name == "final_scene1":
        assert unsolved > 0  # the walk tiles (test_gpu_camera_batch relies on tiles_walked > 0 here)
    _same(on, r14, off, refs(name, (160, 90), 8), name)
    dw.release()


def _listed_everywhere(world, p, cap):
    """The host builder's lists (rtw_primary_lists_host): True when no tile of the frame takes the walk."""
    tw, th = p.tile_width or 8, p.tile_height or 8
    n = -(-p.width // tw) * -(-p.height // th)
    count = np.zeros(n, np.int32)
    lst = np.zeros((n, cap), np.int32)
    i32p = C.POINTER(C.c_int32)
    N.check(N.lib().rtw_primary_lists_host(world.ptr(), C.byref(p), cap, count.ctypes.data_as(i32p), lst.ctypes.data_as(i32p)))
    return bool((count >= 0).all())


def test_every_material_kind_is_a_first_hit(monkeypatch):
    """Lambert, fuzzed metal, dielectric and an emitting sphere as camera hits: each of shade()'s branches runs
    in the fill."""
    world = V.variant_world(0, 0)
    w, h, spp = 96, 54, 4
    raw = world.raw
    seen = V.primary_materials(world, w, h)
    kinds = {raw.materials[m].kind for m in seen}
    assert kinds >= {N.MAT_LAMBERT, N.MAT_METAL, N.MAT_DIELECTRIC, N.MAT_DIFFUSE_LIGHT}, kinds
    assert any(raw.materials[m].kind == N.MAT_METAL and raw.materials[m].fuzz > 0.0 for m in seen)
    p = R.render_params(R.Size2i(w, h), spp, DEPTH, seed=SEED)
    cap = raw.leaf_count  # the cap lifted: every tile of this small world's frame is listed
    assert _listed_everywhere(world, p, cap)
    monkeypatch.setenv("RTW_PRIMARY_LIST_CAP", str(cap))
    dw = R.DeviceWorld(world, 0)
    on, (finished, bounce, unsolved), r14, off = _three_ways(monkeypatch, dw, p, w * h * spp)
    assert finished > 0 and bounce > 0
    ref = O.render(world, R.render_params(R.Size2i(w, h), spp, DEPTH, seed=SEED))
    _same(on, r14, off, ref, "variant world (0, 0)")
    dw.release()


@pytest.mark.parametrize("depth", [1, 2])
def test_shallow_paths(worlds, refs, monkeypatch, depth):
    """max_depth 1: every settled hit ends black in the fill, so nothing settled parks a bounce record."""
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(64, 36), 4, depth, seed=SEED)
    on, (finished, bounce, unsolved), r14, off = _three_ways(monkeypatch, dw, p, 64 * 36 * 4)
    assert finished > 0
    if depth == 1:
        assert bounce == 0
    else:
        assert bounce > 0
    _same(on, r14, off, refs("final_scene1", (64, 36), 4, depth), f"max_depth {depth}")
    dw.release()


def test_normals_mode(worlds, refs, monkeypatch):
    """Every settled sample ends in the fill (a normal colour or the background)."""
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(64, 36), 4, DEPTH, R.RenderMode.Normals, seed=SEED)
    on, (finished, bounce, unsolved), r14, off = _three_ways(monkeypatch, dw, p, 64 * 36 * 4)
    assert finished > 0 and bounce == 0
    _same(on, r14, off, refs("final_scene1", (64, 36), 4, DEPTH, R.RenderMode.Normals), "normals mode")
    dw.release()


def test_nothing_in_view(monkeypatch):
    """Two spheres behind the camera: every fill finishes all its samples and parks nothing, and the launch
    still ends."""
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(wb.new_obj_sphere(0.5, wb.material_lambert_solid((0.7, 0.3, 0.2))).translate((-1.0, 0.5, 12.0)))
    g.add(wb.new_obj_sphere(0.5, wb.material_metal_solid((0.8, 0.8, 0.8), 0.1)).translate((1.0, 0.5, 12.0)))
    cam = R.Camera.build().vertical_fov(40.0, 1.0).position((0.0, 1.0, 6.0)).look_at((0, 1, 0), (0.0, 1.0, 0.0)).build()
    world = g.build().finish(wb, R.BackgroundColor.sky(), cam)
    size, spp = R.Size2i(64, 64), 2
    p = R.render_params(size, spp, DEPTH, seed=SEED)
    ref = O.render(world, p)
    _, st = O.render(world, R.render_params(size, spp, DEPTH, seed=SEED), stats=True)
    assert st["material_reads"] == 0 and st["rays"] == st["samples"] == 64 * 64 * spp  # pure background
    dw = R.DeviceWorld(world, 0)
    on, (finished, bounce, unsolved), r14, off = _three_ways(monkeypatch, dw, p, 64 * 64 * spp)
    assert bounce == 0 and unsolved == 0 and finished == 64 * 64 * spp
    _same(on, r14, off, ref, "nothing in view")
    dw.release()


def test_partial_fill(worlds, refs, monkeypatch):
    """9x5x1 with the cap lifted: 45 samples in padded tiles, partial fills, most waves get none."""
    monkeypatch.setenv("RTW_PRIMARY_LIST_CAP", "65536")
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(9, 5), 1, DEPTH, seed=SEED)
    on, _, r14, off = _three_ways(monkeypatch, dw, p, 45)
    _same(on, r14, off, refs("final_scene1", (9, 5), 1), "9x5x1")
    dw.release()


@pytest.mark.parametrize("tile", [(8, 8), (16, 4)], ids=["8x8", "16x4"])
def test_edge_tiles_and_partitions(worlds, refs, monkeypatch, tile):
    """Padding slots fall inside fills, and the partition's runs are not 64-aligned."""
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    size = R.Size2i(50, 37)
    p = R.render_params(size, 8, DEPTH, seed=SEED, tile=tile, part=(1, 3), layout=N.LAYOUT_TILES)
    on, _, r14, off = _three_ways(monkeypatch, dw, p, _real_pixels((50, 37), tile, (1, 3)) * 8)
    ref = pack_tiles(refs("final_scene1", (50, 37), 8), size, tile, (1, 3), len(on))
    _same(on, r14, off, ref, "partition 1 of 3")
    dw.release()


def test_several_launches_per_frame(worlds, refs, monkeypatch):
    """A colour buffer of 3 samples: 3 launches, each starting on an empty park; the counters hold summed."""
    slots = 20 * 12 * 64
    monkeypatch.setenv("RTW_SAMPLE_BUFFER_BYTES", str(slots * 3 * 4 * 3))
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED)
    on, counts = _on(monkeypatch, dw, p, 160 * 90 * 8)
    assert dw.last_frame()["launches"] == 3
    assert_bit_identical(on.reshape(-1, 3), refs("final_scene1", (160, 90), 8), "3 launches against the oracle")
    dw.release()


def test_accumulator_adds(worlds, refs, monkeypatch):
    """add(3) then add(5): the second launch starts at sample 3; the counters hold per launch."""
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    acc = R.Accumulator(worlds("final_scene1"), R.Size2i(160, 90), DEPTH, seed=SEED)
    acc.dworld.park_counts()
    acc.dworld.fill_counts()
    for n in (3, 5):
        acc.add(n)
        assert acc.dworld.kernel_variant()["name"] == FB_NAME
        _, stored, picked = acc.dworld.park_counts()
        finished, bounce, unsolved = acc.dworld.fill_counts()
        assert finished + bounce + unsolved == stored == picked == 160 * 90 * n
        assert finished > 0 and bounce > 0
    assert_bit_identical(acc.image(), refs("final_scene1", (160, 90), 8), "3 + 5 samples")
    acc.release()


def test_both_work_orders(worlds, refs, monkeypatch):
    """The first frame of a shape runs chunk-major, the second in cost order (tile_perm)."""
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED)
    ref = refs("final_scene1", (160, 90), 8)
    first, c1 = _on(monkeypatch, dw, p, 160 * 90 * 8)
    second, c2 = _on(monkeypatch, dw, p, 160 * 90 * 8)
    assert c1 == c2  # what a fill does with a sample does not depend on the order
    assert_bit_identical(first.reshape(-1, 3), ref, "chunk-major order")
    assert_bit_identical(second.reshape(-1, 3), ref, "cost order")
    dw.release()


def test_textured_world_keeps_the_batch_kernel(worlds, refs, monkeypatch):
    """perlin_spheres runs the TX_ANY batch kernel, which has no first bounce: its seven-place name, its bits,
    and no fill counts."""
    dw = R.DeviceWorld(worlds("perlin_spheres"), 0)
    p = R.render_params(R.Size2i(64, 36), 4, DEPTH, seed=SEED)
    on, counts = _on(monkeypatch, dw, p, 64 * 36 * 4, name="render_kernel_pl<false, 1, 0, 1, false, false, true>")
    assert counts == (0, 0, 0)
    assert_bit_identical(on.reshape(-1, 3), refs("perlin_spheres", (64, 36), 4), "perlin_spheres against the oracle")
    dw.release()
