"""Primary rays resolved from per-tile leaf lists (include/rtw_beam.h, render_kernel_pl; DESIGN.md 5.2
step 5): the images stay bit-identical to the oracle and to the same library with RTW_PRIMARY_LISTS=0,
the device builds the host builder's lists exactly, and worlds out of scope keep the walk."""
import ctypes as C

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


def _on_off(monkeypatch, dw, p):
    """(frame with lists, its last_frame(), frame with RTW_PRIMARY_LISTS=0, its last_frame())."""
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    on = _frame(dw, p)
    lf_on = dw.last_frame()
    name_on = dw.kernel_variant()["name"]
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "0")
    off = _frame(dw, p)
    lf_off = dw.last_frame()
    assert lf_off["tiles_listed"] == 0 and lf_off["tiles_empty"] == 0 and lf_off["tiles_walked"] == 0
    assert dw.kernel_variant()["name"].startswith("render_kernel<")
    return on, lf_on, name_on, off


@pytest.mark.parametrize("cap", [None, 4], ids=["cap16", "cap4"])
@pytest.mark.parametrize("name", ["final_scene1", "defocus_blur"])
def test_whole_frame_parity(worlds, refs, monkeypatch, name, cap):
    if cap is not None:
        monkeypatch.setenv("RTW_PRIMARY_LIST_CAP", str(cap))
    dw = R.DeviceWorld(worlds(name), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED)
    on, lf, kname, off = _on_off(monkeypatch, dw, p)
    print(name, cap, lf, kname)
    assert kname.startswith("render_kernel_pl<false, 1, 0, ")
    assert lf["tiles_listed"] > 0
    assert lf["tiles_listed"] + lf["tiles_empty"] + lf["tiles_walked"] == 20 * 12
    if cap == 4 and name == "final_scene1":  # "walk" tiles beside listed ones in one frame
        assert lf["tiles_walked"] > 0
    assert_bit_identical(on.reshape(-1, 3), off.reshape(-1, 3), f"{name} lists on / off")
    assert_bit_identical(on.reshape(-1, 3), refs(name, (160, 90), 8), f"{name} against the oracle")
    dw.release()


@pytest.mark.parametrize("cap", [None, 4], ids=["cap16", "cap4"])
@pytest.mark.parametrize("name", ["final_scene1", "defocus_blur"])
def test_partition_with_edge_tiles(worlds, refs, monkeypatch, name, cap):
    if cap is not None:
        monkeypatch.setenv("RTW_PRIMARY_LIST_CAP", str(cap))
    dw = R.DeviceWorld(worlds(name), 0)
    size = R.Size2i(50, 37)
    p = R.render_params(size, 8, DEPTH, seed=SEED, part=(1, 3), layout=N.LAYOUT_TILES)
    on, lf, kname, off = _on_off(monkeypatch, dw, p)
    print(name, cap, lf, kname)
    assert_bit_identical(on, off, f"{name} partition 1 of 3, lists on / off")
    assert_bit_identical(on, pack_tiles(refs(name, (50, 37), 8), size, (8, 8), (1, 3), len(on)), f"{name} partition 1 of 3")
    dw.release()


@pytest.mark.parametrize("name", ["final_scene1", "defocus_blur"])
def test_thread_count_three(worlds, refs, monkeypatch, name):
    dw = R.DeviceWorld(worlds(name), 0)
    p = R.render_params(R.Size2i(160, 90), 8, DEPTH, seed=SEED, thread_count=3)
    on, lf, kname, off = _on_off(monkeypatch, dw, p)
    assert kname.startswith("render_kernel_pl<") and lf["tiles_listed"] > 0
    assert_bit_identical(on.reshape(-1, 3), off.reshape(-1, 3), f"{name} thread_count 3, lists on / off")
    assert_bit_identical(on.reshape(-1, 3), refs(name, (160, 90), 8, 3), f"{name} thread_count 3")
    dw.release()


@pytest.mark.parametrize("name", ["final_scene1", "defocus_blur"])
def test_progressive_accumulator(worlds, refs, monkeypatch, name):
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    acc = R.Accumulator(worlds(name), R.Size2i(160, 90), DEPTH, seed=SEED)
    acc.add(3)
    acc.add(5)
    assert acc.dworld.kernel_variant()["name"].startswith("render_kernel_pl<")
    assert acc.dworld.last_frame()["tiles_listed"] > 0
    assert_bit_identical(acc.image(), refs(name, (160, 90), 8), f"{name} 3 + 5 samples")
    acc.release()


@pytest.mark.parametrize("name", ["final_scene1", "defocus_blur"])
def test_device_lists_equal_host_lists(worlds, monkeypatch, name):
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    world = worlds(name)
    dw = R.DeviceWorld(world, 0)
    p = R.render_params(R.Size2i(160, 90), 1, DEPTH, seed=SEED)
    _frame(dw, p)
    count, lst, _ = dw.primary_lists()
    cap = lst.shape[1]
    assert cap == min(16, world.raw.leaf_count) and len(count) == 20 * 12
    hc = np.zeros_like(count)
    hl = np.zeros_like(lst)
    i32p = C.POINTER(C.c_int32)
    N.check(N.lib().rtw_primary_lists_host(world.ptr(), C.byref(p), cap, hc.ctypes.data_as(i32p), hl.ctypes.data_as(i32p)))
    assert (count == hc).all()
    for t in range(len(count)):
        assert (lst[t, : max(0, count[t])] == hl[t, : max(0, hc[t])]).all(), t
    dw.release()


def test_counting_variant_follows_the_lists(worlds, monkeypatch):
    """tree = 1 counts the product kernel's own traversal: with lists the same paths (samples, rays, hits,
    material reads) with fewer node visits -- camera rays are about 40 % of the walk's (profiles/r08/
    primary_share.txt), so at least half of that must go -- and tree = 0 stays the reference's counts."""
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    p = R.render_params(R.Size2i(160, 90), 4, DEPTH, seed=SEED)
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "1")
    on, ref_on = dw.collect_stats(p, tree=1), dw.collect_stats(p, tree=0)
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "0")
    off, ref_off = dw.collect_stats(p, tree=1), dw.collect_stats(p, tree=0)
    print(on, off)
    same = ["samples", "rays", "sphere_hits", "rect_hits", "box_hits", "triangle_hits", "material_reads", "texel_reads"]
    assert {k: on[k] for k in same} == {k: off[k] for k in same}
    assert on["node_visits"] < 0.8 * off["node_visits"]
    assert ref_on == ref_off
    dw.release()


@pytest.mark.parametrize("name", ["earth_motion", "final_scene2"])
def test_worlds_out_of_scope_keep_the_walk(worlds, monkeypatch, name):
    dw = R.DeviceWorld(worlds(name), 0)
    p = R.render_params(R.Size2i(64, 36), 4, DEPTH, seed=SEED)
    on, lf, kname, off = _on_off(monkeypatch, dw, p)
    assert lf["tiles_listed"] == 0 and kname.startswith("render_kernel<")
    assert dw.primary_lists() is None
    assert_bit_identical(on.reshape(-1, 3), off.reshape(-1, 3), f"{name} unchanged")
    dw.release()
