"""Progressive accumulation on the device (rtw_accum, progressive.py).

The invariant: after adds of n1, n2, ... samples the resolved image is bit-identical to a one-shot render
at spp = n1 + n2 + ..., at every intermediate point too -- so to the oracle at that spp."""
import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.distributed import pack_tiles, tile_slots, untile_host
from raytracinginaweekend_amd.progressive import AccumState
from tests.parity import assert_bit_identical, bit_equal

pytestmark = pytest.mark.gpu

DEPTH = 50


def oracle(world, size, spp, seed, depth=DEPTH, mode=R.RenderMode.Default):
    return O.render(world, R.render_params(size, spp, depth, mode, seed=seed))


@pytest.mark.parametrize("name,w,h", [("final_scene1", 64, 36), ("cornell_box", 40, 40), ("cornell_box_smoke", 40, 40),
                                      ("suzanne", 48, 36), ("earth_motion", 64, 36)])
def test_split_invariance_against_the_oracle(worlds, name, w, h):
    world, size = worlds(name), R.Size2i(w, h)
    acc = R.Accumulator(world, size, DEPTH, seed=21)
    total = 0
    for n in (1, 2, 3):
        acc.add(n)
        total += n
        assert acc.samples == total
        if name == "final_scene1" and total < 6:  # every intermediate point is a frame too
            assert_bit_identical(acc.image(), oracle(world, size, total, 21), f"{name} after {total}")
    assert_bit_identical(acc.image(), oracle(world, size, 6, 21), name)
    acc.release()


def test_resolve_is_non_destructive(worlds):
    world, size = worlds("final_scene1"), R.Size2i(32, 18)
    acc = R.Accumulator(world, size, DEPTH, seed=5)
    acc.add(3)
    a, b = acc.image(), acc.image()
    assert_bit_identical(a, b, "second resolve")
    assert_bit_identical(a, oracle(world, size, 3, 5), "spp 3")
    acc.add(0)
    assert acc.samples == 3
    assert_bit_identical(acc.image(), a, "after add(0)")
    acc.add(2)
    assert_bit_identical(acc.image(), oracle(world, size, 5, 5), "spp 5 after a resolve")


def test_partitions_and_padding(worlds):
    world, size, tile = worlds("final_scene1"), R.Size2i(50, 30), (8, 8)  # edge tiles padded in both axes
    ref = oracle(world, size, 4, 9)
    stride = R.rendering.partition_floats(R.render_params(size, 1, 1, tile=tile, part=(0, 3), layout=N.LAYOUT_TILES))
    gathered = np.zeros(3 * stride, np.float32)
    dw = R.DeviceWorld(world, 0)
    padded = 0
    for r in range(3):
        acc = R.Accumulator(dw, size, DEPTH, seed=9, tile=tile, part=(r, 3), layout=N.LAYOUT_TILES)
        acc.add(2)
        acc.add(2)
        img = acc.image()
        slots = tile_slots(size, tile, (r, 3))
        assert img.shape == (len(slots), 3) and acc.slots == len(slots)
        buf = np.zeros(stride, np.float32)
        buf[: img.size] = img.ravel()
        assert_bit_identical(buf, pack_tiles(ref, size, tile, (r, 3), stride), f"part {r}")
        gathered[r * stride: (r + 1) * stride] = buf
        sums = acc.state().sums
        assert (sums.view(np.uint32)[slots < 0] == 0).all(), "exported padding slots hold zeros"
        padded += int((slots < 0).sum())
        acc.release()
    assert padded > 0
    assert_bit_identical(untile_host(gathered, size, tile, 3, stride), ref, "reassembled")


def test_several_launches_inside_one_add(worlds, monkeypatch):
    monkeypatch.setenv("RTW_SAMPLE_BUFFER_BYTES", "50000")  # 768 slots x 12 B: 5 samples fit, so 3 (one chunk) per launch
    monkeypatch.setenv("RTW_CHUNK", "3")
    world, size = worlds("final_scene1"), R.Size2i(32, 18)
    acc = R.Accumulator(world, size, DEPTH, seed=13)
    acc.add(7)
    assert acc.dworld.last_frame()["launches"] > 1
    acc.add(2)
    assert_bit_identical(acc.image(), oracle(world, size, 9, 13), "launch split")


@pytest.mark.parametrize("name,w,h", [("earth_motion", 64, 36), ("final_scene1", 32, 18)])
def test_whole_pixel_items(worlds, name, w, h, monkeypatch):
    world, size = worlds(name), R.Size2i(w, h)
    ref = oracle(world, size, 5, 17)
    images = {}
    for wp in ("1", "0"):
        monkeypatch.setenv("RTW_WHOLE_PIXEL", wp)
        acc = R.Accumulator(world, size, DEPTH, seed=17)
        acc.add(2)
        acc.add(3)
        # earth_motion takes a GEN kernel (generic leaf tables in LDS), which chooses its work items at run time
        # and serves one-shot frames too: continuing a sum there moved that kernel's SGPR spills (8 of 8 GEN
        # variants, profiles/r07/resources_accum.txt), so the resource guard dropped the change for those
        # kernels and their accumulators add single samples.  The WP = true kernels (final_scene1) take it.
        gen = acc.dworld.kernel_variant()["name"].split(", ")[4] == "true"
        assert gen is (name == "earth_motion")
        assert acc.dworld.last_frame()["whole_pixel"] is (wp == "1" and not gen)
        images[wp] = acc.image()
        assert_bit_identical(images[wp], ref, f"{name} RTW_WHOLE_PIXEL={wp}")
        acc.release()
    assert_bit_identical(images["1"], images["0"], "whole-pixel against single-sample items")


def test_interleaving_on_one_world(worlds, monkeypatch):
    import torch

    world, size = worlds("final_scene1"), R.Size2i(40, 24)  # 960 slots x 12 B: 4 samples per 50000 B launch
    dw = R.DeviceWorld(world, 0)
    a = R.Accumulator(dw, size, DEPTH, seed=3)
    a.add(2)
    # a one-shot frame of several launches: it carries its sum in the world's own running buffer
    monkeypatch.setenv("RTW_SAMPLE_BUFFER_BYTES", "50000")
    out = torch.zeros(size.count() * 3, dtype=torch.float32, device="cuda:0")
    dw.render_into(R.render_params(size, 5, DEPTH, seed=3), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert dw.last_frame()["launches"] > 1
    monkeypatch.delenv("RTW_SAMPLE_BUFFER_BYTES")
    b = R.Accumulator(dw, size, DEPTH, seed=4)
    b.add(1)
    a.add(2)
    assert_bit_identical(a.image(), oracle(world, size, 4, 3), "accumulator A")
    assert_bit_identical(out.cpu().numpy().reshape(-1, 3), oracle(world, size, 5, 3), "one-shot frame")
    assert_bit_identical(b.image(), oracle(world, size, 1, 4), "accumulator B")


def test_checkpoint(worlds, tmp_path):
    size = R.Size2i(32, 18)
    world = R.demo_world("simple_plane")
    dw = R.DeviceWorld(world, 0)
    acc = R.Accumulator(dw, size, DEPTH, seed=8)
    acc.add(3)
    path = tmp_path / "frame.npz"
    acc.state().save(path)
    acc.release()
    dw.release()
    del acc, dw, world

    state = AccumState.load(path)
    assert state.samples == 3
    world = R.demo_world("simple_plane")  # a fresh build and upload
    acc = R.Accumulator(R.DeviceWorld(world, 0), size, DEPTH, seed=8)
    acc.load_state(state)
    assert acc.samples == 3
    acc.add(2)
    assert_bit_identical(acc.image(), oracle(world, size, 5, 8), "resumed frame")

    def refused(field, w=world, sz=size, depth=DEPTH, seed=8):
        other = R.Accumulator(w, sz, depth, seed=seed)
        with pytest.raises(N.RtwError) as e:
            other.load_state(state)
        assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT
        assert field in str(e.value), str(e.value)
        assert other.samples == 0
        other.release()

    refused("seed", seed=9)
    refused("width", sz=R.Size2i(48, 10))  # (the same number of slots: the geometry itself is checked)
    refused("max_depth", depth=10)
    refused("world_fingerprint", w=worlds("defocus_blur"))


def test_world_released_before_its_accumulator(worlds):
    """Either release order is safe (a garbage collector picks one): once the world is gone the accumulator
    answers with an error instead of touching freed state, and its own release still works."""
    world, size = worlds("simple_plane"), R.Size2i(32, 18)
    dw = R.DeviceWorld(world, 0)
    acc = R.Accumulator(dw, size, DEPTH, seed=1, moments=True)
    acc.add(2)
    dw.release()
    assert acc.samples == 2  # host bookkeeping
    for call in (lambda: acc.add(1), acc.image, acc.stderr, acc.noise, acc.state):
        with pytest.raises(N.RtwError) as e:
            call()
        assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT and "world was released" in str(e.value)
    acc.release()
    acc.release()


def test_modes_and_refusals(worlds):
    world, size = worlds("cornell_box"), R.Size2i(40, 30)
    acc = R.Accumulator(world, size, DEPTH, R.RenderMode.Normals, seed=2)
    acc.add(1)
    acc.add(1)
    assert_bit_identical(acc.image(), oracle(world, size, 2, 2, mode=R.RenderMode.Normals), "normals")
    world, size = worlds("final_scene1"), R.Size2i(32, 18)
    acc = R.Accumulator(world, size, 2, seed=2)
    acc.add(1)
    acc.add(1)
    assert_bit_identical(acc.image(), oracle(world, size, 2, 2, depth=2), "max_depth 2")

    with pytest.raises(N.RtwError) as e:
        R.Accumulator(world, size, DEPTH, seed=2, thread_count=2)
    assert e.value.code == N.RTW_ERR_UNSUPPORTED
    fresh = R.Accumulator(world, size, DEPTH, seed=2)
    with pytest.raises(N.RtwError) as e:
        fresh.image()  # 0 samples
    assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT
    fresh.add(2)
    with pytest.raises(N.RtwError):
        fresh.stderr()  # no moments
    with pytest.raises(N.RtwError):
        fresh.noise()
    m = R.Accumulator(world, size, DEPTH, seed=2, moments=True)
    m.add(1)
    with pytest.raises(N.RtwError) as e:
        m.stderr()  # one sample
    assert e.value.code == N.RTW_ERR_INVALID_ARGUMENT
    with pytest.raises(N.RtwError):
        m.noise()


@pytest.mark.parametrize("name,w,h", [("final_scene1", 24, 16), ("cornell_box", 20, 20)])
def test_moments(worlds, name, w, h):
    world, size = worlds(name), R.Size2i(w, h)
    p = R.render_params(size, 5, DEPTH, seed=31)
    colors = np.stack([np.stack([O.sample_color(world, p, i % w, i // w, s) for i in range(w * h)]) for s in range(5)])
    f32 = np.float32
    with np.errstate(all="ignore"):
        total = np.zeros((w * h, 3), f32)
        sq = np.zeros((w * h, 3), f32)
        for s in range(5):  # in sample order, every product and sum rounded to f32
            total = total + colors[s]
            sq = sq + colors[s] * colors[s]
        nf = f32(5)
        mean = total / nf
        d = sq - total * mean
        var = np.where(d < 0, f32(0), d) / f32(4)
        se = np.sqrt(var / nf)
        e = ((se[:, 0] + se[:, 1]) + se[:, 2]) / (((mean[:, 0] + mean[:, 1]) + mean[:, 2]) + f32(0.01))
    assert total.dtype == sq.dtype == se.dtype == e.dtype == np.float32
    finite = np.isfinite(e)

    acc = R.Accumulator(world, size, DEPTH, seed=31, moments=True)
    acc.add(2)
    acc.add(3)
    assert acc.dworld.last_frame()["whole_pixel"] is False  # moments: single-sample items
    assert_bit_identical(acc.image(), mean, "mean")
    assert_bit_identical(acc.stderr(), se, "standard error")
    st = acc.state()  # in slot order (tile-major), whatever the layout
    slots = tile_slots(size, (8, 8), (0, 1))
    owned = slots >= 0
    assert st.sums.shape == st.squares.shape == (len(slots), 3)
    assert_bit_identical(st.sums[owned], total[slots[owned]], "exported sums")
    assert_bit_identical(st.squares[owned], sq[slots[owned]], "exported squares")
    assert (st.squares.view(np.uint32)[~owned] == 0).all()
    noise, counted = acc.noise()
    assert counted == int(finite.sum())
    want = float(e[finite].astype(np.float64).mean())
    print(f"{name}: noise {noise!r} numpy {want!r} pixels {counted} of {w * h}")
    assert abs(noise - want) <= 1e-9 * abs(want)

    plain = R.Accumulator(acc.dworld, size, DEPTH, seed=31)
    plain.add(2)
    plain.add(3)
    assert_bit_identical(plain.image(), acc.image(), "moments=False against moments=True")
    assert bit_equal(plain.image(), oracle(world, size, 5, 31)).all()


def test_render_to_noise_and_render_progressive(worlds):
    world, size = worlds("simple_plane"), R.Size2i(32, 18)
    img, n, noise = R.render_to_noise(size, DEPTH, world, 0.0, 8, batch=2, seed=6)
    assert n == 8 and noise > 0.0
    assert_bit_identical(img, oracle(world, size, 8, 6), "target 0: runs to max_samples")
    img, n, noise = R.render_to_noise(size, DEPTH, world, 1e30, 8, batch=2, seed=6)
    assert n == 2 and noise <= 1e30
    assert_bit_identical(img, oracle(world, size, 2, 6), "huge target: stops after the first batch")
    seen = []
    for samples, image in R.render_progressive(size, DEPTH, world, (1, 1, 2), seed=6):
        assert_bit_identical(image, oracle(world, size, samples, 6), f"progressive at {samples}")
        seen.append(samples)
    assert seen == [1, 2, 4]
