"""First-hit AOVs and albedo demodulation on the device (rtw_aov_*, rtw_denoiser_run_albedo).

The contract is bits.  Albedo: the oracle's radiance of the world's emissive twin at max_depth 2 (tests/aov_ref.py).
Normal: the oracle's RenderMode.Normals frame, and an Accumulator(RenderMode.Normals) after the same adds.  Depth
and hits: the per-sample oracle loop.  The demodulated filter: tests/aov_ref.denoise_albedo."""
import ctypes as C

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from tests import aov_ref as A
from tests import denoise_ref as D
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

SIZE, SEED, ADDS = R.Size2i(37, 19), 7, (2, 3)  # no multiple of a tile, a wave or a block
SPP = sum(ADDS)
DEPTH = 50
f32 = np.float32
CASES = [((2, 2), 0, 2, 1), ((2, 2), 3, 3, 2), ((7, 5), 0, 3, 3), ((7, 5), 3, 4, 4), ((37, 23), 0, 5, 5),
         ((37, 23), 3, 3, 6)]


def case_id(c):
    return f"{c[0][0]}x{c[0][1]}-gc{c[1]}-it{c[2]}"


def check_world(world, size, adds, seed, name):
    spp = sum(adds)
    aov = R.AovAccumulator(world, size, seed=seed)
    normals = R.Accumulator(aov.dworld, size, DEPTH, R.RenderMode.Normals, seed=seed)
    for n in adds:
        aov.add(n)
        normals.add(n)
    assert aov.samples == spp and aov.info().channels == 7 and aov.info().seed == seed
    albedo, normal, depth, hits = aov.albedo(), aov.normal(), aov.depth(), aov.hits()
    assert albedo.shape == normal.shape == (size.count(), 3) and depth.shape == hits.shape == (size.count(),)
    assert albedo.dtype == normal.dtype == depth.dtype == np.float32 and hits.dtype == np.uint32
    assert_bit_identical(albedo, A.twin_albedo(world, size, spp, seed), f"{name} albedo against the twin")
    want_n = O.render(world, R.render_params(size, spp, DEPTH, R.RenderMode.Normals, seed=seed))
    assert_bit_identical(normal, want_n, f"{name} normal against the oracle's Normals frame")
    assert_bit_identical(normal, normals.image(), f"{name} normal against Accumulator(Normals)")
    want_d, want_h = A.depth_hits(world, size, spp, seed)
    assert (hits == want_h).all(), f"{name} hits"
    assert_bit_identical(depth, want_d, f"{name} depth")
    assert np.isfinite(depth).all() and (depth[hits == 0] == 0).all()
    # one add of the sum
    once = R.AovAccumulator(aov.dworld, size, seed=seed)
    once.add(spp)
    for what, a, b in (("albedo", once.albedo(), albedo), ("normal", once.normal(), normal),
                       ("depth", once.depth(), depth)):
        assert_bit_identical(a, b, f"{name} {what}: one add of {spp} against adds of {adds}")
    assert (once.hits() == hits).all()
    for h in (aov, normals, once):
        h.release()
    return hits


@pytest.mark.parametrize("name", A.GPU_WORLDS)
def test_aovs_against_the_oracle(worlds, name):
    hits = check_world(worlds(name), SIZE, ADDS, SEED, name)
    assert hits.max() == SPP  # (every world is hit somewhere)


@pytest.mark.parametrize("name", ["final_scene1", "earth_mapped"])
def test_a_second_size(worlds, name):
    check_world(worlds(name), R.Size2i(64, 36), (1, 2), 11, name)


def test_leaf_lists_change_no_bit(worlds, monkeypatch):
    """final_scene1's camera rays come from per-tile leaf lists (a world of plain spheres); with RTW_PRIMARY_LISTS=0
    at create every ray takes the walk.  160 x 90 (tiles with lists, empty lists and ties at sphere rims), 3 samples:
    the same bits, which are the oracle's."""
    world, size = worlds("final_scene1"), R.Size2i(160, 90)
    dw = R.DeviceWorld(world, 0)
    listed = R.AovAccumulator(dw, size, seed=SEED)
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "0")
    walked = R.AovAccumulator(dw, size, seed=SEED)
    monkeypatch.delenv("RTW_PRIMARY_LISTS")
    for aov in (listed, walked):
        aov.add(1)
        aov.add(2)
    for what in ("albedo", "normal", "depth"):
        assert_bit_identical(getattr(listed, what)(), getattr(walked, what)(), f"{what}: lists against the walk")
    assert (listed.hits() == walked.hits()).all()
    want = O.render(world, R.render_params(size, 3, DEPTH, R.RenderMode.Normals, seed=SEED))
    assert_bit_identical(listed.normal(), want, "normal against the oracle's Normals frame")
    assert_bit_identical(listed.albedo(), A.twin_albedo(world, size, 3, SEED), "albedo against the twin")
    listed.release()
    walked.release()


def test_render_aov_and_channel_subsets(worlds):
    world = worlds("cornell_box_smoke")
    full = R.render_aov(SIZE, 3, world, seed=SEED)
    assert set(full) == {"albedo", "normal", "depth", "hits"}
    dw = R.DeviceWorld(world, 0)
    for channels in (("albedo",), ("normal",), ("depth",), ("depth", "albedo")):
        aov = R.AovAccumulator(dw, SIZE, seed=SEED, channels=channels)
        aov.add(3)
        for c in channels:
            assert_bit_identical(getattr(aov, c)(), full[c], f"{c} of an accumulator holding {channels}")
        assert (aov.hits() == full["hits"]).all()
        for c in {"albedo", "normal", "depth"} - set(channels):
            with pytest.raises(ValueError, match=c):
                getattr(aov, c)()
            buf = aov.hits_device()
            bit = {"albedo": N.AOV_ALBEDO, "normal": N.AOV_NORMAL, "depth": N.AOV_DEPTH}[c]
            rc = N.lib().rtw_aov_resolve(aov._h, bit, C.c_void_p(buf.data_ptr()), None)
            assert rc == N.RTW_ERR_INVALID_ARGUMENT and b"channel" in N.lib().rtw_last_error()
        aov.release()


def test_interleaved_with_a_colour_accumulator(worlds):
    world = worlds("final_scene2")
    dw = R.DeviceWorld(world, 0)
    aov = R.AovAccumulator(dw, SIZE, seed=SEED)
    acc = R.Accumulator(dw, SIZE, DEPTH, seed=SEED, moments=True)
    for n in (1, 2, 1):
        aov.add(n)
        acc.add(n)
        acc.image()
        aov.albedo()
    alone = R.AovAccumulator(world, SIZE, seed=SEED)
    alone.add(4)
    assert_bit_identical(aov.albedo(), alone.albedo(), "albedo beside a colour accumulator")
    assert_bit_identical(aov.normal(), alone.normal(), "normal beside a colour accumulator")
    assert_bit_identical(aov.depth(), alone.depth(), "depth beside a colour accumulator")
    assert_bit_identical(acc.image(), O.render(world, R.render_params(SIZE, 4, DEPTH, seed=SEED)),
                         "the colour accumulator beside an AOV accumulator")
    for h in (aov, acc, alone):
        h.release()


# ---- the demodulated filter -----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_run_device_with_albedo(case):
    import torch

    size, gc, iterations, seed = case
    color, se, guide = D.synthetic(size, gc, seed)
    albedo = A.synthetic_albedo(size, seed)
    want, want_var = A.denoise_albedo(color, se, guide, albedo, size, iterations)
    d = R.Denoiser(R.Size2i(*size))
    got, got_var = d.run(color, se, guide, albedo=albedo, iterations=iterations, variance=True)
    assert_bit_identical(got, want, f"device against numpy, image {case_id(case)}")
    assert_bit_identical(got_var, want_var, f"device against numpy, variance {case_id(case)}")
    host = R.denoise_host(R.Size2i(*size), color, se, guide, albedo=albedo, iterations=iterations)
    assert_bit_identical(got, host, "device against the host twin")
    left = np.isnan(want_var)
    assert (got.view(np.uint32)[left] == color.view(np.uint32)[left]).all()
    # albedo=None is the filter as it was
    assert_bit_identical(d.run(color, se, guide, albedo=None, iterations=iterations),
                         D.denoise(color, se, guide, size, iterations)[0], "albedo=None")
    # out aliasing color
    dev = torch.device("cuda", 0)
    tc, ts, ta = (torch.from_numpy(a).to(dev) for a in (color, se, albedo))
    tg = None if guide is None else torch.from_numpy(guide).to(dev)
    same = d.run_device(tc, ts, tg, tc, albedo=ta, iterations=iterations)
    assert same.data_ptr() == tc.data_ptr()
    torch.cuda.synchronize()
    assert_bit_identical(tc.cpu().numpy(), want, "out == color")
    assert_bit_identical(ta.cpu().numpy(), albedo, "the albedo is left alone")
    d.release()


@pytest.fixture(scope="module")
def frame(worlds):
    """earth_mapped 64 x 36: a colour accumulator at 8 spp and an AOV accumulator at 16 on one DeviceWorld."""
    size = R.Size2i(64, 36)
    acc = R.Accumulator(worlds("earth_mapped"), size, DEPTH, seed=31, moments=True)
    acc.add(8)
    aov = R.AovAccumulator(acc.dworld, size, seed=31)
    aov.add(16)
    yield acc, aov, size
    acc.release()
    aov.release()


def test_accumulator_denoised_with_aovs(frame):
    acc, aov, size = frame
    image, se, albedo, normal = acc.image(), acc.stderr(), aov.albedo(), aov.normal()
    want, want_var = A.denoise_albedo(image, se, normal, albedo, (size.width, size.height))
    got, got_var = acc.denoised(guide=aov, albedo=aov, variance=True)
    assert_bit_identical(got, want, "denoised(guide=aov, albedo=aov) against numpy on the accumulator frame")
    assert_bit_identical(got_var, want_var, "its variance")
    d = R.Denoiser(size)
    assert_bit_identical(got, d.run(image, se, normal, albedo=albedo), "against Denoiser.run on the resolved arrays")
    d.release()
    assert_bit_identical(acc.denoised(guide=normal, albedo=albedo), want, "arrays for both")
    assert_bit_identical(acc.denoised(albedo=aov), A.denoise_albedo(image, se, None, albedo, (size.width, size.height))[0],
                         "unguided")
    assert_bit_identical(acc.denoised(guide=aov), D.denoise(image, se, normal, (size.width, size.height))[0],
                         "the AOV normal as the guide of today's filter")
    assert (got.view(np.uint32) != image.view(np.uint32)).any()
    assert_bit_identical(acc.image(), image, "image() after denoised()")
    assert_bit_identical(aov.albedo(), albedo, "the AOV accumulator after denoised()")


def test_refusals(frame, worlds):
    acc, aov, size = frame
    other = R.AovAccumulator(acc.dworld, R.Size2i(32, 18), seed=31)
    other.add(1)
    empty = R.AovAccumulator(acc.dworld, size, seed=31)
    for kw in (dict(guide=other), dict(albedo=other)):
        with pytest.raises(ValueError, match="size"):
            acc.denoised(**kw)
    for kw in (dict(guide=empty), dict(albedo=empty)):
        with pytest.raises(ValueError, match="no samples"):
            acc.denoised(**kw)
    # a resolve at 0 samples, of an unknown channel; hits at any point
    lib = N.lib()
    buf = empty.hits_device()
    assert (empty.hits() == 0).all()
    for channel in (N.AOV_ALBEDO, N.AOV_NORMAL, N.AOV_DEPTH):
        assert lib.rtw_aov_resolve(empty._h, channel, C.c_void_p(buf.data_ptr()), None) == N.RTW_ERR_INVALID_ARGUMENT
        assert b"samples" in lib.rtw_last_error()
    for channel in (0, 3, 8):
        assert lib.rtw_aov_resolve(aov._h, channel, C.c_void_p(buf.data_ptr()), None) == N.RTW_ERR_INVALID_ARGUMENT
        assert b"channel" in lib.rtw_last_error()
    with pytest.raises(R._native.RtwError, match="samples"):
        empty.albedo()
    for n in (-1, 1 << 32):
        with pytest.raises(ValueError, match="n must be"):
            empty.add(n)
    assert empty.samples == 0
    # create on a live world: the same refusals as without one, and nothing comes back
    for field, code, channels, kw in (("layout", N.RTW_ERR_UNSUPPORTED, 7, dict(layout=N.LAYOUT_TILES)),
                                      ("part_count", N.RTW_ERR_UNSUPPORTED, 7, dict(part_count=2)),
                                      ("thread_count", N.RTW_ERR_UNSUPPORTED, 7, dict(thread_count=2)),
                                      ("channels", N.RTW_ERR_INVALID_ARGUMENT, 0, {}),
                                      ("channels", N.RTW_ERR_INVALID_ARGUMENT, 16, {}),
                                      ("reserved0", N.RTW_ERR_INVALID_ARGUMENT, 7, dict(reserved0=1))):
        p = R.render_params(size, 0, 0, seed=1)
        for k, v in kw.items():
            setattr(p, k, v)
        h = C.c_void_p(0xDEAD)
        assert lib.rtw_aov_create(acc.dworld._h, C.byref(p), channels, C.byref(h)) == code, field
        assert field.encode() in lib.rtw_last_error() and not h.value
    # the world released first: the accumulator refuses, and its release stays safe
    dw = R.DeviceWorld(worlds("final_scene1"), 0)
    late = R.AovAccumulator(dw, size, seed=1)
    late.add(1)
    lib.rtw_world_release(dw._h)
    dw._h = None
    assert lib.rtw_aov_add(late._h, 1, None) == N.RTW_ERR_INVALID_ARGUMENT and b"released" in lib.rtw_last_error()
    assert late.samples == 1
    late.release()
    other.release()
    empty.release()
