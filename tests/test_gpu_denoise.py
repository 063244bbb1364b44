"""The preview denoiser on the device (rtw_denoiser_run, Denoiser, Accumulator.denoised).

The contract is bits: the three kernels, the host twin (rtw_denoise_host) and the numpy restatement
(tests/denoise_ref.py) evaluate one fixed f32 expression (include/rtw_denoise.h)."""
import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from tests import adaptive_ref as A
from tests import denoise_ref as D
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

CASES, case_id = D.CASES, D.case_id
DEPTH, SEED, SPP = 50, 31, 8
f32 = np.float32
_denoisers = {}


def denoiser(size):
    if size not in _denoisers:
        _denoisers[size] = R.Denoiser(R.Size2i(*size))
    return _denoisers[size]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_device_host_twin_and_numpy_agree(case):
    size, gc, iterations, seed = case
    color, se, guide = D.synthetic(size, gc, seed)
    want, want_var = D.denoise(color, se, guide, size, iterations, 1.5, 0.35)
    host, host_var = R.denoise_host(R.Size2i(*size), color, se, guide, iterations=iterations, variance=True)
    got, got_var = denoiser(size).run(color, se, guide, iterations=iterations, variance=True)
    assert got.dtype == np.float32 and got.shape == want.shape and got_var.shape == want_var.shape
    assert_bit_identical(got, want, f"device against numpy, image {case_id(case)}")
    assert_bit_identical(got_var, want_var, f"device against numpy, variance {case_id(case)}")
    assert_bit_identical(got, host, "device against the host twin, image")
    assert_bit_identical(got_var, host_var, "device against the host twin, variance")
    left = np.isnan(want_var)
    assert (got.view(np.uint32)[left] == color.view(np.uint32)[left]).all()  # left out: bit for bit as it went in


@pytest.fixture(scope="module")
def frames(worlds):
    """Per world: the accumulator at 8 spp, its Normals twin, and their images on the host (computed once)."""
    cache = {}

    def get(name, w, h):
        if name not in cache:
            size = R.Size2i(w, h)
            acc = R.Accumulator(worlds(name), size, DEPTH, seed=SEED, moments=True)
            acc.add(SPP)
            normals = R.Accumulator(acc.dworld, size, DEPTH, R.RenderMode.Normals, seed=SEED)
            normals.add(SPP)
            cache[name] = (acc, normals, acc.image(), acc.stderr(), normals.image())
        return cache[name]

    return get


@pytest.mark.parametrize("name,w,h", [("final_scene1", 64, 36), ("cornell_box", 40, 40), ("suzanne", 64, 48)])
def test_accumulator_denoised(frames, name, w, h):
    acc, normals, image, se, guide = frames(name, w, h)
    assert image.dtype == se.dtype == guide.dtype == np.float32
    want, want_var = D.denoise(image, se, guide, (w, h))
    got, got_var = acc.denoised(guide=normals, variance=True)
    assert_bit_identical(got, want, f"{name} guided by a Normals accumulator")
    assert_bit_identical(got_var, want_var, f"{name} variance")
    assert_bit_identical(acc.denoised(guide=guide), want, f"{name} guided by an array")
    left = int(np.isnan(want_var).sum())
    print(f"{name} {w}x{h}: {left} pixels left out, {(got.view(np.uint32) != image.view(np.uint32)).any(axis=1).sum()} changed")
    if name == "suzanne":
        assert left >= 1  # (the frame has pixels whose colour is not finite)
    assert (got.view(np.uint32) != image.view(np.uint32)).any()
    # unguided, and with other options
    assert_bit_identical(acc.denoised(), D.denoise(image, se, None, (w, h))[0], f"{name} unguided")
    assert_bit_identical(acc.denoised(guide=normals, iterations=5, sigma_l=2.0, sigma_g=0.5),
                         D.denoise(image, se, guide, (w, h), 5, 2.0, 0.5)[0], f"{name} other options")


def test_adaptive_accumulator(worlds):
    """Tiles with different sample counts flow through the same path."""
    world, size, tile = worlds("cornell_box"), R.Size2i(40, 40), (8, 8)
    acc = R.Accumulator(world, size, DEPTH, seed=SEED, adaptive=True)
    acc.add(SPP)
    st = acc.state()
    E = A.tiles_E(st.sums, st.squares, SPP, size, tile, (0, 1))
    active, _ = acc.adapt(float(f32(np.median(E))), SPP)
    assert 0 < active < acc.tiles
    acc.add(1)
    counts = acc.sample_counts()
    assert set(np.unique(counts)) == {SPP, SPP + 1}
    image, se = acc.image(), acc.stderr()
    got, got_var = acc.denoised(variance=True)
    want, want_var = D.denoise(image, se, None, (40, 40))
    assert_bit_identical(got, want, "adaptive frame")
    assert_bit_identical(got_var, want_var, "adaptive frame, variance")
    acc.release()


def test_non_destructive(worlds):
    world, size = worlds("final_scene1"), R.Size2i(64, 36)
    acc = R.Accumulator(world, size, DEPTH, seed=SEED, moments=True)
    normals = R.Accumulator(acc.dworld, size, DEPTH, R.RenderMode.Normals, seed=SEED)
    acc.add(SPP)
    normals.add(2)
    before, n_before = acc.image(), normals.image()
    first = acc.denoised(guide=normals)
    assert_bit_identical(acc.image(), before, "image() after denoised()")
    assert_bit_identical(normals.image(), n_before, "the guide's image() after denoised()")
    assert_bit_identical(acc.denoised(guide=normals), first, "a second denoised()")
    assert acc.samples == SPP
    acc.add(2)
    assert_bit_identical(acc.image(), O.render(world, R.render_params(size, SPP + 2, DEPTH, seed=SEED)), "a further add")
    acc.release()
    normals.release()


def test_call_shape(worlds):
    import torch

    size = (65, 5)
    n = size[0] * size[1]
    color, se, guide = D.synthetic(size, 3, 11)
    want, want_var = D.denoise(color, se, guide, size, 3, 1.5, 0.35)
    d = R.Denoiser(R.Size2i(*size))
    dev = torch.device("cuda", 0)
    tc, ts, tg = (torch.from_numpy(a).to(dev) for a in (color, se, guide))
    out, var = d.run(tc, ts, tg, variance=True)  # device tensors in, device tensors out
    assert out.device.type == "cuda" and out.shape == (n, 3) and var.shape == (n,)
    torch.cuda.synchronize()
    assert_bit_identical(out.cpu().numpy(), want, "separate buffers")
    assert_bit_identical(var.cpu().numpy(), want_var, "the variance output")
    assert_bit_identical(tc.cpu().numpy(), color, "the input is left alone")
    again = d.run(tc, ts, tg)  # a second run on one Denoiser
    same = d.run_device(tc, ts, tg, tc)  # d_out == d_color
    assert same.data_ptr() == tc.data_ptr()
    torch.cuda.synchronize()
    assert_bit_identical(again.cpu().numpy(), want, "a second run")
    assert_bit_identical(tc.cpu().numpy(), want, "out == color")
    # refusals of the device call: another size, null pointers, bad fields
    with pytest.raises(ValueError, match="color"):
        d.run(color[:-1], se[:-1])
    p = N.DenoiseParams(size[0] + 1, size[1], 3, 0, 1.5, 0.35, 0, 0)
    args = [ts.data_ptr(), ts.data_ptr(), None, out.data_ptr(), None, None]
    lib = N.lib()
    assert lib.rtw_denoiser_run(d._h, p, *args) == N.RTW_ERR_INVALID_ARGUMENT and b"width" in lib.rtw_last_error()
    p = N.DenoiseParams(size[0], size[1] - 1, 3, 0, 1.5, 0.35, 0, 0)
    assert lib.rtw_denoiser_run(d._h, p, *args) == N.RTW_ERR_INVALID_ARGUMENT and b"height" in lib.rtw_last_error()
    p = N.DenoiseParams(size[0], size[1], 3, 2, 1.5, 0.35, 0, 0)
    assert lib.rtw_denoiser_run(d._h, p, *args) == N.RTW_ERR_INVALID_ARGUMENT and b"d_guide" in lib.rtw_last_error()
    p = N.DenoiseParams(size[0], size[1], 3, 0, 1.5, 0.35, 0, 0)
    for i, which in ((0, b"d_color"), (1, b"d_stderr"), (3, b"d_out")):
        a = list(args)
        a[i] = None
        assert lib.rtw_denoiser_run(d._h, p, *a) == N.RTW_ERR_INVALID_ARGUMENT and which in lib.rtw_last_error()
    for field, value in (("iterations", 0), ("iterations", 7), ("guide_channels", 5), ("sigma_l", 0.0),
                         ("sigma_g", float("nan")), ("reserved0", 1), ("reserved1", 1)):
        q = N.DenoiseParams(size[0], size[1], 3, 0, 1.5, 0.35, 0, 0)
        setattr(q, field, value)
        assert lib.rtw_denoiser_run(d._h, q, *args) == N.RTW_ERR_INVALID_ARGUMENT
        assert field.encode() in lib.rtw_last_error()
    d.release()
    # a filter needs the whole image, moments and two samples
    world = worlds("final_scene1")
    tiles = R.Accumulator(world, R.Size2i(32, 16), DEPTH, seed=SEED, moments=True, layout=N.LAYOUT_TILES)
    part = R.Accumulator(tiles.dworld, R.Size2i(32, 16), DEPTH, seed=SEED, moments=True, part=(1, 2))
    plain = R.Accumulator(tiles.dworld, R.Size2i(32, 16), DEPTH, seed=SEED)
    young = R.Accumulator(tiles.dworld, R.Size2i(32, 16), DEPTH, seed=SEED, moments=True)
    for acc in (tiles, part, plain):
        acc.add(2)
    young.add(1)
    for acc, what in ((tiles, "LAYOUT_TILES"), (part, "partition"), (plain, "moments"), (young, "samples")):
        with pytest.raises(ValueError, match=what):
            acc.denoised()
        acc.release()
