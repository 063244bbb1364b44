"""First-hit AOVs and albedo demodulation, the parts that need no GPU: the emissive twin that
defines the albedo AOV, the host twin of the demodulated filter (rtw_denoise_host_albedo) against numpy bit for
bit, the refusals, the demodulated filter's quality on earth_mapped, and the stand-alone program
tests/native/denoise_albedo_check.c -- built once plain and once with -fsanitize=address,undefined, run alone."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from tests import aov_ref as A
from tests import denoise_ref as D
from tests.parity import assert_bit_identical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "denoise_albedo_check.c")
FLAGS = ["-std=c11", "-ffp-contract=off", "-fno-fast-math"]
f32 = np.float32

# sizes (2,2), (7,5), (37,23) with 0 and 3 guide channels: (size, gc, iterations, seed)
CASES = [((2, 2), 0, 2, 1), ((2, 2), 3, 3, 2), ((7, 5), 0, 3, 3), ((7, 5), 3, 4, 4), ((37, 23), 0, 5, 5),
         ((37, 23), 3, 3, 6)]


def case_id(c):
    return f"{c[0][0]}x{c[0][1]}-gc{c[1]}-it{c[2]}"


# ---- 1. the twin is the definition -----------------------------------------------------------------
def test_the_twin_is_the_definition(worlds):
    """final_scene1 24 x 14 x 3: every sample of the oracle's radiance of the emissive twin (max_depth 2) is the
    texture of the material scene_hit finds on the same stream -- its solid colour -- or 1 for a dielectric and on
    a miss; and the twin's frame is the in-order mean of those samples."""
    world, size, spp, seed = worlds("final_scene1"), R.Size2i(24, 14), 3, 7
    twin = A.Twin(world)
    p = R.render_params(size, spp, 2, seed=seed)
    total = np.zeros((size.count(), 3), f32)
    kinds = {"miss": 0, "dielectric": 0, "solid": 0}
    for pix in range(size.count()):
        x, y = pix % size.width, pix // size.width
        for s in range(spp):
            got = O.sample_color(twin, p, x, y, s)
            h = A.primary_hit(world, size, seed, x, y, s)
            if not h.hit:
                want, kind = np.ones(3, f32), "miss"
            else:
                m = world.raw.materials[h.material]
                if m.kind == N.MAT_DIELECTRIC:
                    want, kind = np.ones(3, f32), "dielectric"
                else:
                    t = world.raw.textures[m.texture]
                    assert t.kind == N.TEX_SOLID, "final_scene1 holds solid textures only"
                    want, kind = np.array(list(t.color), f32), "solid"
            kinds[kind] += 1
            assert_bit_identical(got, want, f"pixel ({x}, {y}) sample {s}: {kind}")
            total[pix] = total[pix] + got
    assert all(v > 0 for v in kinds.values()), kinds
    assert_bit_identical(total / f32(spp), O.render(twin, p), "the frame is the samples' in-order mean")


@pytest.mark.parametrize("name", ["earth_mapped", "cornell_box_smoke", "cornell_box"])
def test_twin_frames_are_finite(worlds, name):
    a = A.twin_albedo(worlds(name), R.Size2i(24, 14), 2, 7)
    assert np.isfinite(a).all() and (a >= 0).all()
    if name == "earth_mapped":
        assert a.max() <= 1.0
    if name == "cornell_box":
        assert a.max() == 15.0  # the lamp's emit texture


# ---- 2. the host twin against numpy ----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_host_twin_against_numpy(case):
    size, gc, iterations, seed = case
    n = size[0] * size[1]
    color, se, guide = D.synthetic(size, gc, seed)
    albedo = A.synthetic_albedo(size, seed)
    want, want_var = A.denoise_albedo(color, se, guide, albedo, size, iterations)
    got, got_var = R.denoise_host(R.Size2i(*size), color, se, guide, albedo=albedo, iterations=iterations, variance=True)
    assert got.dtype == np.float32 and got.shape == (n, 3) and got_var.shape == (n,)
    assert_bit_identical(got, want, f"image {case_id(case)}")
    assert_bit_identical(got_var, want_var, f"variance {case_id(case)}")
    # left-out pixels return their input bits, NaN payloads and all
    left = np.isnan(got_var)
    assert (got.view(np.uint32)[left] == color.view(np.uint32)[left]).all()
    bad_albedo = ~np.isfinite(albedo).all(axis=1)
    assert bad_albedo.any() and left[bad_albedo].all()
    if n >= 24:
        assert (~left).any() and (got.view(np.uint32)[~left] != color.view(np.uint32)[~left]).any()
    # out may be color
    buf = color.copy()
    p = N.DenoiseParams(size[0], size[1], iterations, gc, 1.5, 0.35, 0, 0)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    assert N.lib().rtw_denoise_host_albedo(C.byref(p), ptr(buf), ptr(se), ptr(guide), ptr(albedo), ptr(buf), None) == 0
    assert_bit_identical(buf, want, "out aliasing color")
    # albedo=None is today's filter
    today = D.denoise(color, se, guide, size, iterations)[0]
    assert_bit_identical(R.denoise_host(R.Size2i(*size), color, se, guide, albedo=None, iterations=iterations), today,
                         "albedo=None")
    assert_bit_identical(R.denoise_host(R.Size2i(*size), color, se, guide, iterations=iterations), today, "no albedo")
    # an albedo of ones divides and multiplies by 1: today's output on every pixel
    ones = np.ones((n, 3), f32)
    assert_bit_identical(R.denoise_host(R.Size2i(*size), color, se, guide, albedo=ones, iterations=iterations), today,
                         "albedo of ones")


# ---- 3. the refusals ----------------------------------------------------------------------------------
def _aov_create(channels, **kw):
    p = R.render_params(R.Size2i(16, 9), 0, 0, seed=1)
    for k, v in kw.items():
        setattr(p, k, v)
    h = C.c_void_p(0xDEAD)
    rc = N.lib().rtw_aov_create(None, C.byref(p), channels, C.byref(h))
    return rc, (N.lib().rtw_last_error() or b"").decode(), h


def test_refusals():
    # rtw_aov_create checks the params before the world: refused without a device, nothing allocated
    for field, kw in (("layout", dict(layout=N.LAYOUT_TILES)), ("part_count", dict(part_count=2)),
                      ("thread_count", dict(thread_count=2))):
        rc, msg, h = _aov_create(N.AOV_ALBEDO, **kw)
        assert rc == N.RTW_ERR_UNSUPPORTED and field in msg and not h.value, (field, rc, msg)
    for field, channels, kw in (("channels", 0, {}), ("channels", 8, {}), ("channels", N.AOV_NORMAL | 64, {}),
                                ("reserved0", N.AOV_DEPTH, dict(reserved0=1))):
        rc, msg, h = _aov_create(channels, **kw)
        assert rc == N.RTW_ERR_INVALID_ARGUMENT and field in msg and not h.value, (field, rc, msg)
    rc, msg, h = _aov_create(N.AOV_ALBEDO | N.AOV_NORMAL | N.AOV_DEPTH)
    assert rc == N.RTW_ERR_INVALID_ARGUMENT and "world" in msg and not h.value  # good params, no world
    L = N.lib()
    assert L.rtw_aov_add(None, 1, None) == N.RTW_ERR_INVALID_ARGUMENT
    assert L.rtw_aov_resolve(None, N.AOV_ALBEDO, None, None) == N.RTW_ERR_INVALID_ARGUMENT
    assert L.rtw_aov_hits(None, None, None) == N.RTW_ERR_INVALID_ARGUMENT
    assert L.rtw_aov_get_info(None, None) == N.RTW_ERR_INVALID_ARGUMENT
    assert L.rtw_aov_release(None) == N.RTW_OK
    assert C.sizeof(N.AovInfo) == 40
    # the demodulated filter: the existing refusals, and shapes that are not the frame's
    W, H = 6, 5
    color, se, guide = D.synthetic((W, H), 2, 3)
    albedo = np.ones((W * H, 3), f32)
    out = np.zeros((W * H, 3), f32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    good = N.DenoiseParams(W, H, 3, 2, 1.5, 0.35, 0, 0)
    assert L.rtw_denoise_host_albedo(C.byref(good), ptr(color), ptr(se), ptr(guide), ptr(albedo), ptr(out), None) == 0
    for field, value in (("width", 1), ("iterations", 7), ("guide_channels", 5), ("sigma_l", 0.0), ("reserved1", 2)):
        bad = N.DenoiseParams(W, H, 3, 2, 1.5, 0.35, 0, 0)
        setattr(bad, field, value)
        rc = L.rtw_denoise_host_albedo(C.byref(bad), ptr(color), ptr(se), ptr(guide), ptr(albedo), ptr(out), None)
        assert rc == N.RTW_ERR_INVALID_ARGUMENT and field.encode() in L.rtw_last_error(), field
    assert L.rtw_denoise_host_albedo(C.byref(good), None, ptr(se), ptr(guide), ptr(albedo), ptr(out), None) == 1
    assert L.rtw_denoiser_run_albedo(None, C.byref(good), None, None, None, None, None, None, None) == 1
    with pytest.raises(ValueError, match="albedo"):
        R.denoise_host(R.Size2i(W, H), color, se, guide, albedo=albedo[:-1])
    with pytest.raises(ValueError, match="albedo"):
        R.denoise_host(R.Size2i(W, H), color, se, guide, albedo=np.ones((W * H, 4), f32))
    with pytest.raises(ValueError, match="channels"):
        R.AovAccumulator(None, R.Size2i(W, H), seed=1, channels=("albedo", "colour"))
    with pytest.raises(ValueError, match="channels"):
        R.AovAccumulator(None, R.Size2i(W, H), seed=1, channels=())


def test_header_compiles_as_c99():
    src = ('#include "rtw.h"\n#include "rtw_denoise.h"\n'
           "int main(void){rtw_aov* a = 0; rtw_aov_info i; rtw_render_params p = {0}; rtw_denoise_params d = {2, 2, 1, 0, 1.5f, 0.35f, 0, 0};\n"
           "return rtw_aov_create(0, &p, RTW_AOV_ALBEDO | RTW_AOV_NORMAL | RTW_AOV_DEPTH, &a) + rtw_aov_add(a, 1, 0)\n"
           "+ rtw_aov_resolve(a, RTW_AOV_DEPTH, 0, 0) + rtw_aov_hits(a, 0, 0) + rtw_aov_get_info(a, &i) + rtw_aov_release(a)\n"
           "+ rtw_denoiser_run_albedo(0, &d, 0, 0, 0, 0, 0, 0, 0) + rtw_denoise_host_albedo(&d, 0, 0, 0, 0, 0, 0)\n"
           "+ rtw_denoise_image_albedo(&d, 0, 0, 0, 0, 0, 0, 0) + (int)sizeof(rtw_aov_info);}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)


# ---- 4. quality ---------------------------------------------------------------------------------------
def test_demodulation_turns_earth_mapped_into_a_gain(worlds):
    """earth_mapped 96 x 54: oracle colour at 8 spp (seed 31), Normals guide at 8 spp, twin albedo at 64 spp (seed
    31), reference 512 spp (seed 977), MSE over all pixels.  The demodulated MSE must be below the noisy frame's and
    below today's filter's (measured, mean over pixels and channels: 0.000209 noisy, 0.000301 filtered, 0.000109
    demodulated: 0.52x and 0.36x)."""
    world, w, h, spp = worlds("earth_mapped"), 96, 54, 8
    size = R.Size2i(w, h)
    p = R.render_params(size, spp, 50, seed=31)
    with np.errstate(all="ignore"):
        total = np.zeros((w * h, 3), f32)
        sq = np.zeros((w * h, 3), f32)
        for s in range(spp):  # in sample order, as the accumulator adds them
            c = np.stack([O.sample_color(world, p, i % w, i // w, s) for i in range(w * h)])
            total = total + c
            sq = sq + c * c
        nf = f32(spp)
        mean = total / nf
        d = sq - total * mean
        se = np.sqrt(np.where(d < 0, f32(0), d) / f32(spp - 1) / nf)
    assert_bit_identical(mean, O.render(world, p), "the sums are the frame's")
    normals = O.render(world, R.render_params(size, spp, 50, R.RenderMode.Normals, seed=31))
    albedo = A.twin_albedo(world, size, 64, 31)
    ref = O.render(world, R.render_params(size, 512, 50, seed=977)).astype(np.float64)
    today = R.denoise_host(size, mean, se, normals)
    demod = R.denoise_host(size, mean, se, normals, albedo=albedo)
    assert_bit_identical(demod, A.denoise_albedo(mean, se, normals, albedo, (w, h))[0], "host twin on the oracle frame")

    def mse(img):
        return float(((img.astype(np.float64) - ref) ** 2).mean())

    noisy, filtered, demodulated = mse(mean), mse(today), mse(demod)
    print(f"earth_mapped 96x54 8 spp MSE: noisy {noisy:.6f} today's filter {filtered:.6f} demodulated {demodulated:.6f} "
          f"({demodulated / noisy:.2f}x, {demodulated / filtered:.2f}x)")
    assert demodulated < noisy
    assert demodulated < filtered


# ---- 5. the stand-alone program ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("denoise_albedo")
    plain, san = str(d / "denoise_albedo_check"), str(d / "denoise_albedo_check_san")
    subprocess.run(["gcc", "-O2", *FLAGS, "-o", plain, SRC, "-lm"], check=True)
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *FLAGS, "-o", san,
                    SRC, "-lm"], check=True)
    return plain, san


def fnv(a: np.ndarray) -> int:
    u = np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)).astype("<u4")
    h = 0xCBF29CE484222325
    for b in u.tobytes():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_program_on_the_same_cases(programs, tmp_path, sanitized):
    exe = programs[1 if sanitized else 0]
    path = str(tmp_path / "case.bin")
    for case in CASES:
        size, gc, iterations, seed = case
        color, se, guide = D.synthetic(size, gc, seed)
        albedo = A.synthetic_albedo(size, seed)
        for has_albedo, alias in ((1, 0), (1, 1), (0, 0)):
            if has_albedo:
                want, want_var = A.denoise_albedo(color, se, guide, albedo, size, iterations)
            else:
                want, want_var = D.denoise(color, se, guide, size, iterations)
            with open(path, "wb") as f:
                f.write(struct.pack("<6i2f", size[0], size[1], iterations, gc, has_albedo, alias, 1.5, 0.35))
                f.write(color.tobytes())
                f.write(se.tobytes())
                if gc:
                    f.write(guide.tobytes())
                if has_albedo:
                    f.write(albedo.tobytes())
            out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, (case_id(case), out.stdout[-2000:], out.stderr[-2000:])
            lines = out.stdout.split("\n")
            assert lines[0] == f"rc 0 pixels {size[0] * size[1]}", lines[0]
            assert lines[1] == f"sum {fnv(want.reshape(-1)):016x} {fnv(want_var):016x}", (case_id(case), has_albedo, alias)
