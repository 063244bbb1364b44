"""The preview denoiser, the parts that need no GPU: the host twin (rtw_denoise_host, include/rtw_denoise.h)
against the numpy restatement (tests/denoise_ref.py) bit for bit, left-out pixels, the refusals, the C
declarations, the filter's quality on an oracle frame, and the stand-alone program
tests/native/denoise_check.c, which runs the same header loop on the same cases -- built once plain and once
with -fsanitize=address,undefined, and run alone."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from tests import denoise_ref as D
from tests.parity import assert_bit_identical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "denoise_check.c")
FLAGS = ["-std=c11", "-ffp-contract=off", "-fno-fast-math"]
f32 = np.float32

CASES, case_id = D.CASES, D.case_id


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_host_twin_against_numpy(case):
    size, gc, iterations, seed = case
    color, se, guide = D.synthetic(size, gc, seed)
    want, want_var = D.denoise(color, se, guide, size, iterations, 1.5, 0.35)
    got, got_var = R.denoise_host(R.Size2i(*size), color, se, guide, iterations=iterations, variance=True)
    assert got.dtype == np.float32 and got.shape == (size[0] * size[1], 3) and got_var.shape == (size[0] * size[1],)
    assert_bit_identical(got, want, f"image {case_id(case)}")
    assert_bit_identical(got_var, want_var, f"variance {case_id(case)}")
    if size[0] * size[1] >= 24:  # the case exercises both kinds of pixel, and the filter did something
        assert np.isnan(want_var).any() and np.isfinite(want_var).any()
        assert (got.view(np.uint32) != color.view(np.uint32)).any()
    # the variance output is optional, and other sigmas take the same path
    assert_bit_identical(R.denoise_host(R.Size2i(*size), color, se, guide, iterations=iterations), want, "no variance")
    if seed % 100 == 0:
        want2, _ = D.denoise(color, se, guide, size, iterations, 0.7, 1.25)
        got2 = R.denoise_host(R.Size2i(*size), color, se, guide, iterations=iterations, sigma_l=0.7, sigma_g=1.25)
        assert_bit_identical(got2, want2, "other sigmas")


def test_left_out_pixels_pass_through_and_are_read_by_nobody():
    size, gc = (37, 23), 3
    color, se, guide = D.synthetic(size, gc, 7)
    out, var = R.denoise_host(R.Size2i(*size), color, se, guide, iterations=4, variance=True)
    left = np.isnan(var)
    assert 10 < left.sum() < left.size // 2
    # bit for bit as it went in, NaN payloads and all
    assert (out.view(np.uint32)[left] == color.view(np.uint32)[left]).all()
    # other garbage in the left-out pixels' colours: no other output pixel changes
    rng = np.random.default_rng(1)
    color2 = color.copy()
    garbage = rng.integers(0, 2**32, (int(left.sum()), 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):  # (left out for its colour: stays so)
        keep_out = ~np.isfinite((color[left, 0] + color[left, 1]) + color[left, 2])
    garbage[keep_out, 0] = np.nan
    color2[left] = garbage
    out2, var2 = R.denoise_host(R.Size2i(*size), color2, se, guide, iterations=4, variance=True)
    assert (np.isnan(var2) == left).all()
    assert (out2.view(np.uint32)[~left] == out.view(np.uint32)[~left]).all()
    assert (var2.view(np.uint32)[~left] == var.view(np.uint32)[~left]).all()
    assert (out2.view(np.uint32)[left] == color2.view(np.uint32)[left]).all()


def _host_rc(p, color, se, guide, out):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    rc = N.lib().rtw_denoise_host(None if p is None else C.byref(p), ptr(color), ptr(se), ptr(guide), ptr(out), None)
    return rc, (N.lib().rtw_last_error() or b"").decode()


def test_refusals():
    W, H = 6, 5
    color, se, guide = D.synthetic((W, H), 2, 3)
    out = np.zeros((W * H, 3), f32)

    def params(**kw):
        v = dict(width=W, height=H, iterations=3, guide_channels=2, sigma_l=1.5, sigma_g=0.35, reserved0=0, reserved1=0)
        v.update(kw)
        return N.DenoiseParams(**v)

    assert _host_rc(params(), color, se, guide, out)[0] == N.RTW_OK
    bad = [("width", 1), ("height", 1), ("width", 0), ("height", -3), ("iterations", 0), ("iterations", 7),
           ("iterations", -1), ("guide_channels", -1), ("guide_channels", 5), ("sigma_l", 0.0), ("sigma_l", -1.0),
           ("sigma_l", float("nan")), ("sigma_l", float("inf")), ("sigma_g", 0.0), ("sigma_g", -0.35),
           ("sigma_g", float("nan")), ("sigma_g", float("inf")), ("reserved0", 1), ("reserved1", -1)]
    for field, value in bad:
        rc, msg = _host_rc(params(**{field: value}), color, se, guide, out)
        assert rc == N.RTW_ERR_INVALID_ARGUMENT and field in msg, (field, value, rc, msg)
    for which, args in (("params", (None, color, se, guide, out)), ("color", (params(), None, se, guide, out)),
                        ("std_err", (params(), color, None, guide, out)), ("guide", (params(), color, se, None, out)),
                        ("out", (params(), color, se, guide, None))):
        rc, msg = _host_rc(*args)
        assert rc == N.RTW_ERR_INVALID_ARGUMENT and "null" in msg and which in msg, (which, rc, msg)
    # a null guide is fine without guide channels
    assert _host_rc(params(guide_channels=0), color, se, None, out)[0] == N.RTW_OK
    # the device entry points refuse the same before they touch a GPU
    h = C.c_void_p()
    assert N.lib().rtw_denoiser_create(0, 1, 8, C.byref(h)) == N.RTW_ERR_INVALID_ARGUMENT
    assert b"width" in N.lib().rtw_last_error()
    assert N.lib().rtw_denoiser_create(0, 8, 1, C.byref(h)) == N.RTW_ERR_INVALID_ARGUMENT
    assert b"height" in N.lib().rtw_last_error()
    assert N.lib().rtw_denoiser_create(0, 8, 8, None) == N.RTW_ERR_INVALID_ARGUMENT
    assert N.lib().rtw_denoiser_run(None, C.byref(params()), None, None, None, None, None, None) == N.RTW_ERR_INVALID_ARGUMENT
    assert b"null" in N.lib().rtw_last_error()
    assert N.lib().rtw_denoiser_release(None) == N.RTW_OK
    # and the Python face refuses shapes that are not the frame's
    with pytest.raises(ValueError, match="color"):
        R.denoise_host(R.Size2i(W, H), color[:-1], se, guide)
    with pytest.raises(ValueError, match="guide"):
        R.denoise_host(R.Size2i(W, H), color, se, np.zeros((W * H, 5), f32))


def test_header_compiles_as_c99():
    src = ('#include <stdio.h>\n#include "rtw.h"\n#include "rtw_denoise.h"\n'
           "int main(void){rtw_denoiser* d = 0; rtw_denoise_params p = {2, 2, 1, 0, 1.5f, 0.35f, 0, 0};\n"
           "return rtw_denoiser_create(0, 2, 2, &d) + rtw_denoiser_run(d, &p, 0, 0, 0, 0, 0, 0) + rtw_denoiser_release(d)\n"
           "+ rtw_denoise_host(&p, 0, 0, 0, 0, 0) + rtw_denoise_image(&p, 0, 0, 0, 0, 0, 0) + (int)sizeof(rtw_denoise_rec);}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)
    assert C.sizeof(N.DenoiseParams) == 32


def test_quality_on_the_oracle(worlds):
    """cornell_box 64 x 64 at 8 spp (seed 31) with the Normals guide, against the oracle at 2048 spp (seed 977):
    rel = mean over the pixels of |x - ref|^2 / (|ref|^2 + 0.01).  With the defaults the denoised frame's rel
    must be at most half the noisy frame's."""
    world, w, h, spp = worlds("cornell_box"), 64, 64, 8
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
    assert mean.dtype == se.dtype == np.float32
    assert_bit_identical(mean, O.render(world, p), "the sums are the frame's")
    normals = O.render(world, R.render_params(size, spp, 50, R.RenderMode.Normals, seed=31))
    ref = O.render(world, R.render_params(size, 2048, 50, seed=977)).astype(np.float64)
    den = R.denoise_host(size, mean, se, normals)
    assert_bit_identical(den, D.denoise(mean, se, normals, (w, h))[0], "host twin on the oracle frame")

    def rel(img):
        e = ((img.astype(np.float64) - ref) ** 2).sum(axis=1) / ((ref ** 2).sum(axis=1) + 0.01)
        ok = np.isfinite(e)
        return float(e[ok].mean()), int((~ok).sum())

    (noisy, n_bad), (clean, c_bad) = rel(mean), rel(den)
    print(f"cornell_box 64x64 8 spp: rel noisy {noisy:.4f} denoised {clean:.4f} (non-finite pixels {n_bad}, {c_bad})")
    assert n_bad == c_bad
    assert clean <= 0.5 * noisy


# ---- the stand-alone program ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("denoise")
    plain, san = str(d / "denoise_check"), str(d / "denoise_check_san")
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
        want, want_var = D.denoise(color, se, guide, size, iterations, 1.5, 0.35)
        with open(path, "wb") as f:
            f.write(struct.pack("<4i2f", size[0], size[1], iterations, gc, 1.5, 0.35))
            f.write(color.tobytes())
            f.write(se.tobytes())
            if gc:
                f.write(guide.tobytes())
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (case_id(case), out.stdout[-2000:], out.stderr[-2000:])
        lines = out.stdout.split("\n")
        assert lines[0] == f"rc 0 pixels {size[0] * size[1]}", lines[0]
        assert lines[1] == f"sum {fnv(want.reshape(-1)):016x} {fnv(want_var):016x}", case_id(case)
