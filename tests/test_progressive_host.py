"""Progressive accumulation, the parts that need no GPU: the checkpoint file (AccumState), the world
fingerprint a checkpoint is tied to, and the layout of rtw_accum_info."""
import ctypes as C
import os
import pickle
import subprocess
import zipfile

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.progressive import AccumState, world_fingerprint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADER_FIELDS = [n for n, _ in N.AccumInfo._fields_]


def _state(moments: bool) -> AccumState:
    rng = np.random.default_rng(3)
    slots = 7 * 64
    # every bit pattern class: NaN payloads, infinities, negative zero, subnormals
    sums = rng.integers(0, 2**32, (slots, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    sums[0] = (np.float32("nan"), np.float32("-inf"), np.float32(-0.0))
    squares = rng.random((slots, 3), dtype=np.float32) if moments else None
    return AccumState(version=1, flags=1 if moments else 0, width=50, height=30, tile_width=8, tile_height=8,
                      part_index=1, part_count=3, max_depth=-7, render_mode=1, samples=4000000000, reserved=0,
                      seed=0xFEDCBA9876543210, world_fingerprint=0x8000000000000001, slots=slots, sums=sums,
                      squares=squares)


@pytest.mark.parametrize("moments", [False, True])
def test_accum_state_round_trip_keeps_every_bit(tmp_path, moments):
    s = _state(moments)
    path = tmp_path / "frame.npz"
    s.save(path)
    t = AccumState.load(path)
    for n in HEADER_FIELDS:
        assert getattr(t, n) == getattr(s, n), n
    assert t.sums.dtype == np.float32 and t.sums.shape == s.sums.shape
    assert (t.sums.view(np.uint32) == s.sums.view(np.uint32)).all()
    if moments:
        assert (t.squares.view(np.uint32) == s.squares.view(np.uint32)).all()
    else:
        assert t.squares is None
    # plain arrays only: the file loads without pickle support
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(HEADER_FIELDS) | ({"sums", "squares"} if moments else {"sums"})
        for n in z.files:
            assert z[n].dtype != object


def test_accum_state_refuses_a_pickled_object(tmp_path):
    s = _state(False)
    path = tmp_path / "frame.npz"
    s.save(path)
    # an extra entry holding a pickled object
    with np.load(path, allow_pickle=False) as z:
        arrays = {n: z[n] for n in z.files}
    arrays["extra"] = np.array([{"a": 1}], dtype=object)
    bad = tmp_path / "bad.npz"
    np.savez(bad, **arrays)
    with pytest.raises(ValueError):
        AccumState.load(bad)
    # ... and a known entry replaced by one
    arrays.pop("extra")
    arrays["sums"] = np.array([pickle.dumps(1)], dtype=object)
    bad2 = tmp_path / "bad2.npz"
    np.savez(bad2, **arrays)
    with pytest.raises(ValueError):
        AccumState.load(bad2)
    # a missing field is refused too
    with zipfile.ZipFile(path) as zin, zipfile.ZipFile(tmp_path / "short.npz", "w") as zout:
        for item in zin.infolist():
            if item.filename != "seed.npy":
                zout.writestr(item, zin.read(item.filename))
    with pytest.raises(ValueError):
        AccumState.load(tmp_path / "short.npz")


def test_world_fingerprint_of_demo_worlds(assets):
    names = ["final_scene1", "cornell_box", "simple_plane", "defocus_blur"]
    first = {n: world_fingerprint(R.demo_world(n, assets)) for n in names}
    again = {n: world_fingerprint(R.demo_world(n, assets)) for n in names}
    assert first == again  # two builds of the same world
    assert len(set(first.values())) == len(names)  # pairwise distinct
    assert all(0 < v < 2**64 for v in first.values())


def _builder_world(radius=0.5, fov=40.0, texel=128):
    wb = R.WorldBuilder()
    img = np.full((4, 6, 3), 200, np.uint8)
    img[2, 3, 1] = texel
    tex = wb.texture_image_rgb8(img)
    group = wb.new_group()
    group.add(wb.new_obj_sphere(radius, wb.material_lambert(tex)).translate((0.0, 0.0, -2.0)).build())
    group.add(wb.new_obj_sphere(100.0, wb.material_lambert_solid((0.5, 0.5, 0.5))).translate((0.0, -100.5, -2.0)).build())
    cam = R.Camera.build().vertical_fov(fov, 1.5).position((0.0, 0.0, 1.0)).look_at((0.0, 1.0, 0.0), (0.0, 0.0, -2.0)).build()
    return group.build().finish(wb, R.BackgroundColor.sky(), cam)


def test_world_fingerprint_follows_the_contents():
    base = world_fingerprint(_builder_world())
    assert base == world_fingerprint(_builder_world())
    assert base != world_fingerprint(_builder_world(radius=0.5000001))  # one sphere radius
    assert base != world_fingerprint(_builder_world(fov=40.001))  # camera floats
    assert base != world_fingerprint(_builder_world(texel=129))  # one texel
    # one camera float changed in place: nothing else differs
    w = _builder_world()
    w.raw.camera.lens_radius = np.nextafter(np.float32(w.raw.camera.lens_radius), np.float32(1.0))
    assert base != world_fingerprint(w)
    assert N.lib().rtw_world_fingerprint(None, None) == N.RTW_ERR_INVALID_ARGUMENT


def test_accum_info_layout_in_c():
    """rtw.h compiles as C11 and rtw_accum_info has no padding: its size is the sum of its fields, and the
    ctypes mirror agrees field by field."""
    fields = {"version": 4, "flags": 4, "width": 4, "height": 4, "tile_width": 4, "tile_height": 4, "part_index": 4,
              "part_count": 4, "max_depth": 4, "render_mode": 4, "samples": 4, "reserved": 4, "seed": 8,
              "world_fingerprint": 8, "slots": 8}
    assert list(fields) == HEADER_FIELDS
    total = sum(fields.values())
    asserts = "\n".join(
        f'_Static_assert(sizeof(((rtw_accum_info*)0)->{n}) == {size}, "{n} size");\n'
        f'_Static_assert(offsetof(rtw_accum_info, {n}) == {getattr(N.AccumInfo, n).offset}, "{n} offset");'
        for n, size in fields.items())
    src = ('#include <stddef.h>\n#include "rtw.h"\n'
           f'_Static_assert(sizeof(rtw_accum_info) == {total}, "rtw_accum_info is padded");\n{asserts}\n'
           "int main(void){rtw_accum* a = 0; return rtw_accum_release(a) + (int)RTW_ACCUM_MOMENTS;}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)
    assert C.sizeof(N.AccumInfo) == total
    for n, size in fields.items():
        assert getattr(N.AccumInfo, n).size == size
