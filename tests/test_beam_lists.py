"""The primary rays' per-tile leaf lists (include/rtw_beam.h) may leave a leaf out
of a tile's list only if no camera ray of the tile can make the leaf's test accept.  The stand-alone
program tests/native/beam_lists_check.c draws each tile's rays (256 random ones plus the extremes) with
a host restatement of camera_ray and runs the reference's sphere test on every leaf: every accepting leaf
must be listed.  The cap is raised to the leaf count, so no tile falls back to the walk, and the lists
must prove something: some tile empty, some listed, mean length below a quarter of the leaves.

The program is built a second time with -fsanitize=address,undefined and run alone."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "beam_lists_check.c")
FLAGS = ["-std=c11", "-ffp-contract=off", "-fno-fast-math"]
WORLDS = ["final_scene1", "defocus_blur"]
FRAMES = [(480, 270), (50, 37)]  # the second: edge tiles in both directions
TILES = [(8, 8), (16, 4)]


def _dump(world, path) -> int:
    """The camera and the plain-sphere leaf records ({c, r} per leaf) as the program reads them."""
    sph = world.spheres()
    leaves = world.leaves()
    assert all(l.geom_kind == N.GEOM_SPHERE and l.flags == 0 for l in leaves)
    fast = np.stack([sph[l.geom_index] for l in leaves]).astype(np.float32)
    with open(path, "wb") as f:
        f.write(bytes(world.raw.camera))
        f.write(struct.pack("<i", len(leaves)))
        f.write(fast.tobytes())
    return len(leaves)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("beam")
    plain, san = str(d / "blc"), str(d / "blc_san")
    subprocess.run(["gcc", "-O2", *FLAGS, "-o", plain, SRC, "-lm"], check=True)
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *FLAGS, "-o", san,
                    SRC, "-lm"], check=True)
    return plain, san


def _run(exe, dump, w, h, tw, th):
    out = subprocess.run([exe, dump, str(w), str(h), str(tw), str(th), "256"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    m = re.search(r"tiles (\d+) listed (\d+) empty (\d+) walked (\d+) leaves (\d+) mean_len ([\d.]+) tests (\d+) "
                  r"accepted (\d+) violations (\d+)", out.stdout)
    assert m, out.stdout
    return dict(zip(("tiles", "listed", "empty", "walked", "leaves", "mean_len", "tests", "accepted", "violations"),
                    [float(x) if "." in x else int(x) for x in m.groups()]))


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("frame", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", WORLDS)
def test_every_accepting_leaf_is_listed(worlds, programs, tmp_path, name, frame, tile):
    dump = str(tmp_path / "world.bin")
    n = _dump(worlds(name), dump)
    r = _run(programs[0], dump, *frame, *tile)
    print(name, frame, tile, r)
    assert r["violations"] == 0 and r["walked"] == 0 and r["leaves"] == n
    assert r["accepted"] > 0  # the rays do hit leaves
    assert r["listed"] > 0
    if name == "final_scene1":
        # the lists prove something: well below the leaf count everywhere, and sky tiles are empty.  (At
        # 50x37 an 8x8 tile spans a sixth of the frame and none is all sky; defocus_blur's ground fills its
        # frame, so none of its tiles is empty at any size.)
        assert r["mean_len"] < n / 4
        if frame == (480, 270):
            assert r["empty"] > 0


@pytest.mark.parametrize("name", WORLDS)
def test_sanitized_program_runs_clean(worlds, programs, tmp_path, name):
    """The address / undefined-behaviour build of the same program, on the small frame with edge tiles."""
    dump = str(tmp_path / "world.bin")
    _dump(worlds(name), dump)
    for tile in TILES:
        r = _run(programs[1], dump, 50, 37, *tile)
        assert r["violations"] == 0 and r["walked"] == 0


def test_library_builder_matches_the_header(worlds):
    """rtw_primary_lists_host (librtw.so's host entry, no GPU) against the cap: a tile whose list would exceed
    it takes the walk, every other tile's list is the uncapped list, and a world with other leaves is refused."""
    world = worlds("final_scene1")
    n = world.raw.leaf_count
    p = R.render_params(R.Size2i(160, 90), 1, 1)
    tiles = 20 * 12
    i32p = C.POINTER(C.c_int32)

    def lists(cap):
        count = np.zeros(tiles, np.int32)
        lst = np.full((tiles, cap), -7, np.int32)
        N.check(N.lib().rtw_primary_lists_host(world.ptr(), C.byref(p), cap, count.ctypes.data_as(i32p),
                                               lst.ctypes.data_as(i32p)))
        return count, lst

    full_c, full_l = lists(n)
    cap_c, cap_l = lists(4)
    assert (full_c >= 0).all() and (full_c > 4).any() and (full_c <= 4).any()
    for t in range(tiles):
        if full_c[t] > 4:
            assert cap_c[t] == -1
        else:
            assert cap_c[t] == full_c[t]
            assert (cap_l[t, : cap_c[t]] == full_l[t, : full_c[t]]).all()
        assert (np.diff(full_l[t, : full_c[t]]) > 0).all()  # leaf order
    rc = N.lib().rtw_primary_lists_host(worlds("suzanne").ptr(), C.byref(p), 4, cap_c.ctypes.data_as(i32p),
                                        cap_l.ctypes.data_as(i32p))
    assert rc == N.RTW_ERR_UNSUPPORTED
