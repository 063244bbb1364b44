"""What a camera ray hits on the device, against plain f64 mathematics (second axis).

Two kernels answer: the first-hit AOV pass (R.AovAccumulator, one add of one sample: albedo, normal, depth, hits;
its sphere, rect and triangle fast records, per-tile leaf lists and the generic leaf) and the megakernel's walk in
RenderMode.Normals (R.render).  Both are compared, pixel by pixel, with tests/first_hit_ref.cast on the rays
tests/test_first_hit_host.py generates, under the same margins and the same constants K_q (nothing added): hits is
the caster's hit or miss on every compared pixel, depth is t, 2 normal - 1 is the normal, albedo is the albedo.  The
four planes are also bit-identical to the oracle's, so a tolerance failure here that the host test passes can only
be a kernel bug.  On a failure the message names the pixel, the ray, the caster's leaf, t, margins and scales, and
the kernel's values."""
import numpy as np
import pytest

import raytracinginaweekend_amd as R
from tests import first_hit_check as Ck
from tests import first_hit_worlds as FW
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

SEEDS = (1, 2)
DEPTH = 50


def device_planes(world, seed):
    aov = R.AovAccumulator(world, FW.SIZE, seed=seed)
    aov.add(1)
    planes = dict(albedo=aov.albedo(), normal=aov.normal(), depth=aov.depth(), hits=aov.hits())
    aov.release()
    return planes


def check(name, world, seed, tag):
    want = Ck.oracle_planes(name, world, FW.SIZE, seed)
    left = Ck.assert_cases(name, Ck.camera_cast(name, world, FW.SIZE, seed))
    planes = device_planes(world, seed)
    worst = Ck.compare_planes(name, world, FW.SIZE, seed, planes, f"world {name} seed {seed} AOV pass{tag}")
    print(f"{name} seed {seed}{tag}: left out {100 * left:.2f} %, aov_kernel worst (U S) {worst}")
    for k in ("albedo", "normal", "depth"):
        assert_bit_identical(planes[k], want[k], f"{name} seed {seed}{tag} {k} against the oracle")
    assert (planes["hits"] == want["hits"]).all(), f"{name} seed {seed}{tag} hits against the oracle"
    frame = R.render(FW.SIZE, 1, 1, DEPTH, world, R.RenderMode.Normals, seed=seed)
    worst = Ck.compare_planes(name, world, FW.SIZE, seed, dict(normal=frame),
                              f"world {name} seed {seed} RenderMode.Normals{tag}")
    print(f"{name} seed {seed}{tag}: render_kernel worst (U S) {worst}")
    assert_bit_identical(frame, want["normal"], f"{name} seed {seed}{tag} Normals frame against the oracle")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", FW.NAMES)
def test_first_hit(worlds, name, seed):
    check(name, FW.world(name, worlds), seed, "")


@pytest.mark.parametrize("seed", SEEDS)
def test_first_hit_without_leaf_lists(worlds, monkeypatch, seed):
    """final_scene1 once more with RTW_PRIMARY_LISTS=0: every camera ray takes the walk, so both the list step and
    the walk are pinned."""
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "0")
    check("D", FW.world("D", worlds), seed, " (no leaf lists)")
