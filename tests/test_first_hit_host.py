"""What a ray hits and what is read there, oracle against plain f64 mathematics (second axis).

The oracle (oracle/rtw_oracle.c: rtw_oracle_camera_ray, rtw_oracle_scene_hit, the emissive twin for the albedo) on
one side, tests/first_hit_ref.cast on the other: a brute-force numpy float64 caster that shares no code, no f32 and
no tree walk with it.  (a) the camera rays of 93 x 54 frames, seeds 1..3, over the worlds of
tests/first_hit_worlds.py; (b) bounce-like rays from the compared hits and from random points inside the world's
bounds, which reach the inside roots, exit planes and back faces no camera sees; (c) Camera::ray alone from the
rtw_camera fields.  Hit or miss, front_face and the material are exact on every compared ray; t, position, normal,
(u, v) and albedo hold within K_q U S_q (tests/first_hit_ref.py, where the constants and their measurement stand).
tests/test_gpu_first_hit.py asserts the same of the kernels, and their bit identity with the oracle."""
import numpy as np
import pytest

from tests import first_hit_check as Ck
from tests import first_hit_ref as F
from tests import first_hit_worlds as FW

SEEDS = (1, 2, 3)
f32 = np.float32

# What the bounce leg must add to the cameras' cases: at least MIN_RAYS compared rays each, over the three seeds.
BOUNCE_CASES = {
    "A": {("sphere", "front", "plain"), ("sphere", "back", "plain"), ("sphere", "back", "animation")},
    "B": {("rect_xy", "front", "plain"), ("rect_xy", "back", "plain"), ("rect_xz", "front", "plain"),
          ("rect_xz", "back", "plain"), ("rect_yz", "front", "plain"), ("rect_yz", "back", "plain"),
          ("box", "back", "plain"), ("box", "back", "transform(+)"), ("box", "back", "transform(-)"),
          ("box", "front", "transform(+)"), ("box", "front", "transform(-)"),
          ("box", "back", "animation+transform(+)")},
    "C": {("triangle", "front", "plain"), ("triangle", "back", "plain")},
    "D": {("sphere", "front", "plain"), ("sphere", "back", "plain")},
}


def oracle_record(world, rays):
    got = Ck.oracle_hits(world, *rays[:3])
    got["albedo"] = Ck.oracle_albedo(world, *rays[:3])
    return got


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", FW.NAMES)
def test_camera_rays(worlds, name, seed):
    world = FW.world(name, worlds)
    rays = Ck.camera_rays(name, world, FW.SIZE, seed)
    res = Ck.camera_cast(name, world, FW.SIZE, seed)
    left = Ck.assert_cases(name, res)
    worst = Ck.compare(res, rays, oracle_record(world, rays), f"world {name} seed {seed}", FW.SIZE.width)
    print(f"{name} seed {seed}: left out {100 * left:.2f} %, worst (U S) {worst}")


@pytest.mark.parametrize("seed", SEEDS[:2])
@pytest.mark.parametrize("name", FW.NAMES)
def test_oracle_planes(worlds, name, seed):
    """The comparison tests/test_gpu_first_hit.py makes of the device's planes, made of the oracle's here: the twin's
    albedo, the Normals frame (2 normal - 1), depth and hits of a one-sample frame.  The device's planes are
    bit-identical to these, so the constants are measured with this encoding in them."""
    world = FW.world(name, worlds)
    planes = Ck.oracle_planes(name, world, FW.SIZE, seed)
    worst = Ck.compare_planes(name, world, FW.SIZE, seed, planes, f"world {name} seed {seed}, the oracle's planes")
    print(f"{name} seed {seed}: planes worst (U S) {worst}")


# A ray that starts on a surface has a root at t = 0 in exact arithmetic.  The f32 root's error there is K_t U S_t
# with S_t >= surface / cos (first_hit_ref: `surface` is 4 r + 2 |c| of a sphere, 2 |p| of a plane hit, cos the angle
# between the ray and the normal), and the `tstart` margin (twice K_t) leaves the ray out where that reaches the start
# 0.001: for |cos| < UNDECIDED = 2 K_t U surface / 0.001, which for a random direction is a share UNDECIDED of the
# rays.  Hits whose share would exceed 0.15 give no bounce origin (the 100 and 1000 unit ground spheres: 1 and above;
# A's enclosing sphere: 0.32); a random interior point stands in, so the ray count stays.  0.15 on at most half of the
# rays keeps this cause below 7.5 points of the 10 % cap.
MAX_UNDECIDED = 0.15


def bounce_rays(name, world, seed):
    """One ray from every compared camera hit whose surface can start a decidable ray (the caster's position,
    rounded to f32) in a random direction at the camera ray's time, and rays from random points inside the root's
    box at random shutter times: as many again, plus one for every hit that gave no origin."""
    rays = Ck.camera_rays(name, world, FW.SIZE, seed)
    res = Ck.camera_cast(name, world, FW.SIZE, seed)
    rng = np.random.default_rng(1000 + seed)
    m = res["compared"] & res["hit"]
    n = int(m.sum())
    m &= 2 * F.K["t"] * F.U * res["surface"] / F.T_START <= MAX_UNDECIDED
    k = int(m.sum())
    o1, t1 = res["position"][m].astype(f32), rays[2][m]
    tb = F.Tables(world)
    root = tb.nodes[tb.root]
    lo, hi = np.array(list(root["min"]), np.float64), np.array(list(root["max"]), np.float64)
    o2 = rng.uniform(lo, hi, (2 * n - k, 3)).astype(f32)
    cam = world.raw.camera
    t2 = rng.uniform(cam.time0, max(cam.time1, np.nextafter(f32(cam.time0), f32(np.inf))), 2 * n - k).astype(f32)
    d = rng.normal(size=(2 * n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(f32)  # unit to f32 rounding
    return np.concatenate([o1, o2]), d, np.concatenate([t1, t2]), k


@pytest.mark.parametrize("name", sorted(BOUNCE_CASES))
def test_bounce_like_rays(worlds, name):
    world = FW.world(name, worlds)
    total = {}
    for seed in SEEDS:
        *rays, surface = bounce_rays(name, world, seed)
        res = F.cast(world, *rays)
        worst = Ck.compare(res, rays, oracle_record(world, rays), f"world {name} bounce rays of seed {seed}")
        cases, _ = Ck.case_counts(res)
        for k, v in cases.items():
            total[k] = total.get(k, 0) + v
        left = 1 - res["compared"].mean()
        print(f"{name} seed {seed}: {len(rays[0])} rays ({surface} from surfaces), left out {100 * left:.2f} %, "
              f"{F.left_out_by(res)}, misses {int((~res['hit'] & res['compared']).sum())}, worst (U S) {worst}")
        assert left <= 0.10, f"world {name} seed {seed}: {100 * left:.2f} % of the bounce rays left out"
        assert surface >= FW.MIN_RAYS  # (the leg keeps rays that start on surfaces)
    print(name, total)
    for c in BOUNCE_CASES[name]:
        assert total.get(c, 0) >= FW.MIN_RAYS, f"world {name}: bounce case {c} has {total.get(c, 0)} compared rays"


def test_triangle_edge_on_ray():
    """triangle_geometry.rs:33: w1 > 0, strictly.  A ray aimed at a point of the edge p0-p2 (w1 = 0 exactly: every
    coordinate a small dyadic number, so f32 and f64 agree on it) misses; the same ray moved inside by 1/64 hits."""
    import raytracinginaweekend_amd as R

    wb = R.WorldBuilder()
    tri = np.array([[0, 0, 0, 2, 0, 0, 0, 2, 0] + [0, 0, 1] * 3 + [0, 0, 1, 0, 0, 1]], f32)
    g = wb.new_group().add(wb.new_mesh(tri, wb.material_lambert_solid((0.5, 0.5, 0.5))))
    g.add(wb.new_obj_sphere(0.5, wb.material_lambert_solid((0.5, 0.5, 0.5))).translate((8.0, 8.0, -8.0)))
    cam = R.Camera.build().vertical_fov(40.0, 1.0).position((0, 0, 4)).look_at((0, 1, 0), (0, 0, 0)).build()
    world = g.build().finish(wb, R.BackgroundColor.solid((0, 0, 0)), cam)
    # every ray meets the plane z = 0 at t = 4, at origin + 4 d exactly (dyadic numbers, no zero component: a zero
    # would let hit_cond's 0 / 0 refuse the root's box before the triangle is asked)
    target = np.array([[0.0, 1.0, 0.0], [1.0 / 64, 1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], f32)
    d = np.tile(np.array([-0.25, 0.125, -1.0], f32), (4, 1))
    o = target - f32(4) * d
    t = np.zeros(4, f32)
    res = F.cast(world, o, d, t)
    got = Ck.oracle_hits(world, o, d, t)
    # on the edge w1 = 0, just inside it, on the vertex p0 (w1 = w2 = 0), on the edge w2 = 0
    assert list(res["hit"]) == [False, True, False, False]
    assert list(got["hit"]) == [False, True, False, False]


class Paced:
    """A world's tables with another shutter_pace in its camera: the builder has no setter for it (camera.rs:50
    builds it zero), but the field is public (camera.rs:163) and Camera::ray reads it (camera.rs:190)."""

    def __init__(self, world, pace):
        import ctypes as C

        from raytracinginaweekend_amd import _native as N

        self.world = world  # (the tables are the world's own)
        self.raw = N.World()
        C.memmove(C.byref(self.raw), C.byref(world.raw), C.sizeof(N.World))
        self.raw.camera.shutter_pace[0], self.raw.camera.shutter_pace[1] = pace


@pytest.mark.parametrize("name", ["A", "A_lens", "B_inside", "A+pace", "A_lens+pace"])
def test_camera_ray_alone(worlds, name):
    """Camera::ray (camera.rs:175-200) from the rtw_camera fields, in f64.  "+pace": a rolling shutter, shutter_pace =
    (0.375, -0.25), so that the time's `+ shutter_pace . (px, py)` is checked with a pace that is not zero."""
    world = FW.world(name.split("+")[0], worlds)
    if name.endswith("+pace"):
        world = Paced(world, (0.375, -0.25))
    name = name.split("+")[0]
    cam = world.raw.camera
    v = lambda a: np.array(list(a), np.float64)
    pos, ulc, ur, uu, sr, su = (v(a) for a in (cam.position, cam.upper_left_corner, cam.unit_right, cam.unit_up,
                                                 cam.scaled_right, cam.scaled_up))
    lens, pace = float(cam.lens_radius), v(cam.shutter_pace)
    assert pace.any() == isinstance(world, Paced)
    assert abs(ur @ ur - 1) < 8 * F.U and abs(uu @ uu - 1) < 8 * F.U and abs(ur @ uu) < 8 * F.U
    assert (lens > 0) == (name == "A_lens")
    seen = []
    for seed in SEEDS[:2]:
        o, d, t, p = (np.asarray(a, np.float64) for a in Ck.camera_rays(name, world, FW.SIZE, seed))
        scale = np.abs(pos).max() + lens + 1.0
        off = o - pos
        if lens > 0:
            d0, d1 = off @ ur / lens, off @ uu / lens
            # the origin lies in the lens plane, inside the unit disc
            assert np.abs(off - lens * (d0[:, None] * ur + d1[:, None] * uu)).max() <= 8 * F.U * scale
            assert (d0 * d0 + d1 * d1).max() < 1.0 + 8 * F.U * scale / lens
            assert (d0 * d0 + d1 * d1).max() > 0.9 and np.abs(d0.mean()) < 0.05 and np.abs(d1.mean()) < 0.05
            seen.append(np.stack([d0, d1]))
        else:
            assert (off == 0).all()
        # the direction is unit and collinear with ulc + px scaled_right - py scaled_up - offset, pointing the same way
        want = ulc + p[:, :1] * sr - p[:, 1:] * su - off
        wl = np.linalg.norm(want, axis=1)
        assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 4 * F.U
        bound = 8 * F.U * (np.abs(ulc).max() + np.abs(sr).max() + np.abs(su).max() + lens) / wl
        assert (np.linalg.norm(np.cross(d, want / wl[:, None]), axis=1) <= bound).all()
        assert ((d * want).sum(axis=1) > 0).all()
        # the time is in [time0, time1) plus shutter_pace . (px, py)
        start = t - p @ pace
        tol = 4 * F.U * (abs(cam.time1) + np.abs(pace).sum())
        if cam.time0 == cam.time1:
            assert np.abs(start - cam.time0).max() <= tol
        else:
            assert start.min() >= cam.time0 - tol and start.max() < cam.time1 + tol
            assert start.max() - start.min() > 0.9 * (cam.time1 - cam.time0)
        if pace.any():  # the shutter rolls: the time follows the pixel, over most of pace . (1, 1)'s range
            assert np.ptp(p @ pace) > 0.9 * np.abs(pace).sum() and np.ptp(t) > 0.9 * np.abs(pace).sum()
    if len(seen) == 2:  # another seed, another lens sample
        assert not np.array_equal(seen[0], seen[1])


def test_the_ancestor_box_rule_matters(worlds):
    """Without the reference's culling (a leaf counts only if every ancestor box passes hit_cond; an animated leaf
    keeps the box of its rest position) the caster disagrees with the oracle in the animated worlds: the rule is
    pinned by them, not decoration."""
    for name in ("A", "B"):
        world = FW.world(name, worlds)
        rays = Ck.camera_rays(name, world, FW.SIZE, 1)
        got = Ck.oracle_hits(world, *rays[:3])
        res = F.cast(world, *rays[:3], cull=False)
        differ = res["compared"] & ((res["hit"] != got["hit"]) | (np.abs(res["t"] - got["t"]) > 1e-3 * res["t"]))
        print(name, "rays that differ without the rule:", int(differ.sum()))
        assert differ.sum() >= 20
        with pytest.raises(AssertionError):
            Ck.compare(res, rays, got, name)


def test_a_volume_is_refused(worlds):
    with pytest.raises(ValueError, match="volume"):
        F.Tables(worlds("cornell_box_smoke"))
