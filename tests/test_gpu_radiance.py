"""Radiance queries on the device (R.RayCaster.radiance: rtw_radiance_*) against the oracle and plain
f64 mathematics.

Sample k of ray i is compared with rtw_oracle_ray_color of that ray from the stream (seed, first_ray + i,
first_sample + k) -- bit for bit, NaN equal to NaN, sample by sample (tests/radiance_ref.oracle_samples): the first
time shade() is checked on paths that do not start at the camera.  The ray sets are small (about 200 rays x 8
samples): the oracle side is a Python loop."""
import ctypes as C

import numpy as np
import pytest

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd import cast as RC
from tests import analytic_scenes as AS
from tests import first_hit_check as Ck
from tests import first_hit_worlds as FW
from tests import radiance_ref as RR
from tests.parity import assert_bit_identical, bit_equal
from tests.test_first_hit_host import bounce_rays
from tests.test_gpu_world_edges import ONE_LEAF, one_leaf
from tests.world_copy import chain_world

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = f32(np.inf)
SEED = 1
SAMPLES = 8
DEPTH = 50
DEMO = ("cornell_box", "cornell_box_smoke", "final_scene2", "earth_motion", "suzanne", "perlin_spheres")
ANALYTIC = ("S1", "S2", "S2m", "S3", "S4", "S5")

_casters = {}
_sets = {}


def caster(world):
    """One upload per world object for the whole module (the queries leave the world as it was)."""
    if id(world) not in _casters:
        _casters[id(world)] = (R.RayCaster(world), world)
    return _casters[id(world)][0]


def split(rays):
    return rays[:, 0:3], rays[:, 4:7], rays[:, 3]


def thin(rays, want=200):
    return np.ascontiguousarray(rays[:: max(1, len(rays) // want)])


def ray_set(kind, name, worlds):
    """(world, rays (about 200, 8), max_depth): "camera" / "bounce" of a first-hit world, "demo" camera rays of a demo
    world (20 x 10), "analytic" camera rays of an analytic scene (16 x 12)."""
    key = (kind, name)
    if key not in _sets:
        if kind == "camera":
            world = FW.world(name, worlds)
            o, d, t, _ = Ck.camera_rays(name, world, FW.SIZE, SEED)
            _sets[key] = (world, thin(RC.pack_rays(o, d, t)), DEPTH)
        elif kind == "bounce":
            world = FW.world(name, worlds)
            o, d, t, _ = bounce_rays(name, world, SEED)
            _sets[key] = (world, thin(RC.pack_rays(o, d, t)), DEPTH)
        elif kind == "demo":
            world = worlds(name)
            o, d, t, _ = Ck.camera_rays(name, world, R.Size2i(20, 10), 7)
            _sets[key] = (world, RC.pack_rays(o, d, t), DEPTH)
        else:
            world, _, _ = AS.SCENES[name]()
            o, d, t, _ = Ck.camera_rays(name, world, R.Size2i(16, 12), SEED)
            _sets[key] = (world, RC.pack_rays(o, d, t), AS.MAX_DEPTH)
    return _sets[key]


def against_the_oracle(world, rays, what, samples=SAMPLES, max_depth=DEPTH, mode=R.RenderMode.Default, seed=SEED, key=None, **kw):
    """The device's samples of `rays` against the oracle's, bit for bit; returns the device's result."""
    res = caster(world).radiance(*split(rays), samples=samples, max_depth=max_depth, mode=mode, seed=seed, per_sample=True, **kw)
    want = RR.oracle_samples(world, rays, samples, max_depth, int(mode), seed, kw.get("first_sample", 0), kw.get("first_ray", 0),
                             key=key)
    assert res.samples.dtype == f32 and res.samples.shape == (len(rays), samples, 3)
    assert_bit_identical(res.samples, want, f"{what}: samples against the oracle")
    with np.errstate(all="ignore"):
        assert_bit_identical(res.mean, RR.mean_ref(want), f"{what}: mean against the oracle's samples in order")
    return res


# ---- 1. bit for bit against the oracle, sample by sample ---------------------------------------------------------------
SETS = ([("camera", n) for n in ("A", "B", "C")] + [("bounce", n) for n in ("A", "B", "C", "D")]
        + [("demo", n) for n in DEMO] + [("analytic", n) for n in ANALYTIC])


@pytest.mark.parametrize("kind, name", SETS, ids=[f"{k} {n}" for k, n in SETS])
def test_samples_are_the_oracles(worlds, kind, name):
    world, rays, depth = ray_set(kind, name, worlds)
    assert len(rays) >= 150
    for mode in (R.RenderMode.Default, R.RenderMode.Normals):
        res = against_the_oracle(world, rays, f"{kind} {name} {mode.name}", max_depth=depth, mode=mode, key=(kind, name, int(mode)))
        s = res.samples
        if mode == R.RenderMode.Default and kind != "analytic":  # the samples of a ray are samples: they differ
            assert (~bit_equal(s[:, 0], s[:, 1]).all(axis=1)).any(), f"{kind} {name}: every ray's samples 0 and 1 are equal"


# ---- 2. depths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [0, 1, 2, 3])
def test_shallow_depths(worlds, max_depth):
    world, rays, _ = ray_set("bounce", "D", worlds)  # final_scene1
    res = against_the_oracle(world, rays, f"depth {max_depth}", samples=4, max_depth=max_depth, seed=5)
    if max_depth <= 1:  # a hit ends the path at 0: what is left is the background of the misses
        hit = caster(world).occluded(rays[:, 0:3], rays[:, 4:7], rays[:, 3])
        assert hit.any() and not res.samples[hit].any()


# ---- 3. layout edges ---------------------------------------------------------------------------------------------------
def launch_with_sentinels(c, rays, n, samples, seed=SEED):
    """rtw_radiance_samples_device on a buffer with 64 sentinel floats before and after: the (n, samples, 3) samples."""
    import torch

    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays[:max(n, 1)])).to(dev)
    buf = torch.full((64 + n * samples * 3 + 64,), -7.0, dtype=torch.float32, device=dev)
    p = N.RadianceParams(0, 0, DEPTH, samples, 0, 0, seed)
    N.check(N.lib().rtw_radiance_samples_device(c.dworld._h, C.byref(p), C.c_void_p(d_rays.data_ptr()), n,
                                                C.c_void_p(buf.data_ptr() + 256), C.c_void_p(0)))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:64] == -7.0).all() and (out[64 + n * samples * 3:] == -7.0).all(), f"n {n} x {samples}: sentinels"
    return out[64:64 + n * samples * 3].reshape(n, samples, 3)


def test_layout_edges(worlds):
    """Item counts around a wave, around a wave's range of RTW_RAD_ITEMS items and past a block's four ranges; a ray
    boundary inside a wave and a ray across waves.  Paths of a Cornell box differ in length: lanes refill."""
    world = worlds("cornell_box")
    items = N.lib().rtw_debug_radiance_items()
    big = 4 * items + 3
    side = int(np.ceil(np.sqrt(big / 0.5625)))
    o, d, t, _ = Ck.camera_rays("cornell_box", world, R.Size2i(side, int(np.ceil(big / side))), 3)
    rays = RC.pack_rays(o, d, t)
    assert len(rays) >= big
    c = caster(world)
    want = RR.oracle_samples(world, rays[:big], 1, DEPTH, 0, SEED, key=("edges", items))
    for n in (0, 1, 63, 64, 65, items - 1, items, items + 1, big):
        got = launch_with_sentinels(c, rays, n, 1)
        assert_bit_identical(got, want[:n], f"{n} items of one sample")
    assert_bit_identical(launch_with_sentinels(c, rays, 257, 1), want[:257], "samples = 1, n = 257")
    got = launch_with_sentinels(c, rays, 100, 3)
    assert_bit_identical(got, RR.oracle_samples(world, rays[:100], 3, DEPTH, 0, SEED), "samples = 3: a ray boundary inside a wave")
    got = launch_with_sentinels(c, rays, 3, 200)
    assert_bit_identical(got, RR.oracle_samples(world, rays[:3], 200, DEPTH, 0, SEED), "samples = 200: a ray across waves")
    empty = c.radiance(np.zeros((0, 3), f32), np.zeros((0, 3), f32), samples=4, finite=True, per_sample=True)
    assert len(empty) == 0 and empty.mean.shape == (0, 3) and empty.kept.shape == (0,) and empty.samples.shape == (0, 4, 3)


# ---- 4. splits ---------------------------------------------------------------------------------------------------------
def test_a_batch_is_its_parts(worlds):
    import torch

    world, rays, _ = ray_set("demo", "cornell_box_smoke", worlds)
    c = caster(world)
    n, half = len(rays), len(rays) // 2 + 1
    kw = dict(samples=SAMPLES, seed=9, per_sample=True)
    whole = c.radiance(*split(rays), first_ray=40, first_sample=5, **kw)
    # by rays, with first_ray
    a = c.radiance(*split(rays[:half]), first_ray=40, first_sample=5, **kw)
    b = c.radiance(*split(rays[half:]), first_ray=40 + half, first_sample=5, **kw)
    assert_bit_identical(np.concatenate([a.samples, b.samples]), whole.samples, "halves by rays")
    # by samples, with first_sample
    kw["samples"] = 3
    a = c.radiance(*split(rays), first_ray=40, first_sample=5, **kw)
    kw["samples"] = SAMPLES - 3
    b = c.radiance(*split(rays), first_ray=40, first_sample=8, **kw)
    assert_bit_identical(np.concatenate([a.samples, b.samples], axis=1), whole.samples, "parts by samples")
    # a shuffled handful, each ray a call of its own with its first_ray
    kw["samples"] = SAMPLES
    for i in np.random.default_rng(4).permutation(n)[:6]:
        one = c.radiance(*split(rays[i:i + 1]), first_ray=40 + int(i), first_sample=5, **kw)
        assert_bit_identical(one.samples[0], whole.samples[i], f"ray {i} alone")
    assert not bit_equal(c.radiance(*split(rays), first_ray=41, first_sample=5, **kw).samples, whole.samples).all()
    # chunks of a few rays' worth of scratch: the same mean and kept, numpy and tensors
    full = c.radiance(*split(rays), samples=SAMPLES, seed=9, finite=True)
    few = c.radiance(*split(rays), samples=SAMPLES, seed=9, finite=True, max_bytes=7 * SAMPLES * 12 + 5)
    assert_bit_identical(few.mean, full.mean, "chunks of 7 rays: mean")
    assert few.kept.dtype == np.uint32 and np.array_equal(few.kept, full.kept)
    tiny = c.radiance(*split(rays), samples=SAMPLES, seed=9, max_bytes=1)  # (at least one ray a chunk)
    plain = c.radiance(*split(rays), samples=SAMPLES, seed=9)
    assert plain.kept is None and plain.samples is None
    assert_bit_identical(tiny.mean, plain.mean, "chunks of one ray: mean")
    dev = torch.device("cuda", 0)
    o, d, tm = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in split(rays))
    on_device = c.radiance(o, d, tm, samples=SAMPLES, seed=9, finite=True, max_bytes=7 * SAMPLES * 12)
    assert_bit_identical(on_device.mean.cpu().numpy(), full.mean, "tensors, chunks of 7 rays: mean")
    assert np.array_equal(on_device.kept.cpu().numpy().view(np.uint32), full.kept)


def test_the_host_call_chunks_by_rays(worlds, monkeypatch):
    """rtw_radiance (host arrays, any alignment) against the device path: whole, and in chunks of 5 rays."""
    world, rays, _ = ray_set("demo", "cornell_box", worlds)
    c = caster(world)
    n = len(rays)
    want = c.radiance(*split(rays), samples=SAMPLES, seed=3, first_ray=11, finite=True)
    raw = np.zeros(n * 8 + 1, f32)
    off = raw[1:]  # (4 bytes off any 16-byte boundary the allocation has)
    off[:] = rays.reshape(-1)
    for cap in (None, str(5 * SAMPLES * 12)):
        if cap:
            monkeypatch.setenv("RTW_RADIANCE_BUFFER_BYTES", cap)
        mean, kept = np.full((n, 3), -7.0, f32), np.full(n, 77, np.uint32)
        p = N.RadianceParams(N.RADIANCE_FINITE, 0, DEPTH, SAMPLES, 0, 11, 3)
        N.check(N.lib().rtw_radiance(c.dworld._h, C.byref(p), C.c_void_p(off.ctypes.data), n, C.c_void_p(mean.ctypes.data),
                                     C.c_void_p(kept.ctypes.data)))
        assert_bit_identical(mean, want.mean, f"rtw_radiance, cap {cap}: mean")
        assert np.array_equal(kept, want.kept)
    p = N.RadianceParams(0, 0, DEPTH, SAMPLES, 0, 11, 3)
    mean = np.zeros((n, 3), f32)
    N.check(N.lib().rtw_radiance(c.dworld._h, C.byref(p), C.c_void_p(off.ctypes.data), n, C.c_void_p(mean.ctypes.data), None))
    assert_bit_identical(mean, c.radiance(*split(rays), samples=SAMPLES, seed=3, first_ray=11).mean, "rtw_radiance, plain mean")


# ---- 5. reductions -----------------------------------------------------------------------------------------------------
def test_reductions_over_the_devices_own_samples(worlds):
    for kind, name in (("demo", "suzanne"), ("demo", "final_scene2"), ("bounce", "B")):
        world, rays, _ = ray_set(kind, name, worlds)
        c = caster(world)
        res = c.radiance(*split(rays), samples=SAMPLES, seed=SEED, per_sample=True)
        fin = c.radiance(*split(rays), samples=SAMPLES, seed=SEED, per_sample=True, finite=True)
        assert_bit_identical(fin.samples, res.samples, f"{name}: the flag changes no sample")
        with np.errstate(all="ignore"):
            assert_bit_identical(res.mean, RR.mean_ref(res.samples), f"{name}: mean")
            mean, kept = RR.finite_ref(res.samples)
        assert res.kept is None and fin.kept.dtype == np.uint32
        assert_bit_identical(fin.mean, mean, f"{name}: finite mean")
        assert np.array_equal(fin.kept, kept), f"{name}: kept"


def test_finite_means_on_a_mesh(worlds):
    """suzanne: the reference's 0 / 0 pdf makes NaN samples; the plain mean is NaN exactly on their rays, the finite
    mean is finite everywhere and kept is the oracle's count."""
    world = worlds("suzanne")
    rays = RR.pixel_centre_rays(world, 24, 14)
    want = RR.oracle_samples(world, rays, 32, DEPTH, 0, 7, key="suzanne 24 x 14 x 32")
    bad = ~np.isfinite(want).all(axis=2)  # (n, 32)
    assert bad.any(axis=1).any() and (~bad.any(axis=1)).any()
    print(f"suzanne: {int(bad.sum())} non-finite samples of {bad.size} on {int(bad.any(axis=1).sum())} of {len(rays)} rays")
    c = caster(world)
    plain = c.radiance(*split(rays), samples=32, seed=7, per_sample=True)
    assert_bit_identical(plain.samples, want, "suzanne: samples against the oracle")
    assert np.array_equal(np.isnan(plain.mean).any(axis=1), bad.any(axis=1))
    fin = c.radiance(*split(rays), samples=32, seed=7, finite=True)
    assert np.isfinite(fin.mean).all()
    assert np.array_equal(fin.kept, (32 - bad.sum(axis=1)).astype(np.uint32))
    mean, kept = RR.finite_ref(want)
    assert_bit_identical(fin.mean, mean, "suzanne: finite mean against the oracle's samples")


# ---- 6. the analytic probe, independent of the oracle ------------------------------------------------------------------
def test_probe_of_the_cosine_lobe():
    world, _, _ = AS.s2_cosine_lobe()
    rays, F, scale = RR.floor_probe(world)
    res = R.radiance_rays(world, *split(rays), samples=RR.PROBE_SAMPLES, max_depth=AS.MAX_DEPTH, seed=AS.SEED, per_sample=True)
    RR.check_probe_s2(res.samples, F, scale, "device S2 probe")
    # a Bernoulli sample of a dyadic value: the f32 sum is exact, so the mean is the lit fraction times the value
    lit = (res.samples[..., 0] == f32(scale[0])).mean(axis=1)
    assert np.array_equal(res.mean.astype(np.float64), lit[:, None] * scale[None, :])


def test_probe_of_the_light_mixture():
    world, _, _ = AS.s2m_light_mixture()
    rays, F, scale = RR.floor_probe(world)
    res = R.radiance_rays(world, *split(rays), samples=RR.PROBE_SAMPLES, max_depth=AS.MAX_DEPTH, seed=AS.SEED, per_sample=True)
    RR.check_probe_s2m(res.samples, F, scale, "device S2m probe")


# ---- 7. directions and odd rays ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.25, 1.0000001, 1.000001, 3.0])  # (1 + 2^-23: unit to the cull; 1 + 2^-20: not)
def test_directions_need_not_be_unit(worlds, scale):
    """The direction is used as given: reflect, the dielectric's cos_theta (world A has one), the sky's argument --
    and the reference's sphere test, whose roots for such a ray lie nowhere near the sphere (final_scene1 and
    final_scene2 hold plain spheres: the proximity cull's bound does not cover them, the first segment walks without)."""
    for kind, name in (("bounce", "A"), ("bounce", "C"), ("bounce", "D"), ("demo", "final_scene2")):
        world, rays, _ = ray_set(kind, name, worlds)
        scaled = rays.copy()
        scaled[:, 4:7] *= f32(scale)
        res = against_the_oracle(world, scaled, f"{name}, directions x {scale}", samples=4)
        if name == "D" and scale in (0.25, 3.0):  # (its sky reads the direction's y as given: the length matters)
            assert not bit_equal(res.samples, RR.oracle_samples(world, rays, 4, DEPTH, 0, SEED)).all()


def norm_excess(rays):
    """| |d|^2 - 1 | of every ray as the kernel takes it: f32, (x x + y y) + z z, no contraction."""
    d = np.ascontiguousarray(rays[:, 4:7], f32)
    return np.abs(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - f32(1))


@pytest.mark.parametrize("exponent", [-22.25, -21.5], ids=["just inside", "just outside"])
def test_directions_at_the_culls_threshold(worlds, exponent):
    """The first segment is culled while | |d|^2 - 1 | <= 2^-21.  Directions stretched by 1 + 2^exponent (in f64, then
    rounded) put |d|^2 - 1 at about 2^(exponent + 1): for -22.25 inside (2^-22, 2^-21], the culled band's far end,
    where the sphere bound gives up the most; for -21.5 just past it (|d|^2 is a multiple of 2^-23 there and the
    rays' own rounding spreads it over three or four of them: most rays, not all, land where they are aimed).  final_scene1 and final_scene2 hold the plain
    spheres the bound is about: every bounce-like ray of the one, a 60 x 34 frame's camera rays of the other."""
    o, d, t, _ = bounce_rays("D", FW.world("D", worlds), SEED)
    sets = [("final_scene1", FW.world("D", worlds), RC.pack_rays(o, d, t))]
    o, d, t, _ = Ck.camera_rays("final_scene2", worlds("final_scene2"), R.Size2i(60, 34), 7)
    sets.append(("final_scene2", worlds("final_scene2"), RC.pack_rays(o, d, t)))
    for name, world, rays in sets:
        assert len(rays) >= 2000
        scaled = rays.copy()
        scaled[:, 4:7] = (rays[:, 4:7].astype(np.float64) * (1.0 + 2.0 ** exponent)).astype(f32)
        e = norm_excess(scaled)
        inside = (e > f32(2.0 ** -22)) & (e <= f32(2.0 ** -21))
        print(f"{name}, exponent {exponent}: {len(rays)} rays, {100 * inside.mean():.1f} % in (2^-22, 2^-21], "
              f"{100 * (e > f32(2.0 ** -21)).mean():.1f} % above")
        if exponent == -22.25:
            assert inside.mean() >= 0.7
        else:
            assert (e > f32(2.0 ** -21)).mean() >= 0.8
        against_the_oracle(world, scaled, f"{name}, directions x (1 + 2^{exponent})", samples=2)


def test_directions_with_zero_components(worlds):
    from tests.test_gpu_cast import axis_rays

    world = FW.world("B", worlds)
    rays = axis_rays(world)
    rays = np.ascontiguousarray(rays[np.sort(np.random.default_rng(6).permutation(len(rays))[:600])])
    assert (np.signbit(rays[:, 4:7]) & (rays[:, 4:7] == 0)).any()
    against_the_oracle(world, rays, "world B, axis-aligned rays", samples=2)


def test_rays_that_are_not_finite_return(worlds):
    """Every walk is bounded by the tree and every path by max_depth: a NaN or an infinite component comes back."""
    world, rays, _ = ray_set("bounce", "B", worlds)
    odd = rays[:12].copy()
    nan = f32(np.nan)
    odd[0, 0], odd[1, 5], odd[2, 4:7], odd[3, 0:3] = nan, nan, nan, nan
    odd[4, 1], odd[5, 6], odd[6, 2], odd[7, 4] = INF, INF, -INF, -INF
    odd[8, 3], odd[9, 7], odd[10, 7], odd[11, 4:7] = nan, nan, -INF, 0.0
    res = caster(world).radiance(*split(odd), samples=4, per_sample=True)
    want = RR.oracle_samples(world, odd, 4, DEPTH, 0, R.rendering.DEFAULT_SEED)
    assert_bit_identical(res.samples, want, "rays with NaN and infinite components")
    assert_bit_identical(res.samples[9:11], caster(world).radiance(*split(rays[9:11]), samples=4, per_sample=True, first_ray=9).samples,
                         "t_end is not read")


# ---- 8. tree edges -----------------------------------------------------------------------------------------------------
def small_frame(world, what):
    o, d, t, _ = Ck.camera_rays(what, world, R.Size2i(24, 14), SEED)
    rays = RC.pack_rays(o, d, t)
    res = R.radiance_rays(world, *split(rays), samples=4, seed=SEED, per_sample=True)
    want = RR.oracle_samples(world, rays, 4, DEPTH, 0, SEED)
    assert_bit_identical(res.samples, want, what)
    return res


@pytest.mark.parametrize("kind", list(ONE_LEAF))
def test_one_leaf_worlds(kind):
    """root = -1: the walk stands on a leaf at once and the stack is never used."""
    world = one_leaf(kind)
    assert (world.raw.root, world.raw.node_count, world.raw.leaf_count) == (-1, 0, 1)
    small_frame(world, f"one {kind}")


@pytest.mark.parametrize("extra_rect", [False, True], ids=["spheres", "with a rect"])
def test_deepest_tree(extra_rect):
    """A left-deep chain of 32 levels, the camera rays aimed along it: one stack entry per level, every segment."""
    small_frame(chain_world(32, extra_rect=extra_rect), "the chain" + (" with a rect" if extra_rect else ""))


# ---- 9. interleaving ---------------------------------------------------------------------------------------------------
def test_radiance_calls_leave_accumulators_alone(worlds):
    world, rays, _ = ray_set("bounce", "D", worlds)
    size = R.Size2i(48, 27)

    def run(interrupt):
        dw = R.DeviceWorld(world, 0)
        acc = R.Accumulator(dw, size, 8, seed=5, moments=True)
        aov = R.AovAccumulator(dw, size, seed=5)
        c = R.RayCaster(dw)
        acc.add(2)
        aov.add(2)
        if interrupt:
            c.radiance(*split(rays), samples=4, finite=True)
            c.cast(rays[:, 0:3], rays[:, 4:7], rays[:, 3])
        acc.add(3)
        aov.add(1)
        out = [acc.image(), acc.stderr(), aov.albedo(), aov.normal(), aov.depth(), aov.hits().view(f32)]
        acc.release()
        aov.release()
        dw.release()
        return out

    for a, b in zip(run(True), run(False)):
        assert_bit_identical(a, b, "an accumulator interrupted by radiance queries")


# ---- 10. torch tensors -------------------------------------------------------------------------------------------------
def test_device_tensors_in_device_tensors_out(worlds):
    import torch

    world, rays, _ = ray_set("bounce", "B", worlds)
    c = caster(world)
    dev = torch.device("cuda", 0)
    o, d, tm = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in split(rays))
    want = c.radiance(*split(rays), samples=4, finite=True, per_sample=True)
    for got in (c.radiance(o, d, tm, samples=4, finite=True, per_sample=True),
                c.radiance_device(o, d, tm, samples=4, finite=True, per_sample=True)):
        for k in ("mean", "kept", "samples"):
            x = getattr(got, k)
            assert isinstance(x, torch.Tensor) and x.device == dev, k
        assert got.mean.dtype == torch.float32 and got.kept.dtype == torch.int32 and got.samples.shape == (len(rays), 4, 3)
        assert_bit_identical(got.mean.cpu().numpy(), want.mean, "tensors: mean")
        assert_bit_identical(got.samples.cpu().numpy(), want.samples, "tensors: samples")
        assert np.array_equal(got.kept.cpu().numpy().view(np.uint32), want.kept)
    one = c.radiance(o, (0.0, -1.0, 0.0), 0.75, samples=2)
    assert one.kept is None and one.samples is None
    assert_bit_identical(one.mean.cpu().numpy(), c.radiance(rays[:, 0:3], (0.0, -1.0, 0.0), 0.75, samples=2).mean, "broadcast")
    with pytest.raises(ValueError, match="^directions:"):
        c.radiance(o, d.double())
    with pytest.raises(ValueError, match="^origins:"):
        c.radiance(o.cpu(), d)
    with pytest.raises(ValueError, match="^origins:"):
        c.radiance(rays[:, 0:3], rays[:, 4:7], tm)
    with pytest.raises(ValueError, match="^samples:"):
        c.radiance(o, d, tm, samples=0)


# ---- 11. refusals that need the device ---------------------------------------------------------------------------------
def test_device_refusals(worlds):
    import torch

    world, rays, _ = ray_set("camera", "A", worlds)
    c = R.RayCaster(world)
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays[:65].copy()).to(dev)
    d_colors = torch.full((64, 2, 3), -7.0, dtype=torch.float32, device=dev)
    L = N.lib()
    p = N.RadianceParams(0, 0, DEPTH, 2, 0, 0, 1)
    assert L.rtw_radiance_samples_device(c.dworld._h, C.byref(p), C.c_void_p(d_rays.data_ptr() + 4), 64,
                                         C.c_void_p(d_colors.data_ptr()), None) == N.RTW_ERR_INVALID_ARGUMENT
    assert "rays must be 16-byte" in L.rtw_last_error().decode()
    handle = C.c_void_p(c.dworld._h.value)  # (what a C caller keeps past the release)
    c.release()
    assert L.rtw_radiance_samples_device(handle, C.byref(p), C.c_void_p(d_rays.data_ptr()), 64, C.c_void_p(d_colors.data_ptr()),
                                         None) == N.RTW_ERR_INVALID_ARGUMENT
    assert "released" in L.rtw_last_error().decode()
    mean = np.full((64, 3), -7.0, f32)
    assert L.rtw_radiance(handle, C.byref(p), C.c_void_p(rays.ctypes.data), 64, C.c_void_p(mean.ctypes.data), None) \
        == N.RTW_ERR_INVALID_ARGUMENT
    assert "released" in L.rtw_last_error().decode()
    torch.cuda.synchronize()
    assert (d_colors.cpu().numpy() == -7.0).all() and (mean == -7.0).all()  # nothing was launched or written
    with pytest.raises(N.RtwError, match="world"):  # the Python object holds no handle any more
        c.radiance(*split(rays[:4]), samples=2)


def test_radiance_rays_is_one_batch(worlds):
    world, rays, _ = ray_set("camera", "A", worlds)
    a = R.radiance_rays(world, *split(rays), samples=4, seed=3, finite=True)
    b = caster(world).radiance(*split(rays), samples=4, seed=3, finite=True)
    assert_bit_identical(a.mean, b.mean, "radiance_rays")
    assert np.array_equal(a.kept, b.kept)
