"""GPU parity: the HIP megakernel vs the CPU oracle, bit for bit, in "ctr" RNG mode.

Every demo world (so every geometry kind, wrapper, material, texture and the light sampler)
at a size the oracle finishes in seconds.  The tolerance is zero: f32 images must be
bit-identical (NaN == NaN).
"""
import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from tests.parity import assert_bit_identical
from tests.variant_worlds import soup_world as _soup_world, sphere_cloud as _sphere_cloud

pytestmark = pytest.mark.gpu

CASES = [
    ("final_scene1", 64, 36, 6),
    ("final_scene2", 40, 40, 6),
    ("cornell_box", 40, 40, 8),
    ("cornell_box_smoke", 40, 40, 8),
    ("cornell_cube", 40, 40, 8),
    ("suzanne", 48, 36, 4),
    ("earth_mapped", 48, 40, 4),
    ("earth_motion", 64, 36, 4),
    ("moving_spheres", 48, 40, 4),
    ("perlin_spheres", 48, 36, 4),
    ("simple_plane", 64, 36, 8),
    ("defocus_blur", 64, 36, 8),
]


@pytest.mark.parametrize("name,w,h,spp", CASES, ids=[c[0] for c in CASES])
def test_world_bit_identical(worlds, name, w, h, spp):
    world = worlds(name)
    size = R.Size2i(w, h)
    gpu = R.render(size, 1, spp, 50, world, seed=11)
    ref = O.render(world, R.render_params(size, spp, 50, seed=11))
    assert_bit_identical(gpu, ref, name)


@pytest.mark.parametrize("name", ["final_scene1", "cornell_box", "suzanne"])
def test_normals_mode(worlds, name):
    world = worlds(name)
    size = R.Size2i(40, 30)
    gpu = R.render(size, 1, 2, 50, world, R.RenderMode.Normals, seed=3)
    ref = O.render(world, R.render_params(size, 2, 50, R.RenderMode.Normals, seed=3))
    assert_bit_identical(gpu, ref, name + "/normals")


@pytest.mark.parametrize("max_depth", [0, 1, 2, 5])
def test_shallow_depths(worlds, max_depth):
    world = worlds("final_scene1")
    size = R.Size2i(32, 18)
    gpu = R.render(size, 1, 4, max_depth, world, seed=5)
    ref = O.render(world, R.render_params(size, 4, max_depth, seed=5))
    assert_bit_identical(gpu, ref, f"depth {max_depth}")


@pytest.mark.parametrize("chunk,buffer_bytes", [("1", None), ("3", "200000"), ("8", "50000"), ("64", None)])
def test_work_item_split_is_bit_exact(worlds, chunk, buffer_bytes, monkeypatch):
    """Work items of `chunk` samples and frames split over several launches (small colour buffer:
    the running sum is carried between launches) give the oracle's bits."""
    world = worlds("final_scene1")
    monkeypatch.setenv("RTW_CHUNK", chunk)
    if buffer_bytes:
        monkeypatch.setenv("RTW_SAMPLE_BUFFER_BYTES", buffer_bytes)
    p = R.render_params(R.Size2i(40, 24), 37, 50, seed=13)
    gpu = R.render(R.Size2i(40, 24), 1, 37, 50, world, seed=13)
    assert_bit_identical(gpu, O.render(world, p, O.RNG_CTR), f"chunk {chunk}")


@pytest.mark.parametrize("name", ["final_scene1", "suzanne", "cornell_box", "cornell_cube", "final_scene2",
                                  "earth_mapped", "cornell_box_smoke"])
def test_golden_frames(name):
    """The committed golden frames (tests/golden/images.npz), bit for bit, through rtw_render."""
    import os

    from tests.golden.make_golden import IMAGES

    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "images.npz"))
    _, w, h, spp, depth, seed = next(c for c in IMAGES if c[0] == name)
    gpu = R.render(R.Size2i(w, h), 1, spp, depth, R.demo_world(name), seed=seed)
    assert_bit_identical(gpu, fx[name], name)


@pytest.mark.parametrize("name,world_size", [("final_scene1", 2), ("final_scene1", 3), ("final_scene1", 4),
                                             ("final_scene1", 8), ("suzanne", 8)])
def test_tile_partitions_reassemble_bit_exact(worlds, name, world_size):
    """P3 on one GPU: each partition rendered in RTW_LAYOUT_TILES, placed as the all-gather would,
    scattered by the untile kernel == the single-partition frame (and the host mirror agrees)."""
    import torch

    from raytracinginaweekend_amd.distributed import FrameSpec, TileExchange, untile_host

    world = worlds(name)
    spec = FrameSpec(R.Size2i(52, 30), 3, 50, seed=4)
    full = R.render(spec.size, 1, 3, 50, world, seed=4)
    dw = R.DeviceWorld(world, 0)
    xs = [TileExchange(spec, r, world_size) for r in range(world_size)]
    gathered = torch.zeros(xs[0].stride * world_size, dtype=torch.float32, device="cuda:0")
    for r, x in enumerate(xs):
        dw.render_into(x.params, gathered[r * x.stride:].data_ptr(), 0)
    image = torch.zeros(spec.size.width * spec.size.height * 3, dtype=torch.float32, device="cuda:0")
    xs[0].untile(gathered, image, 0)
    torch.cuda.synchronize()
    assert_bit_identical(image.cpu().numpy().reshape(-1, 3), full, "untile_device")
    host = untile_host(gathered.cpu().numpy(), spec.size, spec.tile, world_size, xs[0].stride)
    assert_bit_identical(host, full, "untile_host")


@pytest.mark.parametrize("name", ["final_scene1", "suzanne", "cornell_cube", "earth_motion", "cornell_box"])
def test_leaf_kind_loops_agree(worlds, name, monkeypatch):
    """The traversal loop specialised to the world's leaf kinds (plain spheres only / plain
    spheres and triangles, or with rects) gives the generic loop's bits (RTW_LEAF_KINDS=4) on a frame
    large enough to fill the GPU, and the oracle's on a small one."""
    world = worlds(name)
    size = R.Size2i(320, 180)
    fast = R.render(size, 1, 8, 50, world, seed=21)
    small = R.render(R.Size2i(40, 24), 1, 4, 50, world, seed=21)
    monkeypatch.setenv("RTW_LEAF_KINDS", "4")
    generic = R.render(size, 1, 8, 50, world, seed=21)
    assert_bit_identical(fast, generic, name + " specialised vs generic loop")
    assert_bit_identical(small, O.render(world, R.render_params(R.Size2i(40, 24), 4, 50, seed=21)), name)


@pytest.mark.parametrize("name", ["final_scene1", "suzanne"])
def test_true_division_loop_agrees(worlds, name, monkeypatch):
    """Every ray on the true-division slab test (the general traversal loop, RTW_NO_MARKSTEIN=1)
    gives the Markstein loop's bits on a GPU-filling frame, and the oracle's on a small one."""
    world = worlds(name)
    size = R.Size2i(320, 180)
    fast = R.render(size, 1, 8, 50, world, seed=23)
    monkeypatch.setenv("RTW_NO_MARKSTEIN", "1")
    slow = R.render(size, 1, 8, 50, world, seed=23)
    small = R.render(R.Size2i(40, 24), 1, 4, 50, world, seed=23)
    assert_bit_identical(fast, slow, name + " Markstein vs true-division loop")
    assert_bit_identical(small, O.render(world, R.render_params(R.Size2i(40, 24), 4, 50, seed=23)), name)


def _kernel_tree(world) -> str:
    import torch

    dw = R.DeviceWorld(world, 0)
    out = torch.empty(16 * 16 * 3, dtype=torch.float32, device="cuda:0")
    dw.render_into(R.render_params(R.Size2i(16, 16), 1, 50), out.data_ptr(), 0)
    torch.cuda.synchronize()
    return dw.kernel_variant()["tree"]


@pytest.mark.parametrize("name", ["final_scene1", "suzanne", "cornell_cube", "cornell_box", "earth_motion",
                                  "moving_spheres", "defocus_blur", "simple_plane"])
def test_sah_tree_agrees(worlds, name, monkeypatch):
    """closest hits found on the kernel's SAH tree (verified against the reference
    tree's order, re-traced there where the proof fails) give the reference-tree loop's bits
    (RTW_NO_SAH=1) on a GPU-filling frame, and the oracle's on a small one."""
    world = worlds(name)
    assert _kernel_tree(world).startswith("sah")
    size = R.Size2i(320, 180)
    sah = R.render(size, 1, 8, 50, world, seed=29)
    small = R.render(R.Size2i(40, 24), 1, 4, 50, world, seed=29)
    monkeypatch.setenv("RTW_NO_SAH", "1")
    assert _kernel_tree(world) == "reference"
    ref = R.render(size, 1, 8, 50, world, seed=29)
    assert_bit_identical(sah, ref, name + " SAH vs reference tree")
    assert_bit_identical(small, O.render(world, R.render_params(R.Size2i(40, 24), 4, 50, seed=29)), name)


def _tie_world(mesh: bool = True):
    """Exact ties and grazing hits: four coincident spheres with different materials (every hit on
    them is a tie the reference breaks by its DFS order), a row of touching spheres (tangent
    points on shared box planes), and a quad of two triangles twice over (coincident triangles,
    a shared diagonal)."""
    wb = R.WorldBuilder()
    mats = [wb.material_lambert_solid((0.8, 0.2, 0.2)), wb.material_lambert_solid((0.2, 0.8, 0.2)),
            wb.material_metal_solid((0.7, 0.7, 0.7), 0.1), wb.material_dielectric(1.5)]
    g = wb.new_group()
    g.add(wb.new_obj_sphere(100.0, mats[0]).translate((0.0, -100.0, 0.0)))
    for i in range(4):
        g.add(wb.new_obj_sphere(0.5, mats[i]).translate((0.0, 0.5, 0.0)))
    for k in range(7):
        g.add(wb.new_obj_sphere(0.25, mats[k % 3]).translate((-1.5 + 0.5 * k, 0.25, 1.0)))
    p = [(-2.0, 0.0, -1.0), (2.0, 0.0, -1.0), (2.0, 2.0, -1.0), (-2.0, 2.0, -1.0)]
    n = (0.0, 0.0, 1.0)

    def tri(a, b, c):
        return list(p[a]) + list(p[b]) + list(p[c]) + list(n) * 3 + [0.0] * 6

    quad = np.array([tri(0, 1, 2), tri(0, 2, 3)], np.float32)
    if mesh:
        g.add(wb.new_mesh(quad, mats[1]))
        g.add(wb.new_mesh(quad, mats[2]))
    cam = R.Camera.build().vertical_fov(40.0, 9.0 / 16.0).position((0.3, 1.2, 5.0)).look_at((0, 1, 0), (0, 0.5, 0)).build()
    return g.build().finish(wb, R.BackgroundColor.sky(), cam)


def _tie_world_wrapped():
    """Ties among rects, boxes and wrapped leaves: two coincident rects of different materials, a
    rotated box twice over (its reference Aabb is the untransformed box, the apply_aabb quirk, so
    many of its hits lie outside that box: the proof falls back to the reference tree there), a box
    face flush with a rect, and two coincident moving spheres under motion blur."""
    wb = R.WorldBuilder()
    mats = [wb.material_lambert_solid((0.8, 0.2, 0.2)), wb.material_lambert_solid((0.2, 0.8, 0.2)),
            wb.material_metal_solid((0.7, 0.7, 0.7), 0.1), wb.material_dielectric(1.5)]
    g = wb.new_group()
    g.add(wb.new_obj_sphere(100.0, mats[0]).translate((0.0, -100.0, 0.0)))
    g.add(wb.new_obj_rect_xy((0.0, 1.0, -1.0), 4.0, 2.0, mats[0]))
    g.add(wb.new_obj_rect_xy((0.0, 1.0, -1.0), 4.0, 2.0, mats[1]))
    for m in (mats[1], mats[2]):
        g.add(wb.new_obj_box(0.8, 0.8, 0.8, m).rotate_around_up(25.0).translate((-1.0, 0.4, 0.3)))
    g.add(wb.new_obj_box(0.6, 0.6, 0.6, mats[3]).translate((1.2, 0.3, -0.7)))
    g.add(wb.new_obj_rect_yz((1.5, 0.3, -0.7), 0.6, 0.6, mats[1]))
    for m in (mats[0], mats[3]):
        g.add(wb.new_obj_sphere(0.3, m).translate((0.6, 1.4, 0.5)).animate_moving((0.0, 0.5, 0.0)))
    cam = (R.Camera.build().vertical_fov(40.0, 9.0 / 16.0).position((0.3, 1.2, 5.0)).look_at((0, 1, 0), (0, 0.5, 0))
           .motion_blur(0.0, 1.0).build())
    return g.build().finish(wb, R.BackgroundColor.sky(), cam)


def test_sah_wrapped_ties_and_grazing_hits(monkeypatch):
    world = _tie_world_wrapped()
    assert _kernel_tree(world).startswith("sah")
    size = R.Size2i(96, 54)
    gpu = R.render(size, 1, 8, 50, world, seed=37)
    assert_bit_identical(gpu, O.render(world, R.render_params(size, 8, 50, seed=37)), "wrapped tie world")
    big = R.Size2i(480, 270)
    sah = R.render(big, 1, 4, 50, world, seed=37)
    monkeypatch.setenv("RTW_NO_SAH", "1")
    assert_bit_identical(sah, R.render(big, 1, 4, 50, world, seed=37), "wrapped tie world, SAH vs reference tree")


def _rolling_shutter_world(pace):
    """Fast-moving spheres under motion blur with a rolling shutter: camera.rs:190 adds
    dot(shutter_pace, (px, py)) to each ray's start time, so ray times leave [time0, time1]
    (shutter_pace is a pub field of the reference's Camera, set here the way a Rust caller would)."""
    wb = R.WorldBuilder()
    mats = [wb.material_lambert_solid((0.8, 0.2, 0.2)), wb.material_metal_solid((0.7, 0.7, 0.7), 0.0),
            wb.material_dielectric(1.5), wb.material_lambert_solid((0.2, 0.3, 0.9))]
    g = wb.new_group()
    g.add(wb.new_obj_sphere(100.0, mats[0]).translate((0.0, -100.0, 0.0)))
    for k in range(9):
        v = ((k % 3 - 1) * 1.5, 0.8 + 0.4 * (k % 2), (k // 3 - 1) * 1.2)
        g.add(wb.new_obj_sphere(0.22, mats[k % 4]).translate((-1.6 + 0.4 * k, 0.6, -0.3 * (k % 3))).animate_moving(v))
    cam = (R.Camera.build().vertical_fov(40.0, 9.0 / 16.0).position((0.3, 1.2, 5.0)).look_at((0, 1, 0), (0, 0.5, 0))
           .motion_blur(0.0, 1.0).build())
    world = g.build().finish(wb, R.BackgroundColor.sky(), cam)
    world.raw.camera.shutter_pace[0], world.raw.camera.shutter_pace[1] = pace
    return world


@pytest.mark.parametrize("pace", [(0.8, -0.6), (-1.5, 2.0)])
def test_sah_rolling_shutter_motion(pace, monkeypatch):
    """the SAH tree's boxes of Animation leaves sweep every ray time, the rolling
    shutter's included (rtw_cull.h rtw_ray_time_range): bit-exact against the oracle and the
    reference-tree loop with a non-zero shutter_pace."""
    world = _rolling_shutter_world(pace)
    assert _kernel_tree(world).startswith("sah")
    size = R.Size2i(96, 54)
    gpu = R.render(size, 1, 8, 50, world, seed=43)
    assert_bit_identical(gpu, O.render(world, R.render_params(size, 8, 50, seed=43)), f"rolling shutter {pace}")
    big = R.Size2i(480, 270)
    sah = R.render(big, 1, 4, 50, world, seed=43)
    monkeypatch.setenv("RTW_NO_SAH", "1")
    assert_bit_identical(sah, R.render(big, 1, 4, 50, world, seed=43), f"rolling shutter {pace}, SAH vs reference")


def test_sah_ties_and_grazing_hits(monkeypatch):
    world = _tie_world()
    assert _kernel_tree(world).startswith("sah")
    size = R.Size2i(96, 54)
    gpu = R.render(size, 1, 8, 50, world, seed=31)
    assert_bit_identical(gpu, O.render(world, R.render_params(size, 8, 50, seed=31)), "tie world")
    big = R.Size2i(480, 270)
    sah = R.render(big, 1, 4, 50, world, seed=31)
    monkeypatch.setenv("RTW_NO_SAH", "1")
    assert_bit_identical(sah, R.render(big, 1, 4, 50, world, seed=31), "tie world, SAH vs reference tree")


def test_coop_tie_resolution_decides_images(monkeypatch):
    """the wave-cooperative trace finds every tied leaf and keeps the one the reference's
    DFS visits first (leaf_key); the walk's tied rays and the drain's rays go through it.  Bit-exact
    against the oracle and with the resolution off (re-traced on the reference tree), and an audit
    setting that keeps the DFS-last tied leaf changes the image (the resolution decides pixels)."""
    world = _tie_world()
    dw = R.DeviceWorld(world, 0)
    assert _kernel_tree(world).startswith("sah")
    import torch

    out = torch.empty(16 * 16 * 3, dtype=torch.float32, device="cuda:0")
    dw.render_into(R.render_params(R.Size2i(16, 16), 1, 50), out.data_ptr(), 0)
    torch.cuda.synchronize()
    assert dw.kernel_variant()["leaf_kinds"] <= 2  # plain spheres / rects / triangles: coop_solve applies
    size = R.Size2i(160, 90)
    gpu = R.render(size, 1, 8, 50, world, seed=41)
    assert_bit_identical(gpu, O.render(world, R.render_params(size, 8, 50, seed=41)), "tie world, coop ties")
    monkeypatch.setenv("RTW_COOP_TIES", "0")
    monkeypatch.setenv("RTW_COOP_MAX", "0")
    assert_bit_identical(gpu, R.render(size, 1, 8, 50, world, seed=41), "tie world, coop off")
    monkeypatch.delenv("RTW_COOP_TIES")
    monkeypatch.delenv("RTW_COOP_MAX")
    monkeypatch.setenv("RTW_COOP_AUDIT", "1")
    wrong = R.render(size, 1, 8, 50, world, seed=41)
    assert not np.array_equal(np.asarray(wrong), np.asarray(gpu)), "the DFS-last tied leaf gave the same image"


def _drain_counts(reset: bool = True) -> tuple:
    """(rays posted, posts traced by helper waves, posts traced by their owner) since the last reset
    (rtw_debug_drain_counts: the block-shared drain's counters in the product kernel)."""
    import ctypes as C

    from raytracinginaweekend_amd import _native as N

    fn = N.lib().rtw_debug_drain_counts
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.c_int]
    out = (C.c_uint64 * 3)()
    N.check(fn(0, out, 1 if reset else 0))
    return tuple(int(x) for x in out)


@pytest.mark.parametrize("name", ["suzanne", "soup"])
def test_shared_drain_bit_exact(worlds, name, monkeypatch):
    """a wave's drained rays posted to the block's mailbox and traced by the block's
    finished waves (or by the owner) give the image of each wave tracing its own (RTW_NO_COOP_SHARE=1);
    with one or three posts per batch (RTW_MB_CAP) the rays beyond it walk again from the root, and
    the image stays the same.  Both worlds take the shared drain (leaf kinds 1: plain spheres and
    triangles; suzanne in LDS mode 1, the soup in mode 2), and the drain's counters show that rays were
    posted and that other waves traced some of them (the test must not pass vacuously)."""
    import torch

    world = worlds(name) if name != "soup" else _soup_world(300)
    dw = R.DeviceWorld(world, 0)
    out = torch.empty(16 * 16 * 3, dtype=torch.float32, device="cuda:0")
    dw.render_into(R.render_params(R.Size2i(16, 16), 1, 50), out.data_ptr(), 0)
    torch.cuda.synchronize()
    v = dw.kernel_variant()
    assert v["leaf_kinds"] == 1 and v["tree"] == "sah" and v["lds_mode"] >= 1, v
    dw.release()
    size = R.Size2i(240, 135)
    _drain_counts()
    shared = R.render(size, 1, 16, 50, world, seed=19)
    posted, helped, owned = _drain_counts()
    assert posted > 0 and posted == helped + owned, (posted, helped, owned)
    if name == "suzanne":  # trapped paths: blocks drain long after their first waves finish
        assert helped > 0, (posted, helped, owned)
    monkeypatch.setenv("RTW_NO_COOP_SHARE", "1")
    assert_bit_identical(shared, R.render(size, 1, 16, 50, world, seed=19), f"{name}: shared vs private drain")
    assert _drain_counts() == (0, 0, 0)
    monkeypatch.delenv("RTW_NO_COOP_SHARE")
    for cap in ("1", "3"):
        monkeypatch.setenv("RTW_MB_CAP", cap)
        assert_bit_identical(shared, R.render(size, 1, 16, 50, world, seed=19), f"{name}: {cap} posts per batch")
        posted, helped, owned = _drain_counts()
        assert posted > 0 and posted == helped + owned, (cap, posted, helped, owned)


def test_progress_callback_reports_and_keeps_bits(worlds):
    """rtw_render_progress (the reference's progress thread, rendering.rs:140-157): monotone
    (done, total) reports ending at total, and the image equals rtw_render's."""
    world = worlds("final_scene1")
    size = R.Size2i(1920, 1080)
    seen = []
    img = R.render(size, 1, 48, 50, world, seed=5, progress=lambda d, t: seen.append((d, t)))
    total = 1920 * 1080 * 48
    assert seen and seen[-1] == (total, total)
    assert all(t == total for _, t in seen)
    assert all(a[0] <= b[0] for a, b in zip(seen, seen[1:]))
    assert_bit_identical(img, R.render(size, 1, 48, 50, world, seed=5), "progress render")


def test_device_encoder_matches_host():
    """rtw_encode_rgb8_device (the device to_rgb8_gamma2) == the host encoder, byte for byte, on
    random and special values (NaN, infinities, negatives, the 255 boundary)."""
    import torch

    from raytracinginaweekend_amd.image_io import to_rgb8_gamma2
    from raytracinginaweekend_amd.rendering import encode_rgb8_device

    rng = np.random.default_rng(5)
    special = np.array([0.0, -0.0, 1.0, 0.25, 1e30, -1.0, np.nan, np.inf, -np.inf, (255.0 / 256) ** 2,
                        (254.999 / 256) ** 2], np.float32)
    x = np.concatenate([special, rng.random(30000).astype(np.float32), rng.lognormal(0, 3, 3001).astype(np.float32)])
    x = x[: len(x) // 3 * 3]
    d = torch.from_numpy(x).to("cuda:0")
    out = torch.zeros(len(x), dtype=torch.uint8, device="cuda:0")
    encode_rgb8_device(d.data_ptr(), len(x) // 3, out.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), to_rgb8_gamma2(x.reshape(-1, 3)).ravel())


@pytest.mark.parametrize("name,parts,buffer_bytes", [("suzanne", 1, 0), ("suzanne", 3, 0), ("final_scene1", 2, 0),
                                                     ("final_scene1", 1, 72 * 40 * 12 * 8)])
def test_cost_ordered_frames_are_bit_identical(worlds, name, parts, buffer_bytes, monkeypatch):
    """Frames after the first of a partition shape run their tiles in measured-cost order
    (render_frame's work order); every frame must equal the oracle bit for bit, whatever the order."""
    import torch

    from raytracinginaweekend_amd.distributed import FrameRenderer, FrameSpec, untile_host

    if buffer_bytes:  # several launches per frame (8 samples each), each in cost order
        monkeypatch.setenv("RTW_SAMPLE_BUFFER_BYTES", str(buffer_bytes))
    world = worlds(name)
    size = R.Size2i(72, 40)
    spec = FrameSpec(size, 24, 50, 5)
    ref = O.render(world, R.render_params(size, 24, 50, seed=5))
    bufs = []
    for rank in range(parts):
        fr = FrameRenderer(world, spec, rank, parts, 0)
        frames = []
        for _ in range(3):  # chunk-major, then cost order twice
            fr.launch()
            torch.cuda.synchronize()
            frames.append((fr.image if parts == 1 else fr.tiles).cpu().numpy().copy())
        for f in frames[1:]:
            assert_bit_identical(f, frames[0], f"{name} frame order rank {rank}")
        bufs.append(frames[-1])
    img = bufs[0].reshape(-1, 3) if parts == 1 else untile_host(np.concatenate(bufs), size, spec.tile, parts, len(bufs[0]))
    assert_bit_identical(img, ref, name)


@pytest.mark.parametrize("threads,spp,buffer_bytes", [(1, 16, 0), (3, 16, 0), (16, 16, 0), (16, 5, 0), (3, 37, 40 * 24 * 12 * 5),
                                                      (7, 37, 40 * 24 * 12 * 8), (64, 37, 0), (1000, 16, 0),
                                                      (64, 37, 40 * 24 * 12 * 40)])
def test_thread_count_planes_bit_exact(worlds, threads, spp, buffer_bytes, monkeypatch):
    """thread_count > 1: the device accumulation reproduces split_work_tasks + merge_planes
    (rendering.rs:222-252) bit for bit against the oracle's ctr-mode plane merge (itself checked
    against a numpy restatement in tests/test_planes.py): merged straight from the colours in one
    launch (no plane buffer, also for thread_count > spp), and with plane partials carried across
    launches (the plane buffer's bytes taken out of RTW_SAMPLE_BUFFER_BYTES first)."""
    if buffer_bytes:
        monkeypatch.setenv("RTW_SAMPLE_BUFFER_BYTES", str(buffer_bytes))
    world = worlds("final_scene1")
    size = R.Size2i(40, 24)
    gpu = R.render(size, threads, spp, 50, world, seed=21)
    ref = O.render(world, R.render_params(size, spp, 50, seed=21, thread_count=threads), O.RNG_CTR)
    assert_bit_identical(gpu, ref, f"T={threads} spp={spp}")
    if threads > 1:  # a different plane split really changes bits somewhere (the merge is not a no-op)
        one = O.render(world, R.render_params(size, spp, 50, seed=21), O.RNG_CTR)
        assert not np.array_equal(one.view(np.uint32), ref.view(np.uint32))


def test_one_world_two_streams_bit_exact(worlds):
    """Two frames of one resident world issued back to back on two streams: the second waits for the
    first (they share the world's queue and colour buffers), and both equal the oracle."""
    import torch

    world = worlds("final_scene1")
    size = R.Size2i(64, 36)
    dw = R.DeviceWorld(world, 0)
    p1 = R.render_params(size, 6, 50, seed=11)
    p2 = R.render_params(size, 5, 50, seed=12)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.zeros(size.count() * 3, dtype=torch.float32, device="cuda:0")
    b = torch.zeros_like(a)
    dw.render_into(p1, a.data_ptr(), s1.cuda_stream)
    dw.render_into(p2, b.data_ptr(), s2.cuda_stream)
    torch.cuda.synchronize()
    assert_bit_identical(a.cpu().numpy().reshape(-1, 3), O.render(world, p1), "stream 1")
    assert_bit_identical(b.cpu().numpy().reshape(-1, 3), O.render(world, p2), "stream 2")


@pytest.mark.parametrize("name,parts", [("final_scene1", 1), ("earth_motion", 1), ("suzanne", 1), ("final_scene1", 3)])
def test_whole_pixel_items_bit_exact(worlds, name, parts, monkeypatch):
    """Whole-pixel work items (RTW_WHOLE_PIXEL=1: one lane renders all of a pixel's samples in order and
    sums them in registers, no colour buffer): the oracle's bits, in image layout and as tile partitions,
    over a chunk-major first frame and cost-ordered later frames."""
    import torch

    from raytracinginaweekend_amd.distributed import FrameRenderer, FrameSpec, untile_host

    monkeypatch.setenv("RTW_WHOLE_PIXEL", "1")
    world = worlds(name)
    size = R.Size2i(72, 40)
    spec = FrameSpec(size, 9, 50, 7)
    ref = O.render(world, R.render_params(size, 9, 50, seed=7))
    bufs = []
    for rank in range(parts):
        fr = FrameRenderer(world, spec, rank, parts, 0)
        for _ in range(2):
            fr.launch()
            torch.cuda.synchronize()
            bufs_r = (fr.image if parts == 1 else fr.tiles).cpu().numpy().copy()
            lf = fr.dworld.last_frame()  # rtw_world_last_frame: one launch of whole-pixel items
            assert lf["whole_pixel"] and lf["launches"] == 1 and lf["trace_min"] == 16, lf
            # the whole-pixel kernel variant (WP = true), except a GEN kernel: it takes either item kind at run
            # time (rtw_world_kernel_name: render_kernel<STATS, LDS, LK, TX, GEN, WP>)
            kname = fr.dworld.kernel_variant()["name"]
            args = kname[kname.index("<") + 1:-1].split(", ")
            assert len(args) == 6 and args[0] == "false" and args[5] == ("false" if args[4] == "true" else "true"), kname
            if parts == 1:
                assert_bit_identical(bufs_r.reshape(-1, 3), ref, f"{name} whole-pixel items")
        bufs.append(bufs_r)
    if parts > 1:
        img = untile_host(np.concatenate(bufs), size, spec.tile, parts, len(bufs[0]))
        assert_bit_identical(img, ref, f"{name} whole-pixel items, {parts} partitions")


def test_two_children_walk_ties_and_grazing_hits(monkeypatch):
    """The plain-sphere worlds' two-children SAH walk (its lane state and stack hold a node's children
    packed 16 + 16 bits) on coincident spheres of different materials and touching spheres:
    the oracle's bits, and the reference-tree loop's on a GPU-filling frame."""
    world = _tie_world(mesh=False)
    assert _kernel_tree(world) == "sah"
    size = R.Size2i(96, 54)
    gpu = R.render(size, 1, 8, 50, world, seed=47)
    assert_bit_identical(gpu, O.render(world, R.render_params(size, 8, 50, seed=47)), "sphere tie world")
    big = R.Size2i(480, 270)
    sah = R.render(big, 1, 4, 50, world, seed=47)
    monkeypatch.setenv("RTW_NO_SAH", "1")
    assert_bit_identical(sah, R.render(big, 1, 4, 50, world, seed=47), "sphere tie world, SAH vs reference tree")


def test_whole_pixel_threshold_stays_fixed_after_tuning(worlds, monkeypatch):
    """a whole-pixel frame runs at its fixed threshold (16) even after a per-sample frame of
    the same world has tuned one on the device (plain-sphere worlds keep the tuner only with
    RTW_TUNE_SPHERES=1; their default is a fixed threshold)."""
    import torch

    monkeypatch.setenv("RTW_TUNE_SPHERES", "1")
    world = worlds("final_scene1")
    dw = R.DeviceWorld(world, 0)
    big = R.render_params(R.Size2i(1920, 1080), 32, 50, seed=3)  # tuning needs >= 26 passes over the slots
    out = torch.empty(1920 * 1080 * 3, dtype=torch.float32, device="cuda:0")
    dw.render_into(big, out.data_ptr(), 0)  # per-sample items, long enough to host the tuning epochs
    torch.cuda.synchronize()
    assert dw.last_frame()["whole_pixel"] == 0
    assert dw.tuned_trace_min() > 0, "the per-sample frame did not tune a threshold"
    monkeypatch.setenv("RTW_WHOLE_PIXEL", "1")
    size = R.Size2i(64, 36)
    small = torch.empty(64 * 36 * 3, dtype=torch.float32, device="cuda:0")
    p = R.render_params(size, 5, 50, seed=3)
    dw.render_into(p, small.data_ptr(), 0)
    torch.cuda.synchronize()
    lf = dw.last_frame()
    assert lf["whole_pixel"] == 1 and lf["trace_min"] == 16, lf
    assert_bit_identical(small.cpu().numpy().reshape(-1, 3), O.render(world, p), "whole pixel after tuning")


def _sah_nodes(world, budget, monkeypatch) -> tuple:
    """(SAH nodes, leaves) of the tree build_sah_tables makes at a spatial-split budget (host only)."""
    import ctypes as C

    from raytracinginaweekend_amd import _native as N

    monkeypatch.setenv("RTW_SAH_SPLIT_BUDGET", str(budget))
    fn = N.lib().rtw_debug_sah_tree
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    out = (C.c_double * 10)()
    N.check(fn(C.cast(world.ptr(), C.c_void_p), out))
    assert out[4] == 1.0
    return int(out[0]), world.raw.leaf_count


def _split_tie_world():
    """Ties on a spatially split tree: long slivers crossing near a hub (the shape of the OBJ fan bug's
    origin triangles, obj_loader.rs:227-264, whose overlapping boxes spatial splits cut), twice over with
    different materials (every hit on them is a tie between two leaves the splits reference several
    times), above a row of spheres."""
    wb = R.WorldBuilder()
    mats = [wb.material_lambert_solid((0.8, 0.2, 0.2)), wb.material_lambert_solid((0.2, 0.8, 0.2)),
            wb.material_metal_solid((0.7, 0.7, 0.7), 0.1), wb.material_dielectric(1.5)]
    g = wb.new_group()
    g.add(wb.new_obj_sphere(100.0, mats[0]).translate((0.0, -100.0, 0.0)))
    for k in range(5):
        g.add(wb.new_obj_sphere(0.25, mats[k % 4]).translate((-1.0 + 0.5 * k, 0.25, 1.0)))
    hub = np.array([0.0, 1.2, -0.8], np.float32)
    n = np.array([0.0, 0.0, 1.0], np.float32)
    tris = []
    rs = np.random.default_rng(5)
    for _ in range(40):  # spikes: the fan bug's (v0, ORIGIN, v2) slivers radiating from one point
        d = rs.normal(size=3)
        d /= np.linalg.norm(d)
        p = np.cross(d, [0.3, 1.0, 0.2])
        p /= np.linalg.norm(p)
        tip = hub + 1.5 * d
        a, b = tip - 0.12 * p, tip + 0.12 * p
        base = hub - 1.2 * d  # crossing near the hub (spikes through one common point get no split)
        tris.append(list(base) + list(a) + list(b) + list(n) * 3 + [0.0] * 6)
    fan = np.array(tris, np.float32)
    g.add(wb.new_mesh(fan, mats[1]))
    g.add(wb.new_mesh(fan, mats[2]))
    cam = R.Camera.build().vertical_fov(40.0, 9.0 / 16.0).position((0.3, 1.2, 5.0)).look_at((0, 1, 0), (0, 0.8, 0)).build()
    return g.build().finish(wb, R.BackgroundColor.sky(), cam)


def test_spatial_split_tree_ties_bit_exact(monkeypatch):
    """ties on a tree whose spatial splits duplicate the fan's coincident slivers (budget 4 extra
    references per leaf, far above the default): a leaf met twice must not clear the tie flag another leaf
    set in between.  Bit-exact against the oracle and the reference tree."""
    world = _split_tie_world()
    nodes, leaves = _sah_nodes(world, 4, monkeypatch)
    assert nodes > leaves - 1, f"no spatial split: {nodes} nodes for {leaves} leaves"
    assert _kernel_tree(world).startswith("sah")
    size = R.Size2i(96, 54)
    gpu = R.render(size, 1, 8, 50, world, seed=31)
    assert_bit_identical(gpu, O.render(world, R.render_params(size, 8, 50, seed=31)), "tie world, split tree")
    big = R.Size2i(480, 270)
    sah = R.render(big, 1, 4, 50, world, seed=31)
    monkeypatch.setenv("RTW_NO_SAH", "1")
    assert_bit_identical(sah, R.render(big, 1, 4, 50, world, seed=31), "tie world split tree vs reference tree")


def test_suzanne_large_split_budget_bit_exact(worlds, monkeypatch):
    """suzanne on a spatial-split tree far beyond the default budget (4 extra references per leaf; the LDS
    mode-2 guard off, RTW_SAH_IGNORE_LDS): its shared mesh edges give exact ties between leaves referenced
    several times.  Bit-exact against the oracle and the reference tree."""
    world = worlds("suzanne")
    monkeypatch.setenv("RTW_SAH_IGNORE_LDS", "1")
    nodes, leaves = _sah_nodes(world, 4, monkeypatch)
    assert nodes > leaves + leaves // 2, f"{nodes} nodes for {leaves} leaves"
    size = R.Size2i(48, 36)
    gpu = R.render(size, 1, 4, 50, world, seed=11)
    assert_bit_identical(gpu, O.render(world, R.render_params(size, 4, 50, seed=11)), "suzanne, split budget 4")
    big = R.Size2i(320, 180)
    sah = R.render(big, 1, 8, 50, world, seed=29)
    monkeypatch.setenv("RTW_NO_SAH", "1")
    assert_bit_identical(sah, R.render(big, 1, 8, 50, world, seed=29), "suzanne split budget 4 vs reference tree")


def test_suzanne_depth_capped_tree_in_lds_mode2(worlds, monkeypatch):
    """suzanne's split tree, rebuilt under the depth cap that lets its 16-bit stack, nodes and triangle records
    share the 160 KB (build_sah_tables), runs LDS mode 2 with the mesh's leaf records left out (leaf_record:
    its 968 triangles are leaves 0..967); bit-exact against the oracle.  A far tighter cap (11 levels: median
    splits under most of the tree) must give the reference tree's bits too."""
    import torch

    world = worlds("suzanne")
    dw = R.DeviceWorld(world, 0)
    out = torch.empty(16 * 16 * 3, dtype=torch.float32, device="cuda:0")
    dw.render_into(R.render_params(R.Size2i(16, 16), 1, 50), out.data_ptr(), 0)
    torch.cuda.synchronize()
    v = dw.kernel_variant()
    assert v["lds_mode"] == 2 and v["tree"].startswith("sah") and v["leaf_kinds"] == 1, v
    size = R.Size2i(48, 36)
    assert_bit_identical(R.render(size, 1, 4, 50, world, seed=7), O.render(world, R.render_params(size, 4, 50, seed=7)),
                         "suzanne, depth-capped tree, mode 2")
    monkeypatch.setenv("RTW_SAH_DEPTH_CAP", "11")
    big = R.Size2i(320, 180)
    sah = R.render(big, 1, 8, 50, world, seed=5)
    monkeypatch.setenv("RTW_NO_SAH", "1")
    assert_bit_identical(sah, R.render(big, 1, 8, 50, world, seed=5), "suzanne cap 11 vs reference tree")


def _prefix_world(seed: int = 9):
    """Two meshes then a sphere: the first mesh (an image-textured Lambertian, its leaf_info carries the
    uv flag) is the triangle prefix, the second (another material) is not (tri_prefix_of stops there)."""
    rng = np.random.default_rng(seed)
    wb = R.WorldBuilder()
    img = (rng.uniform(0, 255, (8, 16, 3))).astype(np.uint8)
    mat_a = wb.material_lambert(wb.texture_image_rgb8(img))
    mat_b = wb.material_metal_solid((0.8, 0.7, 0.6), 0.05)
    mat_g = wb.material_lambert_solid((0.5, 0.5, 0.5))
    g = wb.new_group()

    def soup(n, lo, hi):
        c = rng.uniform(lo, hi, (n, 1, 3))
        v = (c + rng.uniform(-0.3, 0.3, (n, 3, 3))).astype(np.float32)
        uv = rng.uniform(0.0, 1.0, (n, 6)).astype(np.float32)
        return np.concatenate([v.reshape(n, 9), np.tile(np.float32([0, 1, 0]), (n, 3)), uv], 1).astype(np.float32)

    g.add(wb.new_mesh(soup(120, (-2.0, 0.2, -1.0), (0.0, 2.0, 1.0)), mat_a))
    g.add(wb.new_mesh(soup(80, (0.0, 0.2, -1.0), (2.0, 2.0, 1.0)), mat_b))
    g.add(wb.new_obj_sphere(100.0, mat_g).translate((0.0, -100.0, 0.0)))
    cam = R.Camera.build().vertical_fov(50.0, 9.0 / 16.0).position((0.0, 1.5, 6.0)).look_at((0, 1, 0), (0, 1, 0)).build()
    return g.build().finish(wb, R.BackgroundColor.sky(), cam)


def test_triangle_prefix_world_bit_exact():
    """walk_leaf_record / leaf_info_of: the leading mesh's leaf records and leaf_info are made up (its
    material and uv flag), the second mesh's and the sphere's are read; bit-exact against the oracle."""
    world = _prefix_world()
    leaves = [world.raw.leaves[i] for i in range(world.raw.leaf_count)]
    p = 0
    while (p < len(leaves) and leaves[p].geom_kind == 3 and leaves[p].flags == 0 and leaves[p].geom_index == p
           and leaves[p].material == leaves[0].material):
        p += 1
    assert 0 < p < len(leaves) - 1, p  # a prefix, then leaves whose records are read
    size = R.Size2i(64, 36)
    assert_bit_identical(R.render(size, 1, 8, 50, world, seed=3), O.render(world, R.render_params(size, 8, 50, seed=3)),
                         "triangle prefix world")


def test_image_texture_record_paths_bit_exact():
    """The three ways to an image texel: a Lambertian whose material record carries the image (RTW_DMAT_IMAGE),
    one over an image 65 536 texels wide (too wide for the record's 16-bit size: the texture record path), and
    a metal over an image (no room in its record: the texture record path, through a checker too).  Bit-exact
    against the oracle."""
    rng = np.random.default_rng(21)
    wb = R.WorldBuilder()
    small = rng.integers(0, 256, (6, 10, 3), dtype=np.uint8)
    wide = rng.integers(0, 256, (1, 65536, 3), dtype=np.uint8)
    t_small = wb.texture_image_rgb8(small)
    t_wide = wb.texture_image_rgb8(wide)
    m_direct = wb.material_lambert(t_small)
    m_wide = wb.material_lambert(t_wide)
    m_metal = _ok_metal(wb, wb.texture_checker(2.0, t_small, wb.texture_solid((0.2, 0.3, 0.9))), 0.1)
    g = wb.new_group()
    g.add(wb.new_obj_sphere(100.0, m_wide).translate((0.0, -100.0, 0.0)))
    g.add(wb.new_obj_sphere(0.8, m_direct).translate((-1.0, 0.8, 0.0)))
    g.add(wb.new_obj_sphere(0.8, m_metal).translate((1.0, 0.8, 0.0)))
    cam = R.Camera.build().vertical_fov(45.0, 9.0 / 16.0).position((0.0, 1.5, 5.0)).look_at((0, 0.8, 0), (0, 1, 0)).build()
    world = g.build().finish(wb, R.BackgroundColor.sky(), cam)
    size = R.Size2i(64, 36)
    assert_bit_identical(R.render(size, 1, 8, 50, world, seed=4), O.render(world, R.render_params(size, 8, 50, seed=4)),
                         "image texture record paths")


def _ok_metal(wb, tex: int, fuzz: float) -> int:
    from raytracinginaweekend_amd import _native as N

    r = N.lib().rtw_material_metal(wb._b, tex, fuzz)
    assert r >= 0
    return r


@pytest.mark.parametrize("n_tri,mode2", [(300, True), (1100, True), (2000, False)])
def test_triangle_records_lds_fallback(n_tri, mode2):
    """LDS mode 2 holds the triangle records component-major at the world's own stride (its triangle
    count: 1100 triangles fit, the 1024-record limit of rounds 2-5 is gone); a mesh world whose records
    do not fit falls back to mode 1 (records from L2), which rtw_world_kernel reports, and both render
    the oracle's bits."""
    import torch

    world = _soup_world(n_tri)
    dw = R.DeviceWorld(world, 0)
    out = torch.empty(16 * 16 * 3, dtype=torch.float32, device="cuda:0")
    dw.render_into(R.render_params(R.Size2i(16, 16), 1, 50), out.data_ptr(), 0)
    torch.cuda.synchronize()
    v = dw.kernel_variant()
    assert (v["lds_mode"] == 2) == mode2 and v["lds_mode"] >= 1, v
    # the exact template name rocprofv3 prints (bench.py matches PMC rows by it): single-sample items, no GEN
    assert v["name"] == f"render_kernel<false, {v['lds_mode']}, {v['leaf_kinds']}, {v['tex_kinds']}, false, false>", v
    size = R.Size2i(40, 24)
    assert_bit_identical(R.render(size, 1, 4, 50, world, seed=13), O.render(world, R.render_params(size, 4, 50, seed=13)),
                         f"soup {n_tri}")


@pytest.mark.parametrize("n,folded", [(16384, True), (16385, False)])
def test_plain_sphere_fold_limit_keeps_sah(n, folded, monkeypatch):
    """the two-children walk's packed node words hold 15-bit children (at most 2^14 leaves);
    a plain-sphere world one leaf beyond keeps its SAH tree (unfolded records, the triangle loop's
    one-child walk) instead of silently falling back to the reference tree.  Both sides of the limit
    render the oracle's bits and the reference-tree loop's."""
    import torch

    world = _sphere_cloud(n)
    assert world.raw.leaf_count == n
    dw = R.DeviceWorld(world, 0)
    out = torch.empty(16 * 16 * 3, dtype=torch.float32, device="cuda:0")
    dw.render_into(R.render_params(R.Size2i(16, 16), 1, 50), out.data_ptr(), 0)
    torch.cuda.synchronize()
    v = dw.kernel_variant()
    dw.release()
    assert v["tree"] == "sah" and v["leaf_kinds"] == (0 if folded else 1), v
    size = R.Size2i(32, 18)
    gpu = R.render(size, 1, 2, 50, world, seed=7)
    assert_bit_identical(gpu, O.render(world, R.render_params(size, 2, 50, seed=7)), f"{n} spheres")
    big = R.Size2i(160, 90)
    sah = R.render(big, 1, 2, 50, world, seed=7)
    monkeypatch.setenv("RTW_NO_SAH", "1")
    assert_bit_identical(sah, R.render(big, 1, 2, 50, world, seed=7), f"{n} spheres: SAH vs reference tree")


def test_plain_sphere_worlds_take_the_fixed_threshold(worlds, monkeypatch):
    """Round 6: per-sample frames of plain-sphere worlds run at the fixed threshold 8 without tuning (their
    8-way shares' short tuning epochs picked 24 on some ranks); RTW_TUNE_SPHERES=1 restores the tuner, and
    both give the oracle's bits."""
    import torch

    world = worlds("final_scene1")
    size = R.Size2i(640, 360)
    p = R.render_params(size, 8, 50, seed=11)
    ref = None
    for tune in (False, True):
        if tune:
            monkeypatch.setenv("RTW_TUNE_SPHERES", "1")
        dw = R.DeviceWorld(world, 0)
        out = torch.empty(size.count() * 3, dtype=torch.float32, device="cuda:0")
        dw.render_into(p, out.data_ptr(), 0)
        torch.cuda.synchronize()
        lf = dw.last_frame()
        assert lf["whole_pixel"] == 0, lf
        if not tune:
            assert lf["trace_min"] == 8 and dw.tuned_trace_min() == 0, (lf, dw.tuned_trace_min())
        img = out.cpu().numpy().reshape(-1, 3)
        if ref is None:
            ref = img
        else:
            assert_bit_identical(img, ref, "tuned vs fixed threshold")
        dw.release()
    small = R.Size2i(40, 24)
    assert_bit_identical(R.render(small, 1, 4, 50, world, seed=11),
                         O.render(world, R.render_params(small, 4, 50, seed=11)), "fixed threshold")
