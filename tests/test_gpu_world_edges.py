"""Worlds at the edges of what rtw_world_check accepts, rendered by the megakernel and compared with the oracle bit
for bit: one-leaf worlds (root = -1, no nodes), a tree exactly RTW_MAX_BVH_DEPTH levels deep, the longest checker
chain the device's loop finishes, Perlin lattices of 2 and of 256 points, 1 x 1 and 1 x N images, a scene light on
each plane.  Every world here passes the validator first (asserted): the refusals live in tests/test_world_check.py
and never reach a launch.  Frames are at most 48 x 27 at 4 spp; where the world takes the SAH tree it is rendered a
second time on the reference tree (RTW_NO_SAH=1).  No tolerances."""
import numpy as np
import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.world import check_world
from tests import variant_worlds as V
from tests.parity import assert_bit_identical
from tests.world_copy import OwnedWorld, add_chain, chain_world, tree_depth

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT, SPP, DEPTH, SEED = 48, 27, 4, 12, 23
KNOBS = ("RTW_LDS_MODE", "RTW_WHOLE_PIXEL", "RTW_NO_SAH", "RTW_LEAF_KINDS", "RTW_TEX_KINDS", "RTW_PRIMARY_LISTS",
         "RTW_CAMERA_BATCH", "RTW_FIRST_BOUNCE", "RTW_TRACE_MIN")
MAX_DEPTH, MAX_CHAIN = 32, 64


@pytest.fixture(autouse=True)
def _knobs_off(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def render(world, monkeypatch, env=None):
    """One frame of a fresh DeviceWorld: (image, kernel_variant())."""
    import torch

    with monkeypatch.context() as m:
        for k, v in (env or {}).items():
            m.setenv(k, v)
        dw = R.DeviceWorld(world, 0)  # (the upload reads RTW_NO_SAH)
        out = torch.empty(WIDTH * HEIGHT * 3, dtype=torch.float32, device="cuda:0")
        dw.render_into(R.render_params(R.Size2i(WIDTH, HEIGHT), SPP, DEPTH, seed=SEED), out.data_ptr(), 0)
        torch.cuda.synchronize()
        image, v = out.cpu().numpy().reshape(-1, 3), dw.kernel_variant()
        dw.release()
    return image, v


def oracle(world):
    return O.render(world, R.render_params(R.Size2i(WIDTH, HEIGHT), SPP, DEPTH, seed=SEED)).reshape(-1, 3)


def check_against_oracle(world, monkeypatch, what, leaf_kinds, tex_kinds, sah, depth):
    """The default launch (and the reference-tree launch of a world that takes the SAH tree) against the oracle."""
    assert check_world(world.raw) == depth == tree_depth(world.raw)
    ref = oracle(world)
    assert np.isfinite(ref).all() and ref.max() > 0.0  # a frame that shows something
    image, v = render(world, monkeypatch)
    assert (v["leaf_kinds"], v["tex_kinds"], v["tree"], v["sah"]) == (leaf_kinds, tex_kinds, "sah" if sah else "reference",
                                                                      1 if sah else 0), v
    assert_bit_identical(image, ref, what)
    if sah:
        image, r = render(world, monkeypatch, {"RTW_NO_SAH": "1"})
        assert (r["leaf_kinds"], r["tree"], r["sah"]) == (leaf_kinds, "reference", 0), r
        assert_bit_identical(image, ref, what + " (reference tree)")
    return v


def camera(position=(0.0, 0.6, 3.0), target=(0.0, 0.3, 0.0), blur=False):
    cam = R.Camera.build().vertical_fov(50.0, 9.0 / 16.0).position(position).look_at((0, 1, 0), target)
    return (cam.motion_blur(0.0, 1.0) if blur else cam).build()


# ---- one-leaf worlds: root = -1, no nodes --------------------------------------------------------------------------
def one_leaf(kind: str):
    wb = R.WorldBuilder()
    red = wb.material_lambert_solid((0.7, 0.3, 0.2))
    g, blur = wb.new_group(), False
    if kind == "sphere":
        g.add(wb.new_obj_sphere(0.5, red).translate((0.0, 0.4, 0.0)))  # (a translated sphere stays plain)
    elif kind == "rect":
        g.add(wb.new_obj_rect_xy((0.0, 0.4, 0.0), 1.6, 1.0, red))
    elif kind == "box":
        g.add(wb.new_obj_box(0.8, 0.6, 0.7, red))
    elif kind == "triangle":
        g.add(wb.new_mesh(V._grid_mesh((-0.8, 0.0, 0.0), (1.6, 0.0, 0.0), (0.0, 1.2, -0.3), 1, 1)[:1], red))
    elif kind == "triangle_image":  # the triangle prefix would be the whole world
        rgb = np.random.default_rng(3).integers(32, 256, (5, 7, 3), dtype=np.uint8)
        g.add(wb.new_mesh(V._grid_mesh((-0.8, 0.0, 0.0), (1.6, 0.0, 0.0), (0.0, 1.2, -0.3), 1, 1)[:1],
                          wb.material_lambert(wb.texture_image_rgb8(rgb))))
    elif kind == "transform":  # (the builder folds a sphere's own translation into its centre: the wrapper is set below)
        g.add(wb.new_obj_sphere(0.5, red).translate((0.0, 0.4, 0.3)))
    elif kind == "animation":
        g.add(wb.new_obj_sphere(0.5, red).translate((0.0, 0.3, 0.0)).animate_moving((0.0, 0.4, 0.0)))
        blur = True
    elif kind == "volume":
        g.add(wb.new_obj_sphere(0.6, wb.material_isotropic_solid((0.9, 0.9, 0.9))).translate((0.0, 0.4, 0.0))
              .set_all_geo_densitity(0.9))
    world = g.build().finish(wb, R.BackgroundColor.sky(), camera(blur=blur))
    if kind == "transform":  # Transformation(offset, rotation around y) over the sphere, as a box or a rect would carry it
        world = OwnedWorld(world)
        leaf = world.arrays["leaves"][0]
        leaf.flags = N.LEAF_TRANSFORM
        leaf.offset[:] = [0.2, 0.1, -0.3]
        leaf.y_sin, leaf.y_cos = float(np.sin(np.float32(np.pi / 6))), float(np.cos(np.float32(np.pi / 6)))
    return world


# kind -> (leaf kinds, texture kinds, the leaf's flags)
ONE_LEAF = {
    "sphere": (V.LK_SPHERES, V.TX_SOLID, 0),
    "rect": (V.LK_PLAIN, V.TX_SOLID, 0),
    "box": (V.LK_WRAPPED, V.TX_SOLID, 0),
    "triangle": (V.LK_TRIS, V.TX_SOLID, 0),
    "triangle_image": (V.LK_TRIS, V.TX_ANY, 0),
    "transform": (V.LK_WRAPPED, V.TX_SOLID, N.LEAF_TRANSFORM),
    "animation": (V.LK_WRAPPED, V.TX_SOLID, N.LEAF_ANIMATION),
    "volume": (V.LK_ANY, V.TX_SOLID, N.LEAF_VOLUME),
}


@pytest.mark.parametrize("kind", list(ONE_LEAF))
def test_one_leaf_world(kind, monkeypatch):
    world = one_leaf(kind)
    lk, tx, flags = ONE_LEAF[kind]
    raw = world.raw
    assert (raw.root, raw.node_count, raw.leaf_count) == (-1, 0, 1)
    assert raw.leaves[0].flags == flags
    assert V.classify(world) == (lk, tx)
    # no tree to replace: the reference walk stands on the leaf at once; a one-leaf world keeps no triangle prefix
    v = check_against_oracle(world, monkeypatch, kind, lk, tx, sah=False, depth=0)
    assert v["tri_prefix"] == 0 and v["name"].startswith("render_kernel<false, "), v
    assert v["lds_mode"] == (2 if kind.startswith("triangle") else 1), v


# ---- a tree exactly RTW_MAX_BVH_DEPTH levels deep ---------------------------------------------------------------------
def test_deepest_tree_plain_spheres(monkeypatch):
    """A left-deep chain over 33 spheres in a row, every node splitting on y: the rays of the upper half of the image
    that reach the far end hold one stack entry per level on the reference tree.  The world takes the SAH tree (the
    two-children walk, with the primary rays' leaf lists), then the reference tree with RTW_NO_SAH=1."""
    world = chain_world(MAX_DEPTH)
    check_against_oracle(world, monkeypatch, "chain of spheres", V.LK_SPHERES, V.TX_SOLID, sah=True, depth=MAX_DEPTH)


def test_deepest_tree_with_a_rect(monkeypatch):
    """The same chain with a rect as its deepest leaf: the one-child walk (SAH tree, then the reference tree)."""
    world = chain_world(MAX_DEPTH, extra_rect=True)
    check_against_oracle(world, monkeypatch, "chain with a rect", V.LK_PLAIN, V.TX_SOLID, sah=True, depth=MAX_DEPTH)


# ---- the deepest accepted checker chain ---------------------------------------------------------------------------
def chained(material_kind: int):
    """Spheres on a ground sphere; the ground's material (Lambertian or metal) samples a chain of 63 checkers whose
    even and odd are the next texture and which ends in a solid colour that is not black (the device's give-up value
    after 64 steps would show)."""
    wb = R.WorldBuilder()
    g = wb.new_group()
    ground = wb.material_lambert_solid((0.5, 0.5, 0.5)) if material_kind == N.MAT_LAMBERT else wb.material_metal_solid((0.5, 0.5, 0.5), 0.2)
    g.add(wb.new_obj_sphere(100.0, ground).translate((0.0, -100.0, 0.0)))
    g.add(wb.new_obj_sphere(0.4, wb.material_dielectric(1.5)).translate((-0.6, 0.4, 0.5)))
    g.add(wb.new_obj_sphere(0.4, wb.material_lambert_solid((0.2, 0.4, 0.8))).translate((0.6, 0.4, 0.2)))
    world = OwnedWorld(g.build().finish(wb, R.BackgroundColor.sky(), camera()))
    assert world.raw.materials[0].kind == material_kind  # add_chain hangs the chain on the first material
    add_chain(world, MAX_CHAIN)
    return world


@pytest.mark.parametrize("material_kind", [N.MAT_LAMBERT, N.MAT_METAL], ids=["lambert", "metal"])
def test_longest_checker_chain(material_kind, monkeypatch):
    world = chained(material_kind)
    check_against_oracle(world, monkeypatch, "checker chain", V.LK_SPHERES, V.TX_ANY, sah=True, depth=tree_depth(world.raw))
    # the chain's end colour reaches the frame: the ground under the camera's lower rows is neither black nor grey
    ref = oracle(world).reshape(HEIGHT, WIDTH, 3)
    assert (ref[-3:, :, 0] > 1.2 * ref[-3:, :, 2]).any()


# ---- Perlin lattices of 2 and of 256 points ----------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 8])
def test_marble_lattice(bits, monkeypatch):
    world = OwnedWorld(V.variant_world(V.LK_SPHERES, V.TX_ANY))  # a marble sphere in front, checker and image textures
    assert world.raw.perlin_count == 1
    p = world.arrays["perlins"][0]
    p.bits = bits
    rng = np.random.default_rng(40 + bits)
    for a in ("perm_x", "perm_y", "perm_z"):  # true permutations of 0 .. 2^bits - 1; the rest is never read
        perm = rng.permutation(1 << bits)
        for k in range(256):
            getattr(p, a)[k] = int(perm[k]) if k < (1 << bits) else 0xFFFFFFFF
    check_against_oracle(world, monkeypatch, f"marble bits {bits}", V.LK_SPHERES, V.TX_ANY, sah=True, depth=tree_depth(world.raw))


# ---- the smallest images -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)], ids=["1x1", "1xN", "Nx1"])
def test_smallest_images(shape, monkeypatch):
    """(height, width) of the image on the ground sphere and on a front sphere: the texel clamp at width - 1 = 0."""
    wb = R.WorldBuilder()
    rgb = np.random.default_rng(9).integers(32, 256, (*shape, 3), dtype=np.uint8)
    tex = wb.texture_image_rgb8(rgb)
    g = wb.new_group()
    g.add(wb.new_obj_sphere(100.0, wb.material_lambert(tex)).translate((0.0, -100.0, 0.0)))
    g.add(wb.new_obj_sphere(0.5, wb.material_lambert(tex)).translate((0.0, 0.5, 0.0)))
    g.add(wb.new_obj_sphere(0.3, wb.material_metal_solid((0.8, 0.8, 0.8), 0.0)).translate((0.9, 0.3, 0.4)))
    world = g.build().finish(wb, R.BackgroundColor.sky(), camera())
    assert (world.raw.images[0].height, world.raw.images[0].width) == shape
    check_against_oracle(world, monkeypatch, f"image {shape}", V.LK_SPHERES, V.TX_ANY, sah=True, depth=tree_depth(world.raw))


# ---- a scene light on each plane --------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [N.PLANE_XY, N.PLANE_XZ, N.PLANE_YZ], ids=["xy", "xz", "yz"])
def test_scene_light_on_each_plane(plane, monkeypatch):
    """A one-rect world (a Lambertian floor) whose light sampler aims at a rect region on `plane`: half of the floor's
    bounce rays are drawn towards it (light_generate) and every pdf mixes its value (light_value)."""
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(wb.new_obj_rect_xz((0.0, 0.0, 0.0), 4.0, 4.0, wb.material_lambert_solid((0.7, 0.6, 0.5))))
    world = OwnedWorld(g.build().finish(wb, R.BackgroundColor.sky(), camera(position=(0.0, 1.5, 3.0), target=(0.0, 0.0, 0.0))))
    assert (world.raw.root, world.raw.leaf_count, world.raw.has_light) == (-1, 1, 0)
    world.raw.has_light = 1
    light = world.raw.light
    light.plane = plane
    light.dist = {N.PLANE_XY: -1.5, N.PLANE_XZ: 2.0, N.PLANE_YZ: 1.5}[plane]
    # the region's two in-plane ranges (rect_geometry.rs:14-21: Xy -> x, y; Xz -> x, z; Yz -> y, z), above the floor
    light.r0[:], light.r1[:] = {N.PLANE_XY: ((-0.5, 0.7), (0.4, 1.3)), N.PLANE_XZ: ((-0.6, 0.5), (-0.4, 0.8)),
                                N.PLANE_YZ: ((0.5, 1.4), (-0.7, 0.6))}[plane]
    check_against_oracle(world, monkeypatch, f"light on plane {plane}", V.LK_PLAIN, V.TX_SOLID, sah=False, depth=0)
