"""Small worlds for every native (leaf kinds, texture kinds) pair of the render-kernel dispatch table, and
worlds of a chosen size (plain helpers, no fixtures; tests/test_variant_worlds.py checks them on the CPU,
tests/test_gpu_variants.py renders them through every kernel variant).

World `lk` holds every leaf kind up to `lk` (launch_render's LK_* classes):
  LK_SPHERES  plain spheres (a translated sphere's offset is applied to its centre: it stays plain);
  LK_TRIS     + two meshes of different materials, the leading one first in the world (the triangle prefix);
  LK_PLAIN    + plain rects, one of them the DiffuseLight rect the light sampler takes;
  LK_WRAPPED  + a rotated and translated box, a translated box, a translated rect, a moving sphere;
  LK_ANY      + a constant-density volume over a sphere and over a box.
Every object has a material of its own, so a hit's material names the object (primary_materials)."""
import ctypes as C

import numpy as np

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N

LK_SPHERES, LK_TRIS, LK_PLAIN, LK_WRAPPED, LK_ANY = range(5)
TX_SOLID, TX_ANY = 0, 1
PAIRS = [(lk, tx) for lk in range(5) for tx in range(2)]
LK_NAMES = ("spheres", "tris", "plain", "wrapped", "any")
TX_NAMES = ("solid", "textured")


def pair_id(pair) -> str:
    return f"{LK_NAMES[pair[0]]}-{TX_NAMES[pair[1]]}"


# ------------------------------------------------------------------------------------------------
# launch_render's classification (rtw_world_upload: leaf_kinds / tex_kinds), restated
# ------------------------------------------------------------------------------------------------
def leaf_class(leaf) -> int:
    """The least LK_* loop that can test this leaf."""
    if leaf.flags & N.LEAF_VOLUME:
        return LK_ANY
    if leaf.flags != 0 or leaf.geom_kind == N.GEOM_BOX:
        return LK_WRAPPED
    if leaf.geom_kind == N.GEOM_RECT:
        return LK_PLAIN
    if leaf.geom_kind == N.GEOM_TRIANGLE:
        return LK_TRIS
    return LK_SPHERES


def classify(world) -> tuple:
    """(leaf kinds, texture kinds) of a world whose plain-sphere SAH tree, if any, is folded (at most 2^14
    leaves; beyond that a plain-sphere world is promoted to LK_TRIS)."""
    raw = world.raw
    lk = max([LK_SPHERES] + [leaf_class(raw.leaves[i]) for i in range(raw.leaf_count)])
    tx = TX_ANY if any(raw.textures[i].kind != N.TEX_SOLID for i in range(raw.texture_count)) else TX_SOLID
    return lk, tx


def tri_prefix(world) -> int:
    """tri_prefix_of: the leading run of plain triangle leaves i with triangle i and leaf 0's material."""
    raw, p = world.raw, 0
    while (p < raw.leaf_count and raw.leaves[p].geom_kind == N.GEOM_TRIANGLE and raw.leaves[p].flags == 0
           and raw.leaves[p].geom_index == p and raw.leaves[p].material == raw.leaves[0].material):
        p += 1
    return p


def texture_kinds_of(world, material: int) -> set:
    """The texture kinds a material can sample (a checker's branches included)."""
    raw = world.raw
    m = raw.materials[material]
    if m.kind == N.MAT_DIELECTRIC or m.texture < 0:
        return set()
    out, todo = set(), [m.texture]
    while todo:
        t = raw.textures[todo.pop()]
        out.add(t.kind)
        if t.kind == N.TEX_CHECKER:
            todo += [t.even, t.odd]
    return out


# ------------------------------------------------------------------------------------------------
# the ten variant worlds
# ------------------------------------------------------------------------------------------------
def _grid_mesh(origin, du, dv, nu: int, nv: int) -> np.ndarray:
    """A parallelogram origin + s du + t dv as nu x nv cells of two triangles: (2 nu nv, 24) f32 records
    [positions 3x3, normals 3x3, uvs 3x2] with the plane's normal and uv = (s, t)."""
    o, du, dv = (np.asarray(v, np.float64) for v in (origin, du, dv))
    n = np.cross(du, dv)
    n /= np.linalg.norm(n)
    tris = []

    def vert(i, j):
        s, t = i / nu, j / nv
        return list(o + s * du + t * dv), [s, t]

    for j in range(nv):
        for i in range(nu):
            for corners in (((i, j), (i + 1, j), (i + 1, j + 1)), ((i, j), (i + 1, j + 1), (i, j + 1))):
                ps, uvs = zip(*(vert(*c) for c in corners))
                tris.append([x for p in ps for x in p] + list(n) * 3 + [x for uv in uvs for x in uv])
    return np.asarray(tris, np.float32)


def _image(rng, h: int, w: int) -> np.ndarray:
    return rng.integers(32, 256, (h, w, 3), dtype=np.uint8)


def variant_world(lk: int, tx: int):
    """The world of leaf kinds `lk` and texture kinds `tx` (at most about 60 leaves)."""
    rng = np.random.default_rng(100 + 10 * lk + tx)
    wb = R.WorldBuilder()
    lib = N.lib()
    textured = tx == TX_ANY

    def lambert(color, tex=None):
        return wb.material_lambert(tex) if textured and tex is not None else wb.material_lambert_solid(color)

    def metal(color, fuzz, tex=None):
        if textured and tex is not None:
            return R.world._ok(lib.rtw_material_metal(wb._b, tex, fuzz))
        return wb.material_metal_solid(color, fuzz)

    def light(color, tex=None):
        if textured and tex is not None:
            return R.world._ok(lib.rtw_material_diffuse_light(wb._b, tex))
        return wb.material_diffuse_light_solid(color)

    def isotropic(color, tex=None):
        if textured and tex is not None:
            return R.world._ok(lib.rtw_material_isotropic(wb._b, tex))
        return wb.material_isotropic_solid(color)

    def image(h, w):
        return wb.texture_image_rgb8(_image(rng, h, w)) if textured else None

    checker = marble = None
    if textured:  # a checker with an image branch, a marble
        checker = wb.texture_checker(0.7, wb.texture_image_rgb8(_image(rng, 5, 9)), wb.texture_solid((0.9, 0.9, 0.8)))
        marble = wb.texture_marble(3.0, R.Rng())
    g = wb.new_group()
    if lk >= LK_TRIS:  # the leading mesh first: its triangles are leaves 0.. (the triangle prefix), image-textured
        g.add(wb.new_mesh(_grid_mesh((-2.4, 0.1, -1.0), (2.2, 0.0, 0.2), (0.0, 2.0, -0.3), 4, 3),
                          lambert((0.7, 0.6, 0.3), image(6, 10))))
        g.add(wb.new_mesh(_grid_mesh((0.2, 0.1, -0.4), (1.2, 0.0, 0.0), (0.0, 1.4, -0.6), 2, 2),
                          metal((0.8, 0.7, 0.6), 0.05)))
    g.add(wb.new_obj_sphere(100.0, lambert((0.5, 0.5, 0.5), checker)).translate((0.0, -100.0, 0.0)))
    front = [lambert((0.7, 0.3, 0.2), marble), metal((0.8, 0.8, 0.8), 0.1, image(4, 7)), wb.material_dielectric(1.5),
             lambert((0.2, 0.4, 0.8), image(7, 5)), light((2.0, 1.8, 1.5))]
    for k, m in enumerate(front):
        g.add(wb.new_obj_sphere(0.35, m).translate((-1.8 + 0.9 * k, 0.35, 1.6)))
    for k in range(8):
        m = (lambert((0.3 + 0.08 * k, 0.7 - 0.06 * k, 0.4)), metal((0.9, 0.6 + 0.04 * k, 0.4), 0.3),
             wb.material_dielectric(1.3 + 0.05 * k))[k % 3]
        g.add(wb.new_obj_sphere(0.2, m).translate((-2.1 + 0.6 * k, 1.2 + 0.15 * (k % 2), 0.3)))
    if lk >= LK_PLAIN:
        g.add(wb.new_obj_rect_xy((1.3, 2.2, -1.0), 1.8, 0.7, light((4.0, 4.0, 4.0), image(3, 8))).set_all_geo_as_poi())
        g.add(wb.new_obj_rect_xy((2.3, 0.8, -1.0), 1.0, 1.6, lambert((0.3, 0.7, 0.3), marble)))
        g.add(wb.new_obj_rect_yz((-2.8, 0.8, 0.5), 1.6, 2.0, metal((0.7, 0.7, 0.9), 0.0)))
    if lk >= LK_WRAPPED:
        g.add(wb.new_obj_box(0.6, 0.6, 0.6, lambert((0.8, 0.8, 0.2), checker)).rotate_around_up(25.0).translate((-1.5, 0.3, 2.6)))
        g.add(wb.new_obj_box(0.5, 0.5, 0.5, metal((0.6, 0.8, 0.6), 0.2)).translate((1.5, 0.25, 2.6)))
        # (a transformed leaf keeps its untransformed box, hittable.rs apply_aabb: the rect moves inside its plane)
        g.add(wb.new_obj_rect_xy((0.6, 0.45, 2.6), 0.6, 0.6, lambert((0.8, 0.3, 0.7), image(5, 5))).translate((0.15, 0.1, 0.0)))
        g.add(wb.new_obj_sphere(0.25, lambert((0.2, 0.8, 0.8))).translate((-0.5, 0.25, 2.6)).animate_moving((0.0, 0.4, 0.0)))
    if lk >= LK_ANY:
        g.add(wb.new_obj_sphere(0.45, isotropic((0.9, 0.9, 0.9), image(6, 6))).translate((-0.9, 0.45, 3.6))
              .set_all_geo_densitity(0.9))
        g.add(wb.new_obj_box(0.7, 0.7, 0.7, isotropic((0.1, 0.1, 0.1))).translate((0.9, 0.35, 3.6)).set_all_geo_densitity(0.9))
    cam = R.Camera.build().vertical_fov(70.0, 9.0 / 16.0).position((0.3, 2.0, 6.5)).look_at((0, 1, 0), (0.0, 0.4, 0.0))
    if lk >= LK_WRAPPED:
        cam = cam.motion_blur(0.0, 1.0)
    return g.build().finish(wb, R.BackgroundColor.sky(), cam.build())


# ------------------------------------------------------------------------------------------------
# worlds of a chosen size
# ------------------------------------------------------------------------------------------------
def soup_world(n_tri: int, seed: int = 5, textured: bool = False):
    """A random triangle soup over a ground sphere (mesh worlds of any size).  textured: the mesh, added first
    (the triangle prefix), is an image-textured Lambertian with random uvs."""
    rng = np.random.default_rng(seed)
    wb = R.WorldBuilder()
    mats = [wb.material_lambert_solid((0.7, 0.3, 0.2)), wb.material_metal_solid((0.8, 0.8, 0.8), 0.2)]
    g = wb.new_group()
    if not textured:
        g.add(wb.new_obj_sphere(100.0, mats[0]).translate((0.0, -100.0, 0.0)))
    c = rng.uniform((-2.0, 0.2, -2.0), (2.0, 2.2, 2.0), (n_tri, 1, 3))
    v = (c + rng.uniform(-0.25, 0.25, (n_tri, 3, 3))).astype(np.float32)
    uv = rng.uniform(0.0, 1.0, (n_tri, 6)).astype(np.float32) if textured else np.zeros((n_tri, 6), np.float32)
    tris = np.concatenate([v.reshape(n_tri, 9), np.tile(np.float32([0, 1, 0]), (n_tri, 3)), uv], 1).astype(np.float32)
    if textured:
        g.add(wb.new_mesh(tris, wb.material_lambert(wb.texture_image_rgb8(_image(rng, 8, 16)))))
        g.add(wb.new_obj_sphere(100.0, mats[0]).translate((0.0, -100.0, 0.0)))
    else:
        g.add(wb.new_mesh(tris, mats[1]))
    cam = R.Camera.build().vertical_fov(50.0, 9.0 / 16.0).position((0.0, 1.5, 6.0)).look_at((0, 1, 0), (0, 1, 0)).build()
    return g.build().finish(wb, R.BackgroundColor.sky(), cam)


def sphere_cloud(n: int, seed: int = 3):
    """n small plain spheres in a slab over a ground sphere (n - 1 spheres + ground = n leaves)."""
    rng = np.random.default_rng(seed)
    wb = R.WorldBuilder()
    mats = [wb.material_lambert_solid((0.7, 0.3, 0.2)), wb.material_metal_solid((0.8, 0.8, 0.8), 0.1),
            wb.material_dielectric(1.5)]
    g = wb.new_group()
    g.add(wb.new_obj_sphere(1000.0, mats[0]).translate((0.0, -1000.0, 0.0)))
    c = rng.uniform((-8.0, 0.05, -8.0), (8.0, 3.0, 8.0), (n - 1, 3)).astype(np.float32)
    for i in range(n - 1):
        g.add(wb.new_obj_sphere(0.04, mats[i % 3]).translate(tuple(float(x) for x in c[i])))
    cam = R.Camera.build().vertical_fov(50.0, 9.0 / 16.0).position((0.0, 2.0, 10.0)).look_at((0, 1, 0), (0, 1, 0)).build()
    return g.build().finish(wb, R.BackgroundColor.sky(), cam)


def big_soup(n: int, textured: bool = False):
    """A triangle soup of n triangles (n + 1 leaves with the ground sphere)."""
    return soup_world(n, textured=textured)


def big_wrapped(n: int, seed: int = 7, textured: bool = False):
    """n wrapped leaves in a slab over a ground sphere, translated boxes and moving spheres alternating
    (n + 1 leaves, n // 2 + n % 2 boxes, n // 2 + 1 spheres; LK_WRAPPED).  Solid textures, or with `textured`
    an image on the ground and on a third of the leaves (TX_ANY)."""
    rng = np.random.default_rng(seed)
    wb = R.WorldBuilder()
    c = rng.uniform((-6.0, 0.1, -6.0), (6.0, 3.0, 4.0), (n, 3)).astype(np.float32)
    mats = [wb.material_lambert_solid((0.7, 0.3, 0.2)), wb.material_metal_solid((0.8, 0.8, 0.8), 0.1),
            wb.material_dielectric(1.5), wb.material_lambert_solid((0.2, 0.5, 0.8))]
    if textured:
        mats[0] = wb.material_lambert(wb.texture_image_rgb8(_image(rng, 16, 32)))
        mats[3] = wb.material_lambert(wb.texture_image_rgb8(_image(rng, 6, 9)))
    g = wb.new_group()
    g.add(wb.new_obj_sphere(1000.0, mats[0]).translate((0.0, -1000.0, 0.0)))
    for i in range(n):
        at = tuple(float(x) for x in c[i])
        if i % 2 == 0:
            g.add(wb.new_obj_box(0.16, 0.16, 0.16, mats[1 + i // 2 % 3]).translate(at))
        else:
            g.add(wb.new_obj_sphere(0.09, mats[1 + i // 2 % 3]).translate(at).animate_moving((0.0, 0.15, 0.0)))
    cam = (R.Camera.build().vertical_fov(50.0, 9.0 / 16.0).position((0.0, 2.0, 10.0)).look_at((0, 1, 0), (0, 1, 0))
           .motion_blur(0.0, 1.0).build())
    return g.build().finish(wb, R.BackgroundColor.sky(), cam)


# ------------------------------------------------------------------------------------------------
# what the oracle's camera rays see
# ------------------------------------------------------------------------------------------------
def primary_materials(world, width: int, height: int) -> set:
    """The materials the oracle's closest hits of the camera rays through the pixel corners land on
    (rtw_oracle_camera_ray + rtw_oracle_scene_hit, one ray per pixel; a volume's hit is random)."""
    from oracle import pyoracle as O

    L = O.lib()
    seen = set()
    o, d, t = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    rs = (C.c_uint64 * 2)(0x9E3779B97F4A7C15, 0xD1B54A32D192ED03)
    h = O.OracleHit()
    inf = float("inf")
    for y in range(height):
        for x in range(width):
            L.rtw_oracle_camera_ray(C.byref(world.raw.camera), x / (width - 1), y / (height - 1), rs, o, d, C.byref(t))
            L.rtw_oracle_scene_hit(world.ptr(), o, d, t.value, 0.001, inf, rs, C.byref(h))
            if h.hit:
                seen.add(h.material)
    return seen
