"""The worlds of the first-hit tests (tests/test_first_hit_host.py on the CPU, tests/test_gpu_first_hit.py on the
device), built through WorldBuilder, at most 40 leaves each, solid background (D is final_scene1 as it is).

Every world states the cases it must reach, `CASES[name]`: (leaf kind, "front" | "back", wrapper) triples, a rect's
kind with its plane, wrapper one of "plain", "transform", "animation", "animation+transform" as the leaf's flags
in the finished tables say, a rotation with the sign of its y_sin (the builder folds a translation, and a mesh's
whole transformation, into the geometry: no triangle is ever hit under a wrapper), and `TEXTURES[name]`: the texture
kinds that end the albedo's chain ("dielectric": no texture, reads as white).  The tests assert at least
200 compared rays for each, so a world that silently stops exercising a case fails.

The cameras of A and B are pinholes at a fixed time that is not 0 (motion_blur(t, t)): an animated leaf is then
displaced by velocity * t while its box in the tree stays where the builder put it (apply_aabb is the identity),
so the ancestor-box rule of the caster removes real hits in these worlds."""
import numpy as np

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N

SIZE = R.Size2i(93, 54)  # no multiple of a tile, a wave or a block
ASPECT = 54.0 / 93.0
BACKGROUND = (0.25, 0.5, 0.75)
MIN_RAYS = 200

KIND_NAMES = {N.GEOM_SPHERE: "sphere", N.GEOM_RECT: "rect", N.GEOM_BOX: "box", N.GEOM_TRIANGLE: "triangle"}
PLANE_NAMES = {-1: "", N.PLANE_XY: "_xy", N.PLANE_XZ: "_xz", N.PLANE_YZ: "_yz"}
TEX_NAMES = {N.TEX_SOLID: "solid", N.TEX_CHECKER: "checker", N.TEX_MARBLE: "marble", N.TEX_IMAGE: "image",
             -2: "dielectric"}


def wrapper_name(flags: int, y_sin: float = 0.0) -> str:
    """"plain", "animation", "transform" and "animation+transform" by the leaf's flags; a rotation adds the sign of
    its y_sin, "transform(+)" or "transform(-)", so that a rotation by +theta and one by -theta are cases apart."""
    sign = "(+)" if y_sin > 0 else "(-)" if y_sin < 0 else ""
    names = [n for bit, n in ((N.LEAF_ANIMATION, "animation"), (N.LEAF_TRANSFORM, "transform" + sign)) if flags & bit]
    return "+".join(names) or "plain"


CASES = {
    "A": {("sphere", "front", "plain"), ("sphere", "back", "plain"), ("sphere", "front", "animation")},
    "A_lens": {("sphere", "front", "plain"), ("sphere", "back", "plain"), ("sphere", "front", "animation")},
    "B": {("rect_xz", "front", "plain"), ("rect_xz", "back", "plain"), ("rect_yz", "front", "plain"),
          ("rect_yz", "back", "plain"), ("rect_xy", "back", "plain"), ("box", "front", "plain"),
          ("box", "front", "transform(+)"), ("box", "front", "transform(-)"), ("box", "front", "animation"),
          ("box", "front", "animation+transform(+)")},
    "B_behind": {("rect_xy", "front", "plain")},
    "B_inside": {("box", "back", "transform(+)")},
    "C": {("triangle", "front", "plain"), ("triangle", "back", "plain"), ("rect_xz", "back", "plain")},
    "D": {("sphere", "front", "plain")},
}
TEXTURES = {
    "A": {"solid", "checker", "marble", "image", "dielectric"},
    "A_lens": {"solid", "checker", "marble", "image", "dielectric"},
    "B": {"solid", "marble", "image"},
    "B_behind": {"image"},
    "B_inside": {"marble"},
    "C": {"image", "solid"},
    "D": {"solid"},
}
NAMES = list(CASES)


def _image(seed):
    """A 7 x 5 random rgb8: no dimension is a power of two."""
    return np.random.default_rng(seed).integers(0, 256, (5, 7, 3), dtype=np.uint8)


def _camera(position, target, fov, time=None, aperture=None):
    cam = R.Camera.build().vertical_fov(fov, ASPECT).position(position).look_at_focus((0, 1, 0), target)
    if aperture is not None:
        cam = cam.aperture(aperture)
    if time is not None:
        cam = cam.motion_blur(*time)
    return cam.build()


def world_a(lens: bool = False):
    """Spheres: plain and animated ones, a ground sphere, one sphere that encloses the camera (every ray that
    reaches it takes the larger root and a back-face normal); checker, marble, image and dielectric materials."""
    wb = R.WorldBuilder()
    solid = lambda c: wb.material_lambert_solid(c)
    image = wb.material_lambert(wb.texture_image_rgb8(_image(1)))
    image2 = wb.material_lambert(wb.texture_image_rgb8(_image(2)))
    marble = wb.material_lambert(wb.texture_marble(4.0, R.Rng()))
    checker = wb.material_lambert(wb.texture_checker(2.5, wb.texture_solid((0.2, 0.3, 0.1)), wb.texture_marble(1.5, R.Rng())))
    glass = wb.material_dielectric(1.5)
    g = wb.new_group()
    g.add(wb.new_obj_sphere_ground(100.0, 0.0, checker))
    g.add(wb.new_obj_sphere(40.0, image2).translate((1.0, 2.0, -3.0)))  # encloses the camera
    row = [(image, 0.9), (marble, 0.8), (glass, 0.9), (solid((0.7, 0.3, 0.2)), 0.9)]
    for k, (m, r) in enumerate(row):
        g.add(wb.new_obj_sphere(r, m).translate((-3.3 + 2.2 * k, r, 0.0)))
    moving = [(image, (-0.8, 0.3, 0.0)), (solid((0.2, 0.8, 0.8)), (0.6, 0.0, 0.0)), (marble, (0.0, 0.3, 0.4))]
    for k, (m, v) in enumerate(moving):
        g.add(wb.new_obj_sphere(0.8, m).translate((-2.4 + 2.4 * k, 2.6, -0.5)).animate_moving(v))
    # one that rises from the floor to the camera's height: the boxes above it in the tree stay below the camera, so
    # hit_cond refuses every ray that climbs (its upper half is not there: the ancestor-box rule at work)
    g.add(wb.new_obj_sphere(0.6, solid((0.9, 0.2, 0.6))).translate((-0.2, 0.6, 2.9)).animate_moving((0.0, 1.75, 0.0)))
    for k in range(6):  # small ones in front, overlapping the rows in the image
        g.add(wb.new_obj_sphere(0.3, solid((0.1 + 0.15 * k, 0.5, 0.9 - 0.1 * k))).translate((-2.5 + k, 0.3, 1.8)))
    if lens:
        cam = _camera((0.4, 1.9, 7.0), (0.0, 1.4, 0.0), 60.0, time=(0.25, 1.0), aperture=0.3)
    else:
        cam = _camera((0.4, 1.9, 7.0), (0.0, 1.4, 0.0), 60.0, time=(0.75, 0.75))
    return g.build().finish(wb, R.BackgroundColor.solid(BACKGROUND), cam)


def world_b(view: str = "front"):
    """Rects of all three planes seen from both sides, a translated box, boxes under rotate_around_up(+-25) and
    translate, an animated box, a rotated and animated box.  view: "front", "behind" (the XY wall from its other side) or "inside" (the camera
    sits inside the box rotated by +25: every ray takes the exit plane and a far normal)."""
    wb = R.WorldBuilder()
    solid = lambda c: wb.material_lambert_solid(c)
    image = wb.material_lambert(wb.texture_image_rgb8(_image(3)))
    marble = wb.material_lambert(wb.texture_marble(3.0, R.Rng()))
    g = wb.new_group()
    g.add(wb.new_obj_rect_xz((0.0, 0.0, 0.0), 11.0, 10.0, image))          # floor: seen from above (back face)
    g.add(wb.new_obj_rect_xz((0.0, 4.2, -1.0), 9.0, 7.0, marble))          # ceiling: seen from below (front face)
    g.add(wb.new_obj_rect_yz((-4.8, 2.5, -0.5), 5.0, 9.0, solid((0.8, 0.2, 0.2))))  # left wall (back)
    g.add(wb.new_obj_rect_yz((4.45, 2.5, -1.0), 5.0, 7.0, image))           # right wall (front)
    g.add(wb.new_obj_rect_xy((0.0, 2.0, -3.5), 9.0, 4.0, image))           # far wall: back from the front view
    s = 1.7
    g.add(wb.new_obj_box(s, s, s, solid((0.8, 0.8, 0.2))).translate((-4.1, 0.0, 0.0)))
    g.add(wb.new_obj_box(s, s, s, marble).rotate_around_up(25.0).translate((-1.9, 0.0, 0.3)))
    g.add(wb.new_obj_box(s, s, s, solid((0.3, 0.8, 0.3))).rotate_around_up(-25.0).translate((0.9, 0.0, -0.5)))
    g.add(wb.new_obj_box(s, s, s, image).translate((2.6, 0.0, 0.0)).animate_moving((0.0, 1.0, 0.3)))
    # Animation(Transformation(Surface)): rotated, then moving along x and z, so the order of the two inverses shows
    # (the builder composes parent first: the box is moved, then turned about the world's origin; it floats)
    g.add(wb.new_obj_box(1.2, 1.2, 1.2, solid((0.2, 0.3, 0.9))).rotate_around_up(35.0).translate((-1.56, 2.5, 0.13))
          .animate_moving((-0.7, 0.0, 0.5)))
    if view == "front":
        cam = _camera((0.2, 2.1, 6.0), (0.0, 1.5, 0.0), 84.0, time=(0.75, 0.75))
    elif view == "behind":
        cam = _camera((-0.6, 2.4, -9.0), (0.0, 1.8, 0.0), 60.0, time=(0.75, 0.75))
    else:  # the box rotated by +25 holds (-1.9 .. , 0 .. 1.7, ..): its centre
        c, sn = np.cos(np.radians(25.0)), np.sin(np.radians(25.0))
        centre = (-1.9 + c * s / 2 + sn * s / 2, s / 2, 0.3 - sn * s / 2 + c * s / 2)
        cam = _camera(centre, (centre[0] + 1.0, centre[1] + 0.2, centre[2] - 2.0), 90.0, time=(0.75, 0.75))
    return g.build().finish(wb, R.BackgroundColor.solid(BACKGROUND), cam)


def _sheet(origin, du, dv, nu, nv, bend, flip, rng):
    """A bent sheet of 2 nu nv triangles: (n, 24) f32 records [positions 3x3, normals 3x3, uvs 3x2].  The vertex
    normals are the sheet's smooth normal plus a random tilt (never the face normal, not unit); `flip` turns them
    to the sheet's other side."""
    o, du, dv = (np.asarray(v, np.float64) for v in (origin, du, dv))
    up = np.cross(du, dv)
    up /= np.linalg.norm(up)
    verts = {}
    for j in range(nv + 1):
        for i in range(nu + 1):
            s, t = i / nu, j / nv
            p = o + s * du + t * dv + up * bend * np.sin(3.0 * s + 2.0 * t)
            n = up + 0.35 * rng.uniform(-1, 1, 3)
            n *= rng.uniform(0.7, 1.3) * (-1.0 if flip else 1.0)
            verts[i, j] = (p, n, (0.05 + 0.9 * s, 0.05 + 0.9 * t))
    tris = []
    for j in range(nv):
        for i in range(nu):
            for corners in (((i, j), (i + 1, j), (i + 1, j + 1)), ((i, j), (i + 1, j + 1), (i, j + 1))):
                ps, ns, uvs = zip(*(verts[c] for c in corners))
                tris.append([x for p in ps for x in p] + [x for n in ns for x in n] + [x for uv in uvs for x in uv])
    return np.asarray(tris, np.float32)


def world_c():
    """A mesh of 24 triangles in two sheets through new_mesh, per-vertex normals that are not the face normal (one
    sheet's turned away: back faces), uvs, an image texture, under rotate_around_up + translate; a floor rect."""
    rng = np.random.default_rng(11)
    wb = R.WorldBuilder()
    image = wb.material_lambert(wb.texture_image_rgb8(_image(4)))
    g = wb.new_group()
    g.add(wb.new_mesh(_sheet((-2.6, 0.3, 0.0), (2.4, 0.0, 0.4), (0.0, 2.4, -0.5), 3, 2, 0.15, False, rng), image)
          .rotate_around_up(30.0).translate((0.3, 0.1, -0.4)))
    g.add(wb.new_mesh(_sheet((0.3, 0.4, 0.2), (2.3, 0.2, -0.3), (0.1, 2.2, 0.4), 3, 2, 0.2, True, rng),
                      wb.material_lambert_solid((0.9, 0.6, 0.1)))
          .rotate_around_up(-20.0).translate((0.2, 0.0, 0.5)))
    g.add(wb.new_obj_rect_xz((0.0, 0.0, 0.0), 9.0, 9.0, image))
    cam = _camera((0.2, 1.8, 5.0), (0.0, 1.4, 0.0), 65.0)
    return g.build().finish(wb, R.BackgroundColor.solid(BACKGROUND), cam)


_cache = {}


def world(name: str, demo=None):
    """The world `name` of NAMES (cached); D needs `demo`, the session's demo-world getter."""
    if name not in _cache:
        if name == "D":
            _cache[name] = demo("final_scene1") if demo is not None else R.demo_world("final_scene1")
        else:
            _cache[name] = {"A": lambda: world_a(False), "A_lens": lambda: world_a(True),
                            "B": lambda: world_b("front"), "B_behind": lambda: world_b("behind"),
                            "B_inside": lambda: world_b("inside"), "C": world_c}[name]()
    return _cache[name]
