"""The worlds of the path-step tests (tests/test_path_host.py on the CPU, tests/test_gpu_path.py on the device), built
through WorldBuilder, a dozen leaves each, cameras of 93 x 54.

  P-glass    a glass sphere (ior 1.5), a glass box under rotate_around_up(25) (its normal goes through the wrapper),
             a sphere of ior 0.8 (ratio > 1 on the FRONT face: total internal reflection from outside), one of ior 2.4 (a
             reflectance of 0.17 and more: the coin's heads on both faces); seen from
             outside by the camera and from inside by the paths' own later segments
  P-metal    metal spheres of fuzz 0, 0.3 and 1.0 (fuzzed directions below the surface are absorbed), a fuzzed metal
             mesh whose vertex normals are tilted 20-30 degrees from the face normal (the absorb test is on the shading
             normal), a metal floor seen on its back face and a metal canopy seen on its front face
  P-lambert  Lambert sphere, floor rect, rotated box and mesh (its vertex normals tilted and not unit: the lobe's
             0 / 0 weight), a sphere that moves while the shutter is open (the time a path carries); solid, checker and
             image albedos; no light: prob is 1 or NaN
  P-mix      P-lambert's floor, a sphere and a box under a rect light that is the world's light (has_light;
             cornell_box's 130 x 105 light of 15 at 554 above a 555 room, scaled by 1 / 50 and lowered to 1.9): light draws
             from the sphere's lower half and the box's sides fall below the surface's horizon (prob = 0), most lobe
             draws miss the light

Every world comes in two copies.  "detector": enclosed by a sphere of radius 60 whose material is a DiffuseLight
over a 256 x 128 image of random texels, seen from inside: a scattered ray that leaves the subject ends on a texel
that identifies its direction to 1.4 degrees, and `emit` on a back face is exercised on every such path.  "sky": no
detector, the sky background: the background along the PRIMARY ray, the scattered ray's hit or miss.

`CASES[name]`: the (material, decision[, face or branch detail]) cases that must keep at least MIN_STEPS compared
steps in leg a of tests/test_path_host.py, so a world that silently stops exercising a case fails."""
import numpy as np

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N
from tests import first_hit_worlds as FW

SIZE = R.Size2i(93, 54)
ASPECT = 54.0 / 93.0
MIN_STEPS = 200
NAMES = ("P-glass", "P-metal", "P-lambert", "P-mix")
COPIES = ("detector", "sky")
DETECTOR_RADIUS = 60.0
DETECTOR_SHAPE = (128, 256)

CASES = {
    "P-glass": {("dielectric", "refract", "front"), ("dielectric", "reflect", "front"), ("dielectric", "tir", "front"),
                ("dielectric", "refract", "back"), ("dielectric", "reflect", "back"), ("dielectric", "tir", "back")},
    "P-metal": {("metal", "reflect"), ("metal", "absorbed")},
    "P-lambert": {("lambert", "lobe_branch"), ("lambert", "lobe_branch", "nan")},
    "P-mix": {("lambert", "light_branch"), ("lambert", "lobe_branch"), ("lambert", "light_branch", "below"),
              ("lambert", "lobe_branch", "unlit"), ("lambert", "lobe_branch", "lit")},
}
MAT_NAMES = {N.MAT_LAMBERT: "lambert", N.MAT_METAL: "metal", N.MAT_DIELECTRIC: "dielectric",
             N.MAT_DIFFUSE_LIGHT: "light"}


def detector_image():
    return np.random.default_rng(25).integers(0, 256, DETECTOR_SHAPE + (3,), dtype=np.uint8)


def _tilted_sheet(origin, du, dv, nu, nv, rng, scale=(1.0, 1.0)):
    """A flat sheet of 2 nu nv triangles, (n, 24) f32 records: every vertex normal is the face normal tilted by
    20-30 degrees about a random axis in the sheet's plane, its length drawn from `scale`."""
    o, du, dv = (np.asarray(v, np.float64) for v in (origin, du, dv))
    up = np.cross(du, dv)
    up /= np.linalg.norm(up)
    e0 = du / np.linalg.norm(du)
    e1 = np.cross(up, e0)
    verts = {}
    for j in range(nv + 1):
        for i in range(nu + 1):
            s, t = i / nu, j / nv
            tilt, phi = np.radians(rng.uniform(20.0, 30.0)), rng.uniform(0.0, 2.0 * np.pi)
            n = np.cos(tilt) * up + np.sin(tilt) * (np.cos(phi) * e0 + np.sin(phi) * e1)
            verts[i, j] = (o + s * du + t * dv, n * rng.uniform(*scale), (0.05 + 0.9 * s, 0.05 + 0.9 * t))
    tris = []
    for j in range(nv):
        for i in range(nu):
            for corners in (((i, j), (i + 1, j), (i + 1, j + 1)), ((i, j), (i + 1, j + 1), (i, j + 1))):
                ps, ns, uvs = zip(*(verts[c] for c in corners))
                tris.append([x for p in ps for x in p] + [x for n in ns for x in n] + [x for uv in uvs for x in uv])
    return np.asarray(tris, np.float32)


def _camera(position, target, fov, time=None):
    cam = R.Camera.build().vertical_fov(fov, ASPECT).position(position).look_at_focus((0, 1, 0), target)
    if time is not None:
        cam = cam.motion_blur(*time)
    return cam.build()


def _finish(wb, g, copy, cam):
    if copy == "detector":
        tex = wb.texture_image_rgb8(detector_image())
        light = R.world._ok(N.lib().rtw_material_diffuse_light(wb._b, tex))
        g.add(wb.new_obj_sphere(DETECTOR_RADIUS, light))
        return g.build().finish(wb, R.BackgroundColor.solid((0.0, 0.0, 0.0)), cam)
    assert copy == "sky"
    return g.build().finish(wb, R.BackgroundColor.sky(), cam)


def p_glass(copy):
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(wb.new_obj_sphere(1.1, wb.material_dielectric(1.5)).translate((-2.3, 1.2, 0.2)))
    g.add(wb.new_obj_box(1.7, 1.7, 1.7, wb.material_dielectric(1.5)).rotate_around_up(25.0).translate((-0.9, 0.1, -0.4)))
    g.add(wb.new_obj_sphere(1.1, wb.material_dielectric(0.8)).translate((2.4, 1.2, 0.3)))
    g.add(wb.new_obj_sphere(1.15, wb.material_dielectric(2.4)).translate((1.0, 3.1, 0.6)))  # r0 = 0.17: the coin's heads
    return _finish(wb, g, copy, _camera((0.3, 2.6, 6.0), (0.0, 1.5, 0.0), 50.0))


def p_metal(copy):
    rng = np.random.default_rng(26)
    wb = R.WorldBuilder()
    g = wb.new_group()
    for k, fuzz in enumerate((0.0, 0.3, 1.0)):
        g.add(wb.new_obj_sphere(0.85, wb.material_metal_solid((0.9, 0.7 - 0.1 * k, 0.5 + 0.2 * k), fuzz))
              .translate((-2.6 + 2.0 * k, 0.9, 0.4)))
    g.add(wb.new_mesh(_tilted_sheet((1.9, 0.2, -0.2), (1.6, 0.0, 0.5), (-0.1, 1.9, -0.3), 2, 2, rng),
                      wb.material_metal_solid((0.8, 0.8, 0.9), 0.3)))
    g.add(wb.new_obj_rect_xz((0.0, 0.0, 0.0), 9.0, 7.0, wb.material_metal_solid((0.7, 0.8, 0.7), 0.6)))   # back face
    g.add(wb.new_obj_rect_xz((0.0, 3.3, -0.5), 8.0, 4.0, wb.material_metal_solid((0.9, 0.9, 0.6), 0.0)))  # front face
    return _finish(wb, g, copy, _camera((0.3, 1.9, 6.0), (0.0, 1.3, 0.0), 58.0))


def _floor(wb):
    checker = wb.texture_checker(2.0, wb.texture_solid((0.2, 0.3, 0.1)), wb.texture_solid((0.9, 0.9, 0.8)))
    return wb.new_obj_rect_xz((0.0, -0.37, 0.0), 9.0, 7.0, wb.material_lambert(checker))  # (a checker is 0 on y = 0)


def p_lambert(copy):
    rng = np.random.default_rng(27)
    wb = R.WorldBuilder()
    image = wb.material_lambert(wb.texture_image_rgb8(FW._image(5)))
    g = wb.new_group()
    g.add(_floor(wb))
    g.add(wb.new_obj_sphere(0.9, image).translate((-2.5, 0.9, 0.3)))
    g.add(wb.new_obj_box(1.3, 1.3, 1.3, wb.material_lambert_solid((0.7, 0.3, 0.2))).rotate_around_up(-20.0)
          .translate((-0.9, 0.0, 0.6)))
    g.add(wb.new_mesh(_tilted_sheet((0.8, 0.0, -0.3), (2.6, 0.0, 0.7), (-0.1, 2.7, -0.5), 3, 2, rng, (0.5, 0.8)),
                      wb.material_lambert(wb.texture_image_rgb8(FW._image(6)))))
    g.add(wb.new_obj_sphere(0.5, wb.material_lambert_solid((0.2, 0.5, 0.9))).translate((-0.6, 2.3, 0.0))
          .animate_moving((1.2, 0.0, 0.3)))
    return _finish(wb, g, copy, _camera((0.3, 2.0, 6.0), (0.0, 1.2, 0.0), 58.0, time=(0.25, 1.0)))


def p_mix(copy):
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(_floor(wb))
    g.add(wb.new_obj_sphere(0.9, wb.material_lambert_solid((0.7, 0.6, 0.5))).translate((-1.5, 0.9, 0.2)))
    g.add(wb.new_obj_box(1.2, 1.6, 1.2, wb.material_lambert(wb.texture_image_rgb8(FW._image(7)))).rotate_around_up(20.0)
          .translate((0.9, 0.0, -0.2)))
    g.add(wb.new_obj_rect_xz((0.2, 1.9, 0.1), 2.6, 2.1, wb.material_diffuse_light_solid((15.0, 15.0, 15.0)))
          .set_all_geo_as_poi())
    return _finish(wb, g, copy, _camera((0.3, 2.1, 6.0), (0.0, 1.0, 0.0), 55.0))


_BUILD = {"P-glass": p_glass, "P-metal": p_metal, "P-lambert": p_lambert, "P-mix": p_mix}
_cache = {}


def world(name, copy):
    """The world `name` of NAMES in the copy `copy` of COPIES (cached)."""
    if (name, copy) not in _cache:
        _cache[name, copy] = _BUILD[name](copy)
    return _cache[name, copy]


def case_counts(res, raw):
    """{case: compared steps} of a step() result: (material, decision) for every live hit, a dielectric's with its
    face, and the Lambert details: "nan" (prob is NaN), "below" (a light draw with prob 0), "lit" / "unlit" (a lobe
    draw that light_value does or does not see: prob below 2 or exactly 2)."""
    out = {}

    def add(key, mask):
        out[key] = out.get(key, 0) + int(mask.sum())

    m = res["compared"] & res["hit"] & (res["end"] != 2)
    for kind, mname in MAT_NAMES.items():
        mk = m & (res["mat_kind"] == kind)
        for dec in np.unique(res["decision"][mk]):
            md = mk & (res["decision"] == dec)
            if kind == N.MAT_DIELECTRIC:
                add((mname, str(dec), "front"), md & res["front_face"])
                add((mname, str(dec), "back"), md & ~res["front_face"])
            else:
                add((mname, str(dec)), md)
        if kind == N.MAT_LAMBERT:
            lobe, light = mk & (res["decision"] == "lobe_branch"), mk & (res["decision"] == "light_branch")
            add((mname, "lobe_branch", "nan"), lobe & np.isnan(res["prob"]))
            add((mname, "light_branch", "below"), light & (res["prob"] == 0))
            if raw.has_light:
                add((mname, "lobe_branch", "unlit"), lobe & (res["prob"] == 2.0))
                add((mname, "lobe_branch", "lit"), lobe & (res["prob"] > 0) & (res["prob"] < 2.0))
    return out
