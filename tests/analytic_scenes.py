"""Scenes in which the estimator's per-pixel expectation is a closed-form number (plain helpers, no fixtures;
tests/test_analytic_host.py renders them with the oracle, tests/test_gpu_analytic.py with the kernels).

Every scene function returns (world, (W, H), expect).  expect(world, W, H, n=12) gives, in numpy f64 only and
from the fields of the built camera and the built primitives in world.raw (never from the numbers passed to the
builder, never through the oracle, librtw's arithmetic or rtw_scalar.h), an `Expectation`:

  scale   the one non-zero value a sample can take, per channel (dyadic: f32 sums of up to 4096 samples are exact)
  mean    (H, W) per-pixel expectation of sample / scale
  var     (H, W) per-pixel single-sample variance of sample / scale, or None where it is not closed-form (S2m)

In every scene but S1 and S2m a sample is scale * X with X Bernoulli(P(px, py)) for a closed-form P of the film
point; sample s of pixel (x, y) takes px = x/(W-1) + U[0, 1/(W-1)), py = y/(H-1) + U[0, 1/(H-1)), so the pixel's X
is Bernoulli(mean) with mean the average of P over the jitter square (an n x n midpoint rule) and var = mean (1 - mean).

What of the algorithm goes into P (oracle/rtw_oracle.c, camera_ray / ray_color / rect_hit):
  * upper_left_corner is relative to the camera position: direction = unit(ulc + scaled_right px - scaled_up py
    - lens_offset), origin = position + lens_offset;
  * an escaping ray takes the background of the primary ray: every scene here has a solid background;
  * a rect's front face is the side its -axis normal faces."""
from dataclasses import dataclass

import numpy as np

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N

MAX_DEPTH = 8
TWO_PI = 2.0 * np.pi


@dataclass
class Expectation:
    scale: np.ndarray  # (3,) f64
    mean: np.ndarray  # (H, W) f64
    var: np.ndarray | None  # (H, W) f64


# ------------------------------------------------------------------------------------------------
# the built world, read back in f64
# ------------------------------------------------------------------------------------------------
def _f64(v) -> np.ndarray:
    return np.array(list(v), np.float64)


class _Cam:
    def __init__(self, world):
        c = world.raw.camera
        self.position, self.ulc = _f64(c.position), _f64(c.upper_left_corner)
        self.unit_right, self.unit_up = _f64(c.unit_right), _f64(c.unit_up)
        self.scaled_right, self.scaled_up = _f64(c.scaled_right), _f64(c.scaled_up)
        self.lens_radius = float(c.lens_radius)
        assert c.time0 == c.time1

    def film(self, px, py):
        """ulc + scaled_right px - scaled_up py, three components that broadcast over (px, py) (a component that
        does not depend on px or py keeps the smaller shape: the closed forms cost less)."""
        out = []
        for k in range(3):
            c = self.ulc[k]
            if self.scaled_right[k] != 0.0:
                c = c + self.scaled_right[k] * px
            if self.scaled_up[k] != 0.0:
                c = c - self.scaled_up[k] * py
            out.append(c)
        return out


def _material_color(world, material: int) -> np.ndarray:
    m = world.raw.materials[material]
    t = world.raw.textures[m.texture]
    assert t.kind == N.TEX_SOLID
    return _f64(t.color)


def _leaves_of(world, geom_kind: int, mat_kind: int):
    """The leaves of this geometry and material kind."""
    raw, out = world.raw, []
    for i in range(raw.leaf_count):
        leaf = raw.leaves[i]
        if leaf.geom_kind == geom_kind and raw.materials[leaf.material].kind == mat_kind:
            out.append(leaf)
    return out


def _only(leaves):
    assert len(leaves) == 1, len(leaves)
    return leaves[0]


def _background(world) -> np.ndarray:
    assert world.raw.background.kind == N.BG_SOLID
    return _f64(world.raw.background.color)


_RECT_AXES = {N.PLANE_XY: (0, 1, 2), N.PLANE_XZ: (0, 2, 1), N.PLANE_YZ: (1, 2, 0)}


def _rect(world, leaf):
    assert leaf.flags == 0
    g = world.raw.rects[leaf.geom_index]
    return _RECT_AXES[g.plane], float(g.dist), _f64(g.r0), _f64(g.r1)


# ------------------------------------------------------------------------------------------------
# the jitter square's midpoint rule
# ------------------------------------------------------------------------------------------------
def pixel_mean(prob, W: int, H: int, n: int, rows: int = 8) -> np.ndarray:
    """(H, W) averages of prob(px, py) over each pixel's jitter square, n x n midpoints.  prob takes px of shape
    (1, W n) and py of shape (r n, 1) and returns a shape that broadcasts to (r n, W n).  Bands of rows go to a few
    threads (numpy's loops run outside the interpreter lock)."""
    import os
    from concurrent.futures import ThreadPoolExecutor

    mid = (np.arange(n, dtype=np.float64) + 0.5) / n
    px = ((np.arange(W, dtype=np.float64)[:, None] + mid[None, :]) / (W - 1)).reshape(1, W * n)
    out = np.empty((H, W), np.float64)

    def band(y0):
        y1 = min(H, y0 + rows)
        py = ((np.arange(y0, y1, dtype=np.float64)[:, None] + mid[None, :]) / (H - 1)).reshape((y1 - y0) * n, 1)
        p = np.broadcast_to(prob(px, py), (py.shape[0], px.shape[1]))
        out[y0:y1] = p.reshape(y1 - y0, n, W, n).mean(axis=(1, 3))

    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        cpus = os.cpu_count() or 1
    with ThreadPoolExecutor(max(1, min(cpus, 8))) as pool:
        list(pool.map(band, range(0, H, rows)))
    return out


def _bernoulli(scale, mean) -> Expectation:
    return Expectation(np.asarray(scale, np.float64), mean, mean * (1.0 - mean))


def _finish(wb, group, background, camera):
    return group.build().finish(wb, R.BackgroundColor.solid(background), camera)


# ------------------------------------------------------------------------------------------------
# S1, the weight: spdf / p has identical operands
# ------------------------------------------------------------------------------------------------
def s1_weight(W: int = 64, H: int = 64):
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(wb.new_obj_sphere(1.0, wb.material_lambert_solid((0.25, 0.5, 0.75))))
    cam = R.Camera.build().vertical_fov(6.0, 1.0).position((0.0, 0.0, 8.0)).look_at((0, 1, 0), (0, 0, 0)).build()
    return _finish(wb, g, (1.0, 2.0, 0.5), cam), (W, H), expect_s1


def expect_s1(world, W: int, H: int, n: int = 12) -> Expectation:
    """Every sample is albedo * background, but for the trap below: mean 1, variance 0 (of sample / scale).  The
    view must lie inside the sphere's silhouette: checked at the film's corners."""
    cam = _Cam(world)
    leaf = _only(_leaves_of(world, N.GEOM_SPHERE, N.MAT_LAMBERT))
    s = world.raw.spheres[leaf.geom_index]
    oc = _f64(s.center) - cam.position
    for px in (0.0, 1.0 + 1.0 / (W - 1)):
        for py in (0.0, 1.0 + 1.0 / (H - 1)):
            d = np.array(cam.film(px, py))
            d /= np.linalg.norm(d)
            assert oc @ oc - (oc @ d) ** 2 < 0.5 * s.radius**2
    scale = _material_color(world, leaf.material) * _background(world)
    return Expectation(scale, np.ones((H, W)), np.zeros((H, W)))


def s1_trap_probability(world) -> float:
    """A worst-case bound on the probability that an S1 sample is 0 instead of albedo * background.

    The algorithm as written (the reference's sphere hit, sphere_geometry.rs:21-54, and the 0.001 start of every
    ray) traps a sample when f32 rounding puts the camera ray's hit point a depth delta inside the sphere and the
    bounce grazes: from there the far root, about sqrt(c^2 + 2 delta) - c for the bounce's cosine c to the normal,
    exceeds 0.001, the bounce hits the sphere from inside, and every later bounce stays inside until the depth runs
    out: the sample is 0.  That needs c < (2 delta - 1e-6) / 0.002.  With u = 2^-24, D the camera's distance and
    the film inside half the squared radius (expect_s1): the discriminant half_b^2 - c, two numbers near D^2, is
    off by at most 12 u D^2, its root (>= r sqrt(1/2)) by that / (2 r sqrt(1/2)), t by 2 u D more and the hit
    point by 3 u D more: delta below their sum.  The lobe has cos^2 uniform: P(cos < c) = c^2."""
    cam = _Cam(world)
    s = world.raw.spheres[_only(_leaves_of(world, N.GEOM_SPHERE, N.MAT_LAMBERT)).geom_index]
    u, D, r = 2.0**-24, float(np.linalg.norm(_f64(s.center) - cam.position)), float(s.radius)
    delta = 12 * u * D * D / (2 * r * np.sqrt(0.5)) + 5 * u * D
    c = max((2 * delta - 1e-6) / 0.002, 0.0) / r
    return min(c * c, 1.0)


def assert_s1(image: np.ndarray, world, W: int, H: int, spp: int) -> int:
    """Every pixel is bit for bit f32(albedo background), or holds j trapped samples and is exactly (spp - j) / spp
    of it; no NaN; the trapped samples within s1_trap_probability.  Returns their number."""
    e = expect_s1(world, W, H)
    img = np.asarray(image, np.float32).reshape(H * W, 3)
    assert not np.isnan(img).any(), f"{int(np.isnan(img).any(axis=1).sum())} NaN pixels"
    want = np.ascontiguousarray(np.broadcast_to(e.scale.astype(np.float32), img.shape))
    assert (want.astype(np.float64) == e.scale).all()
    whole = (img.view(np.uint32) == want.view(np.uint32)).all(axis=1)
    k = img[~whole].astype(np.float64) / e.scale * spp  # (bad, 3)
    assert (k == np.round(k)).all() and (k >= 0).all() and (k < spp).all() and (k == k[:, :1]).all(), k
    trapped = int((spp - k[:, 0]).sum())
    bound = s1_trap_probability(world) * W * H * spp
    assert trapped <= bound + 5.0 * np.sqrt(bound), (trapped, bound)
    return trapped


# ------------------------------------------------------------------------------------------------
# S2 / S2m, the cosine lobe and the light mixture: the form factor of a parallel rectangle
# ------------------------------------------------------------------------------------------------
def _lobe_world(poi: bool):
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(wb.new_obj_rect_xz((0.0, 0.0, 0.0), 40.0, 40.0, wb.material_lambert_solid((1.0, 0.5, 0.25))))
    light = wb.new_obj_rect_xz((0.3, 1.0, -0.2), 1.5, 1.0, wb.material_diffuse_light_solid((1.0, 2.0, 4.0)))
    if poi:
        light.set_all_geo_as_poi()
    g.add(light)
    cam = R.Camera.build().vertical_fov(40.0, 1.0).position((0.2, 0.5, 0.1)).look_at((0, 0, 1), (0.2, 0.0, 0.1)).build()
    return _finish(wb, g, (0.0, 0.0, 0.0), cam)


def s2_cosine_lobe(W: int = 48, H: int = 48):
    world = _lobe_world(False)
    assert world.raw.has_light == 0
    return world, (W, H), expect_s2


def s2m_light_mixture(W: int = 48, H: int = 48):
    world = _lobe_world(True)
    assert world.raw.has_light == 1
    return world, (W, H), expect_s2m


def _corner_form_factor(a, b, h):
    """The form factor from a surface point to a parallel a x b rectangle at height h with one corner over the
    point; odd in a and in b."""
    ra, rb = np.sqrt(a * a + h * h), np.sqrt(b * b + h * h)
    return (a / ra * np.arctan(b / ra) + b / rb * np.arctan(a / rb)) / TWO_PI


_LOBE_MEANS = {}  # S2 and S2m share camera, floor and light: one quadrature serves both


def _lobe_mean(world, W, H, n):
    raw = world.raw
    key = (bytes(raw.camera), tuple(bytes(raw.rects[i]) for i in range(raw.rect_count)), W, H, n)
    if key not in _LOBE_MEANS:
        _LOBE_MEANS[key] = _lobe_mean_uncached(world, W, H, n)
    return _LOBE_MEANS[key]


def _lobe_mean_uncached(world, W, H, n):
    cam = _Cam(world)
    (fa0, fa1, fn), fdist, fr0, fr1 = _rect(world, _only(_leaves_of(world, N.GEOM_RECT, N.MAT_LAMBERT)))
    (la0, la1, ln), ldist, lr0, lr1 = _rect(world, _only(_leaves_of(world, N.GEOM_RECT, N.MAT_DIFFUSE_LIGHT)))
    assert (fa0, fa1, fn) == (la0, la1, ln)
    h = ldist - fdist
    assert h > 0 and (cam.position[fn] - fdist) * (cam.position[fn] - ldist) < 0  # the camera between the two

    def prob(px, py):
        d = cam.film(px, py)
        t = (fdist - cam.position[fn]) / d[fn]
        u, v = cam.position[fa0] + t * d[fa0], cam.position[fa1] + t * d[fa1]
        assert np.all(t > 0) and np.all(u > fr0[0]) and np.all(u < fr0[1]) and np.all(v > fr1[0]) and np.all(v < fr1[1])
        a0, a1, b0, b1 = lr0[0] - u, lr0[1] - u, lr1[0] - v, lr1[1] - v
        return (_corner_form_factor(a1, b1, h) - _corner_form_factor(a0, b1, h)
                - _corner_form_factor(a1, b0, h) + _corner_form_factor(a0, b0, h))

    return pixel_mean(prob, W, H, n)


def _lobe_scale(world):
    floor = _only(_leaves_of(world, N.GEOM_RECT, N.MAT_LAMBERT))
    light = _only(_leaves_of(world, N.GEOM_RECT, N.MAT_DIFFUSE_LIGHT))
    return _material_color(world, floor.material) * _material_color(world, light.material)


def expect_s2(world, W: int, H: int, n: int = 12) -> Expectation:
    """albedo Le F(p): the bounce, drawn with the cosine density and weight exactly 1, finds the light with the
    probability F of the form factor."""
    return _bernoulli(_lobe_scale(world), _lobe_mean(world, W, H, n))


def expect_s2m(world, W: int, H: int, n: int = 12) -> Expectation:
    """The same expectation under the light mixture (the weight spdf / p is no longer 1: no closed-form variance)."""
    return Expectation(_lobe_scale(world), _lobe_mean(world, W, H, n), None)


# ------------------------------------------------------------------------------------------------
# S3, the metal fuzz ball
# ------------------------------------------------------------------------------------------------
def s3_fuzz_ball(W: int = 48, H: int = 48):
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(wb.new_obj_rect_xz((0.0, 0.0, 0.0), 400.0, 400.0, wb.material_metal_solid((0.5, 1.0, 0.25), 1.0)))
    cam = R.Camera.build().vertical_fov(10.0, 1.0).position((0.0, 0.3, 0.0)).look_at((0, 1, 0), (1.0, 0.0, 0.0)).build()
    return _finish(wb, g, (1.0, 0.5, 2.0), cam), (W, H), expect_s3


def _plane_cosine(cam, rect, px, py):
    """The incidence cosine of the primary ray on the rect's plane; asserts that every ray lands inside the rect."""
    (a0, a1, nn), dist, r0, r1 = rect
    d = cam.film(px, py)
    t = (dist - cam.position[nn]) / d[nn]
    u, v = cam.position[a0] + t * d[a0], cam.position[a1] + t * d[a1]
    assert np.all(t > 0) and np.all(u > r0[0]) and np.all(u < r0[1]) and np.all(v > r1[0]) and np.all(v < r1[1])
    return np.abs(d[nn]) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), d[nn]


def expect_s3(world, W: int, H: int, n: int = 12) -> Expectation:
    """albedo B (1 - absorbed): the bounce mirror + fuzz ball is absorbed when the ball's normal component is
    <= -c / fuzz, which a uniform ball does with probability (2 - 3 u + u^3) / 4, u = min(c / fuzz, 1)."""
    cam = _Cam(world)
    leaf = _only(_leaves_of(world, N.GEOM_RECT, N.MAT_METAL))
    rect = _rect(world, leaf)
    fuzz = float(world.raw.materials[leaf.material].fuzz)
    assert fuzz > 0

    def prob(px, py):
        c, _ = _plane_cosine(cam, rect, px, py)
        u = np.minimum(c / fuzz, 1.0)
        return 1.0 - (2.0 - 3.0 * u + u**3) / 4.0

    return _bernoulli(_material_color(world, leaf.material) * _background(world), pixel_mean(prob, W, H, n))


# ------------------------------------------------------------------------------------------------
# S4, the free path
# ------------------------------------------------------------------------------------------------
def s4_free_path(W: int = 48, H: int = 48):
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(wb.new_obj_sphere(1.0, wb.material_isotropic_solid((0.0, 0.0, 0.0))).set_all_geo_densitity(0.8))
    cam = R.Camera.build().vertical_fov(12.0, 1.0).position((0.0, 0.0, 8.0)).look_at((0, 1, 0), (0, 0, 0)).build()
    return _finish(wb, g, (1.0, 0.5, 2.0), cam), (W, H), expect_s4


def expect_s4(world, W: int, H: int, n: int = 12) -> Expectation:
    """B exp(-density L), L the primary ray's chord (0 where it misses): a black medium ends the path at 0."""
    cam = _Cam(world)
    leaf = _only(_leaves_of(world, N.GEOM_SPHERE, N.MAT_ISOTROPIC))
    assert leaf.flags == N.LEAF_VOLUME
    assert not _material_color(world, leaf.material).any()
    s = world.raw.spheres[leaf.geom_index]
    oc = _f64(s.center) - cam.position
    density = -1.0 / float(leaf.neg_inv_density)
    r2 = float(s.radius) ** 2
    assert oc @ oc > r2  # the camera outside

    def prob(px, py):
        d = cam.film(px, py)
        dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        along = (oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2]) / np.sqrt(dd)
        chord = 2.0 * np.sqrt(np.maximum(r2 - (oc @ oc - along * along), 0.0))
        return np.exp(-density * chord)

    return _bernoulli(_background(world), pixel_mean(prob, W, H, n))


# ------------------------------------------------------------------------------------------------
# S5, the Schlick coin
# ------------------------------------------------------------------------------------------------
def s5_schlick_coin(W: int = 48, H: int = 48):
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(wb.new_obj_rect_xz((0.0, 0.0, 0.0), 400.0, 400.0, wb.material_dielectric(1.5)))
    g.add(wb.new_obj_rect_xz((0.0, 1.0, 0.0), 4000.0, 4000.0, wb.material_diffuse_light_solid((0.0, 0.0, 0.0))))
    cam = R.Camera.build().vertical_fov(30.0, 1.0).position((0.0, -0.3, 0.0)).look_at((0, 1, 0), (1.0, 0.0, 0.0)).build()
    return _finish(wb, g, (1.0, 0.5, 2.0), cam), (W, H), expect_s5


def expect_s5(world, W: int, H: int, n: int = 12) -> Expectation:
    """B [r0 + (1 - r0)(1 - c)^5]: the reflected ray escapes to the background, the refracted one ends on the
    black absorber behind the pane.  ratio = 1 / ior on the front face (the side the -axis normal faces), ior on
    the other, where it reflects totally once ratio sin > 1."""
    cam = _Cam(world)
    leaf = _only(_leaves_of(world, N.GEOM_RECT, N.MAT_DIELECTRIC))
    rect = _rect(world, leaf)
    ior = float(world.raw.materials[leaf.material].index_of_refraction)
    absorber = _only(_leaves_of(world, N.GEOM_RECT, N.MAT_DIFFUSE_LIGHT))
    assert not _material_color(world, absorber.material).any()
    # the absorber behind the pane as seen from the camera
    assert (_rect(world, absorber)[1] - rect[1]) * (cam.position[rect[0][2]] - rect[1]) < 0

    def prob(px, py):
        c, dn = _plane_cosine(cam, rect, px, py)
        ratio = np.where(dn > 0, 1.0 / ior, ior)  # dot(-axis, d) < 0: front face
        r0 = ((1.0 - ratio) / (1.0 + ratio)) ** 2
        total = ratio * np.sqrt(1.0 - c * c) > 1.0
        return np.where(total, 1.0, r0 + (1.0 - r0) * (1.0 - c) ** 5)

    return _bernoulli(_background(world), pixel_mean(prob, W, H, n))


# ------------------------------------------------------------------------------------------------
# S6, the lens disc
# ------------------------------------------------------------------------------------------------
def s6_lens_disc(W: int = 48, H: int = 48):
    wb = R.WorldBuilder()
    g = wb.new_group()
    g.add(wb.new_obj_rect_xy((-500.0, 0.0, -3.0), 1000.0, 1000.0, wb.material_diffuse_light_solid((1.0, 0.5, 2.0))))
    cam = (R.Camera.build().vertical_fov(20.0, 1.0).position((0.0, 0.0, 0.0)).look_at((0, 1, 0), (0.0, 0.0, -1.0))
           .aperture(0.4).focus_distance(1.5).build())
    return _finish(wb, g, (0.0, 0.0, 0.0), cam), (W, H), expect_s6


def _disc_cdf(x):
    """P(d0 <= x) of the first coordinate of a uniform point of the unit disc."""
    x = np.clip(x, -1.0, 1.0)
    return 0.5 + (x * np.sqrt(1.0 - x * x) + np.arcsin(x)) / np.pi


def s6_column_edges(world, W: int):
    """(W,) the least and greatest disc abscissa x0 at which a column's samples change from dark to lit, over the
    column's jitter interval: a column with both beyond +-1 is all lit or all dark."""
    cam = _Cam(world)
    px = (np.arange(W, dtype=np.float64)[:, None] + np.array([0.0, 1.0])[None, :]) / (W - 1)
    x0 = _s6_threshold(world, cam, px)
    return x0.min(axis=1), x0.max(axis=1)


def _s6_geometry(world, cam):
    leaf = _only(_leaves_of(world, N.GEOM_RECT, N.MAT_DIFFUSE_LIGHT))
    (a0, a1, nn), dist, r0, r1 = _rect(world, leaf)
    assert (a0, a1, nn) == (0, 1, 2) and cam.lens_radius > 0
    # the lens lies in the plane of the light's axes and its first coordinate runs along x
    assert cam.unit_right[2] == 0 and cam.unit_up[2] == 0 and cam.unit_up[0] == 0 and cam.unit_right[1] == 0
    assert cam.ulc[1] != 0 and cam.scaled_right[2] == 0 and cam.scaled_up[2] == 0
    return leaf, dist, r0, r1


def _s6_threshold(world, cam, px):
    """The sample with disc point (d0, d1) and film abscissa px lands at x = (1 - s) lens_radius right_x d0 + s Pf.x
    on the light's plane, s = (dist - position.z) / ulc.z; it is lit when x < edge, the light's upper x bound
    (its other bounds are out of reach): d0 > x0 for (1 - s) right_x < 0."""
    _, dist, r0, r1 = _s6_geometry(world, cam)
    s = (dist - cam.position[2]) / cam.ulc[2]
    k = (1.0 - s) * cam.lens_radius * cam.unit_right[0]
    assert s > 1 and k < 0
    pfx = cam.ulc[0] + cam.scaled_right[0] * px
    reach = abs(k) + s * (abs(cam.ulc[0]) + abs(cam.scaled_right[0]) * 1.1) + abs(cam.position[0])
    reach_y = abs(k) + s * (abs(cam.ulc[1]) + abs(cam.scaled_up[1]) * 1.1) + abs(cam.position[1])
    assert r0[0] < -reach and r1[0] < -reach_y and r1[1] > reach_y
    return (r0[1] - cam.position[0] - s * pfx) / k


def expect_s6(world, W: int, H: int, n: int = 12) -> Expectation:
    """emit P(d0 > x0): d0, the lens disc's first coordinate, has the CDF 1/2 + (x sqrt(1 - x^2) + asin x) / pi."""
    cam = _Cam(world)
    leaf, *_ = _s6_geometry(world, cam)

    def prob(px, py):
        return 1.0 - _disc_cdf(_s6_threshold(world, cam, px))

    return _bernoulli(_material_color(world, leaf.material), pixel_mean(prob, W, H, n))


# ------------------------------------------------------------------------------------------------
# the statistics the tests assert
# ------------------------------------------------------------------------------------------------
SCENES = {"S1": s1_weight, "S2": s2_cosine_lobe, "S2m": s2m_light_mixture, "S3": s3_fuzz_ball, "S4": s4_free_path,
          "S5": s5_schlick_coin, "S6": s6_lens_disc}
BERNOULLI = ("S2", "S3", "S4", "S5", "S6")
LOBE = ("S2", "S2m")  # a Lambertian bounce: see normalised_lobe
Z_BOUND = 5.0  # a false-alarm rate of about 1e-5 over some twenty assertions with fixed seeds: a choice, not a measurement
QUADRATURE_MARGIN = 0.25  # of sigma


LOBE_NAN_PROBABILITY = 2.0**-24


def normalised(image: np.ndarray, e: Expectation, W: int, H: int) -> np.ndarray:
    """(H, W, 3) f64 image / scale; no pixel may be NaN and none is left out."""
    img = np.asarray(image, np.float32).reshape(H, W, 3)
    assert not np.isnan(img).any(), f"{int(np.isnan(img).any(axis=2).sum())} NaN pixels"
    return img.astype(np.float64) / e.scale


def normalised_lobe(image: np.ndarray, e: Expectation, world, W: int, H: int, spp: int, seed: int):
    """`normalised` for a scene that bounces off a Lambertian (S2, S2m), where the algorithm as written makes a NaN
    sample of its own: (x (pixels, 3), the expectation over the same pixels, the number of NaN pixels).

    The lobe is unit(n + s) with s = UnitSphere's (x1 f, x2 f, 1 - 2 sum), f = 2 sqrt(1 - sum).  Where the
    coordinate of s along n rounds to -1 exactly (a uniform coordinate within about 2^-25 of -1; the product and
    the root add a rounding each: probability below LOBE_NAN_PROBABILITY = 2^-24 a draw) while the rest of s stays
    above unit_or_else's 1e-8, the direction has cosine exactly 0, spdf = p = 0 and the weight spdf / p is 0 / 0:
    the sample is NaN, and so is its pixel (the reference's 0/0 pdf quirk, material.rs:17-40 + rendering.rs:73-92).
    So a NaN pixel is admitted only if (1) the NaN pixels number within that probability's 5 sigma, and (2) the
    oracle's replay of that pixel's samples, two levels deep, shows a NaN sample of the first bounce; it then leaves
    the statistic together with its expectation and variance (one grazing draw in spp: no bias to speak of)."""
    from oracle import pyoracle as O

    img = np.asarray(image, np.float32).reshape(H * W, 3)
    nan = np.isnan(img).any(axis=1)
    bound = LOBE_NAN_PROBABILITY * W * H * spp
    assert nan.sum() <= bound + 5.0 * np.sqrt(bound), (int(nan.sum()), bound)
    p2 = R.render_params(R.Size2i(W, H), spp, 2, seed=seed)
    for pix in np.flatnonzero(nan):
        col = np.array([O.sample_color(world, p2, int(pix % W), int(pix // W), s) for s in range(spp)])
        assert np.isnan(col).any(), f"pixel {pix} is NaN but none of the oracle's first bounces is"
    keep = ~nan
    var = None if e.var is None else e.var.reshape(-1)[keep]
    return img[keep].astype(np.float64) / e.scale, Expectation(e.scale, e.mean.reshape(-1)[keep], var), int(nan.sum())


def bernoulli_channel(x: np.ndarray) -> np.ndarray:
    """(H, W) channel 0 of a Bernoulli scene's normalised image: the fraction of the pixel's samples that took the
    value `scale`, every channel within [0, 1].  (Not asserted to be a whole number of samples: about one bounce in
    10^7 leaves a hit point that f32 rounding put below a rect's plane so flat that it meets the rect again, and
    that sample takes the dyadic value albedo^2 ...; the sums stay exact and the mean moves by 1e-7.)"""
    assert (x >= 0.0).all() and (x <= 1.0).all()
    return x[..., 0]


def mean_z(x: np.ndarray, e: Expectation, spp: int, sigma: float | None = None) -> dict:
    """The image mean of channel 0 against the expectation, in units of the standard error `sigma` of that mean
    (from the f64 variance unless given)."""
    m, E = float(x[..., 0].mean()), float(e.mean.mean())
    if sigma is None:
        sigma = float(np.sqrt(e.var.sum() / spp)) / e.mean.size
    return {"mean": m, "expect": E, "sigma": sigma, "z": (m - E) / sigma}


def expectation_with_margin(scene_expect, world, W, H, sigma_of, n: int = 12, n_max: int = 96):
    """The expectation at the least n (doubling from 12) whose n -> 2 n change of the image mean stays below
    QUADRATURE_MARGIN sigma; sigma_of(e) gives the standard error of the image mean.  Returns (e, n, shift, sigma)."""
    e = scene_expect(world, W, H, n)
    while True:
        e2 = scene_expect(world, W, H, 2 * n)
        shift, sigma = abs(float(e2.mean.mean()) - float(e.mean.mean())), sigma_of(e)
        if shift < QUADRATURE_MARGIN * sigma or 2 * n > n_max:
            return e, n, shift, sigma
        e, n = e2, 2 * n


def bernoulli_sigma(spp: int):
    return lambda e: float(np.sqrt(e.var.sum() / spp)) / e.mean.size


def dispersion(m: np.ndarray, e: Expectation, spp: int) -> tuple:
    """(chi^2, n, bound): sum (m_i - F_i)^2 / (F_i (1 - F_i) / spp) over the pixel means m_i against n = their
    number; it must lie within 5 sqrt(2 n) of n."""
    chi2 = float((((m - e.mean) ** 2) / (e.var / spp)).sum())
    return chi2, m.size, 5.0 * np.sqrt(2.0 * m.size)


# ------------------------------------------------------------------------------------------------
# the checks, for any renderer `render(world, W, H, spp, seed) -> (H*W, 3) f32`
# ------------------------------------------------------------------------------------------------
SEED = 0x5EED


def report(line: str) -> None:
    """Print the figures; the file named by RTW_ANALYTIC_REPORT, if any, collects them."""
    import os

    print(line)
    path = os.environ.get("RTW_ANALYTIC_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _report_z(where, name, w, h, spp, n, shift, z, nan=0):
    report(f"{where} {name} {w}x{h}x{spp} samples={w * h * spp} n={n} mean={z['mean']:.9f} expect={z['expect']:.9f} "
           f"sigma={z['sigma']:.3e} z={z['z']:+.3f} quadrature_shift={shift:.3e} ({shift / z['sigma']:.4f} sigma)"
           + (f" nan_pixels={nan}" if nan else ""))


def check_image_mean(render, name: str, w: int, h: int, spp: int, where: str) -> None:
    """|image mean - E| <= 5 sigma for a Bernoulli scene, sigma from the f64 variance, the quadrature's n -> 2 n
    change below a quarter of it."""
    world, (w, h), expect = SCENES[name](w, h)
    e, n, shift, sigma = expectation_with_margin(expect, world, w, h, bernoulli_sigma(spp))
    assert shift < QUADRATURE_MARGIN * sigma, (shift, sigma, n)
    img, nan = render(world, w, h, spp, SEED), 0
    if name in LOBE:
        x, e, nan = normalised_lobe(img, e, world, w, h, spp, SEED)
    else:
        x = normalised(img, e, w, h)
    bernoulli_channel(x)
    z = mean_z(x, e, spp)
    _report_z(where, name, w, h, spp, n, shift, z, nan)
    assert abs(z["z"]) <= Z_BOUND, z


def check_mixture_mean(render, w: int, h: int, spp: int, where: str) -> None:
    """S2m: the mean of K = 8 seeds against the expectation, sigma from the spread of the 8 image means; the f32
    sums are not exact here, so the worst-case accumulation bound spp 2^-24 (relative) joins the tolerance."""
    assert spp <= 1024
    world, (w, h), expect = s2m_light_mixture(w, h)
    e0 = expect(world, w, h, 12)
    means, nan = [], 0
    for k in range(8):
        x, ek, nk = normalised_lobe(render(world, w, h, spp, SEED + 1 + k), e0, world, w, h, spp, SEED + 1 + k)
        assert (x >= 0.0).all()
        # (a seed that lost a pixel is compared on the pixels it kept: its mean moves by that pixel's share)
        means.append(float(x[..., 0].mean()) - float(ek.mean.mean()) + float(e0.mean.mean()))
        nan += nk
    sigma = float(np.std(means, ddof=1) / np.sqrt(8.0))
    e, n, shift, _ = expectation_with_margin(expect, world, w, h, lambda _e: sigma)
    assert shift < QUADRATURE_MARGIN * sigma, (shift, sigma, n)
    z = {"mean": float(np.mean(means)), "expect": float(e.mean.mean()), "sigma": sigma}
    z["z"] = (z["mean"] - z["expect"]) / sigma
    _report_z(where, "S2m(8 seeds, samples each)", w, h, spp, n, shift, z, nan)
    assert abs(z["mean"] - z["expect"]) <= Z_BOUND * sigma + spp * 2.0**-24 * z["expect"], z


def check_lens_columns(render, w: int, h: int, spp: int, where: str) -> None:
    """S6 per column: exact where every sample of the column is lit or dark, within 5 sigma of the column's
    expectation elsewhere (its own n -> 2 n change below a quarter of the column's sigma)."""
    world, (w, h), expect = s6_lens_disc(w, h)
    n = 24
    e, e2 = expect(world, w, h, n), expect(world, w, h, 2 * n)
    x = normalised(render(world, w, h, spp, SEED), e, w, h)
    m = bernoulli_channel(x)
    lo, hi = s6_column_edges(world, w)
    eps = 1e-5  # f32 rounding of the film point and of the lens offset moves x0 by a few 1e-7
    dark, lit = lo > 1.0 + eps, hi < -1.0 - eps
    assert dark.any() and lit.any() and (~(dark | lit)).sum() >= w // 4
    assert (x[:, dark] == 0.0).all() and (x[:, lit] == 1.0).all()
    assert (e.mean[:, dark] == 0.0).all() and (e.mean[:, lit] == 1.0).all()
    col_mean, col_e = m.mean(axis=0), e.mean.mean(axis=0)
    col_sigma = np.sqrt(e.var.sum(axis=0) / spp) / h
    part = col_sigma > 0
    assert (np.abs(e2.mean.mean(axis=0) - col_e)[part] < QUADRATURE_MARGIN * col_sigma[part]).all()
    assert (col_mean[~part] == col_e[~part]).all()
    zc = (col_mean[part] - col_e[part]) / col_sigma[part]
    report(f"{where} S6 columns {w}x{h}x{spp}: {int(dark.sum())} dark and {int(lit.sum())} lit exact; "
           f"{int(part.sum())} partial, max |z| = {np.abs(zc).max():.3f}")
    assert np.abs(zc).max() <= Z_BOUND


def check_dispersion(render, w: int, h: int, spp: int, where: str) -> None:
    """S2 over the pixels: correlated samples within a pixel, or streams shared between pixels, inflate chi^2."""
    world, (w, h), expect = s2_cosine_lobe(w, h)
    e = expect(world, w, h)
    x, e, _ = normalised_lobe(render(world, w, h, spp, SEED), e, world, w, h, spp, SEED)
    chi2, n, bound = dispersion(bernoulli_channel(x), e, spp)
    report(f"{where} S2 dispersion over pixels {w}x{h}x{spp}: chi2={chi2:.1f} n={n} bound=+-{bound:.1f}")
    assert abs(chi2 - n) <= bound
