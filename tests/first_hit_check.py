"""What the first-hit tests share: the camera rays of a frame (the oracle's (seed, pixel, sample) stream and
Camera::ray, as tests/aov_ref.primary_hit takes them), the oracle's hit records of a ray set, and the comparison of
any implementation's first-hit quantities with tests/first_hit_ref.cast under its margins and constants."""
import ctypes as C

import numpy as np

from oracle import pyoracle as O
from tests import aov_ref as A
from tests import first_hit_ref as F
from tests import first_hit_worlds as FW

f32 = np.float32
_rays = {}
_casts = {}
_planes = {}
_worlds = {}


def _key(world, size, seed):
    """The caches are keyed by the world object itself (and hold it, so its id stays its own)."""
    _worlds[id(world)] = world
    return (id(world), size.width, size.height, seed)


def camera_rays(name, world, size, seed):
    """(origin (n, 3) f32, direction (n, 3) f32, time (n,) f32, point (n, 2) f32) of sample 0 of every pixel, row-major
    from the top-left pixel; cached by (world, size, seed).  `name` only labels messages."""
    key = _key(world, size, seed)
    if key not in _rays:
        n = size.count()
        o, d, t, p = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros((n, 2), f32)
        for pix in range(n):
            ro, rd, rt, _, pt = A.primary_ray(world, size, seed, pix % size.width, pix // size.width, 0)
            o[pix], d[pix], t[pix], p[pix] = list(ro), list(rd), rt.value, pt
        _rays[key] = (o, d, t, p)
    return _rays[key]


def camera_cast(name, world, size, seed):
    """The caster's answer to camera_rays(...), cached (the host and the device tests share it, unchanged)."""
    key = _key(world, size, seed)
    if key not in _casts:
        o, d, t, _ = camera_rays(name, world, size, seed)
        _casts[key] = F.cast(world, o, d, t)
    return _casts[key]


def oracle_hits(world, o, d, t):
    """rtw_oracle_scene_hit over [0.001, inf) for every ray: a dict of arrays like the caster's."""
    L = O.lib()
    n = len(o)
    out = dict(hit=np.zeros(n, bool), t=np.zeros(n, f32), position=np.zeros((n, 3), f32), normal=np.zeros((n, 3), f32),
               uv=np.zeros((n, 2), f32), front_face=np.zeros(n, bool), material=np.full(n, -1))
    h = O.OracleHit()
    o, d, t = (np.ascontiguousarray(a, f32) for a in (o, d, t))
    fp = C.POINTER(C.c_float)
    for i in range(n):
        state = (C.c_uint64 * 2)(1, 2)
        assert L.rtw_oracle_scene_hit(world.ptr(), o[i].ctypes.data_as(fp), d[i].ctypes.data_as(fp), float(t[i]),
                                      f32(F.T_START), f32(np.inf), state, C.byref(h)) == 0
        out["hit"][i] = bool(h.hit)
        if h.hit:
            out["t"][i], out["front_face"][i], out["material"][i] = h.t, bool(h.front_face), h.material
            out["position"][i], out["normal"][i], out["uv"][i] = list(h.position), list(h.normal), list(h.uv)
    return out


def oracle_albedo(world, o, d, t):
    """The albedo at the first hit through aov_ref.Twin: the emissive twin's radiance at max_depth 2 (1 on a miss)."""
    tw = A.Twin(world)
    L = O.lib()
    o, d, t = (np.ascontiguousarray(a, f32) for a in (o, d, t))
    out = np.zeros((len(o), 3), f32)
    fp = C.POINTER(C.c_float)
    for i in range(len(o)):
        state = (C.c_uint64 * 2)(1, 2)
        assert L.rtw_oracle_ray_color(tw.ptr(), o[i].ctypes.data_as(fp), d[i].ctypes.data_as(fp), float(t[i]), 2, 0,
                                      state, out[i].ctypes.data_as(fp)) == 0
    return out


def describe(res, rays, i, got):
    o, d, t = rays[:3]
    lines = [f"ray {i}: origin {o[i]} direction {d[i]} time {t[i]}",
             f"  caster: hit {res['hit'][i]} leaf {res['leaf'][i]} t {res['t'][i]:.9g} position {res['position'][i]} "
             f"normal {res['normal'][i]} uv ({res['u'][i]:.7g}, {res['v'][i]:.7g}) front {res['front_face'][i]} "
             f"material {res['material'][i]} albedo {res['albedo'][i]}",
             "  margins: " + ", ".join(f"{k} {v[i]:.3g}" for k, v in res["margins"].items()),
             "  scales:  " + ", ".join(f"{k} {v[i]:.3g}" for k, v in res["S"].items()),
             "  got:     " + ", ".join(f"{k} {np.asarray(v)[i]}" for k, v in got.items())]
    return "\n".join(lines)


def compare(res, rays, got, what, width=None):
    """`got` holds some of hit, t, position, normal, uv, front_face, material, albedo (arrays over the rays).  Asserts
    on the compared rays: hit or miss and the integers exactly, the floats within K_q U S_q.  Returns the worst
    error of each float quantity in units of U S_q."""
    m = res["compared"]
    hit = res["hit"]

    def fail(i, why):
        where = f" pixel ({i % width}, {i // width})" if width else ""
        raise AssertionError(f"{what}:{where} {why}\n" + describe(res, rays, i, got))

    if "hit" in got:
        bad = m & (np.asarray(got["hit"], bool) != hit)
        if bad.any():
            fail(int(np.nonzero(bad)[0][0]), f"hit or miss differs on {int(bad.sum())} compared rays")
    mh = m & hit
    for k in ("front_face", "material"):
        if k in got:
            bad = mh & (np.asarray(got[k]) != res[k])
            if bad.any():
                fail(int(np.nonzero(bad)[0][0]), f"{k} differs on {int(bad.sum())} compared rays")
    worst = {}

    def floats(key, have, want, scale, mask, kq):
        err = np.abs(np.asarray(have, np.float64) - want)
        if err.ndim == 2:
            err = err.max(axis=1)
        with np.errstate(invalid="ignore"):
            rel = np.where(mask, err / (F.U * scale), 0.0)
        rel = np.where(np.isnan(rel), np.inf, rel)
        worst[key] = max(worst.get(key, 0.0), float(rel.max()) if len(rel) else 0.0)
        if (rel > F.K[kq]).any():
            i = int(np.argmax(rel))
            fail(i, f"{key} is off by {rel[i]:.3g} U S (allowed {F.K[kq]}), on {int((rel > F.K[kq]).sum())} compared rays")

    S = res["S"]
    if "t" in got:
        floats("t", got["t"], res["t"], S["t"], mh, "t")
    if "position" in got:
        floats("position", got["position"], res["position"], S["position"], mh, "position")
    if "normal" in got:  # a Normals frame holds the background on a miss: compared too, scale 1
        floats("normal", got["normal"], res["normal"], np.where(hit, S["normal"], 1.0), m if "encoded normal" in got else mh,
               "normal")
    if "uv" in got:
        uv = np.asarray(got["uv"], np.float64)
        floats("uv", uv[:, 0], res["u"], S["u"], mh, "uv")
        floats("uv", uv[:, 1], res["v"], S["v"], mh, "uv")
    if "albedo" in got:
        floats("albedo", got["albedo"], res["albedo"], S["albedo"], m, "albedo")
        marble = mh & (res["tex_kind"] == FW.N.TEX_MARBLE)
        if marble.any():  # (recorded apart: its scale is the only hand-built one among the textures)
            floats("albedo of marble", got["albedo"], res["albedo"], S["albedo"], marble, "albedo")
    return worst


def case_counts(res):
    """({(kind, face, wrapper): compared rays}, {texture kind: compared rays})."""
    m = res["compared"] & res["hit"]
    cases, tex = {}, {}
    for k, pl, ff, fl, ys in zip(res["kind"][m], res["plane"][m], res["front_face"][m], res["flags"][m], res["y_sin"][m]):
        key = (FW.KIND_NAMES[int(k)] + FW.PLANE_NAMES[int(pl)], "front" if ff else "back",
               FW.wrapper_name(int(fl), float(ys)))
        cases[key] = cases.get(key, 0) + 1
    for k in res["tex_kind"][m]:
        tex[FW.TEX_NAMES[int(k)]] = tex.get(FW.TEX_NAMES[int(k)], 0) + 1
    tex["checker"] = int(res["checkered"][m].sum())
    return cases, tex


def assert_cases(name, res):
    cases, tex = case_counts(res)
    for c in FW.CASES[name]:
        assert cases.get(c, 0) >= FW.MIN_RAYS, f"world {name}: case {c} has {cases.get(c, 0)} compared rays: {cases}"
    for t in FW.TEXTURES[name]:
        assert tex.get(t, 0) >= FW.MIN_RAYS, f"world {name}: texture {t} has {tex.get(t, 0)} compared rays: {tex}"
    left = 1.0 - res["compared"].mean()
    assert left <= 0.10, f"world {name}: {100 * left:.2f} % of the rays left out: {F.left_out_by(res)}"
    return left


def oracle_planes(name, world, size, seed):
    """The oracle's four first-hit planes of a one-sample frame: albedo (the twin), normal (the Normals frame),
    depth and hits (the per-sample loop); cached."""
    import raytracinginaweekend_amd as R

    key = _key(world, size, seed)
    if key not in _planes:
        depth, hits = A.depth_hits(world, size, 1, seed)
        normal = O.render(world, R.render_params(size, 1, 50, R.RenderMode.Normals, seed=seed))
        _planes[key] = dict(albedo=A.twin_albedo(world, size, 1, seed), normal=normal, depth=depth, hits=hits)
    return _planes[key]


def compare_planes(name, world, size, seed, planes, what):
    """The planes of a one-sample frame (any of albedo, normal, depth, hits; `normal` is the Normals encoding
    0.5 (n + 1), the background on a miss) against the caster on the frame's camera rays, under the same rules and
    constants as the records: hits is hit or miss, depth is t, 2 normal - 1 is the normal, albedo is the albedo.
    Returns the worst errors in units of U S."""
    rays = camera_rays(name, world, size, seed)
    res = camera_cast(name, world, size, seed)
    got = {}
    if "hits" in planes:
        assert set(np.unique(planes["hits"])) <= {0, 1}
        got["hit"] = np.asarray(planes["hits"]) == 1
    if "depth" in planes:
        got["t"] = planes["depth"]
    if "normal" in planes:
        n = np.asarray(planes["normal"], np.float64)
        got["normal"] = np.where(res["hit"][:, None], 2.0 * n - 1.0, n)
        got["encoded normal"] = n
    if "albedo" in planes:
        got["albedo"] = planes["albedo"]
    return compare(res, rays, got, what, size.width)
