"""A plain f64 restatement of one segment of ray_color: "what a path does at a hit" (DESIGN.md 3, U13).

The oracle's material_scatter, dist_generate, light_generate, light_value, material_scattering_pdf and ray_color's
bookkeeping (oracle/rtw_oracle.c) and the kernels' shade() come from one reading of the Rust text by one author.
This module is the other side: numpy float64, written from the mathematics, sharing with them only the stream of
draws.  `step(world, origin, direction, time, state, depth, primary_direction)` answers, for every ray,

  the caster's hit fields (tests/first_hit_ref.cast over [0.001, inf), with its margins),
  end (CONTINUES, END_MISS, END_DEPTH, END_ABSORBED), scatters, the decision taken (`decision`: "miss", "depth",
  "emit", "absorbed", "reflect", "refract", "tir", "light_branch", "lobe_branch"; `fallback_normal` apart),
  direction, a (attenuation), e (emitted; the background along the PRIMARY ray at a miss), prob, the stream's
  state afterwards, and the margins and scales of what it decided and computed.

Reference lines (file:line of the Rust's src/lib):
  Lambert      material.rs:59-63, 17-33   albedo, Cosine(normal): unit_or_else(normal + UnitSphere, normal); value
                                          max(dot(normal, dir), 0) / pi; vec3.rs:223-230 (len_sq > 1e-8)
  Metal        material.rs:65-79          reflect + fuzz * UnitBall (drawn only if fuzz > 0); scatter only if
                                          dot(direction, normal) > 0 on the hit's (shading) normal; then unit()
  Dielectric   material.rs:80-105         ratio = front ? 1 / ior : ior; cos = min(dot(-d, n), 1); cannot_refract =
                                          ratio sin > 1; Schlick's r0 from the RATIO, powi(5); `reflectance > gen::<f32>()`
                                          is drawn only when refraction is possible (|| short-circuits); unit(); white
  reflect      vec3.rs:232-234            ray - 2 dot(ray, n) n
  refract      vec3.rs:235-240            perp = eta (ray + min(dot(-ray, n), 1) n); par = -sqrt|1 - |perp|^2| n
  DiffuseLight material.rs:112, 132-137   no scatter; emit samples the texture whatever the face
  mixture      rendering.rs:73-92         gen_bool(0.5) first; true: the light's generate; p = 0.5 light + 0.5 lobe
  light        rect_geometry.rs:60-85     generate draws p0 then p1, unit(e - origin); value hits the rect along
                                          (origin, dir, time 0) over [0.001, inf): t^2 / (|dot(n, dir)| area)
  weight       rendering.rs:46-58         prob = scattering_pdf / pdf (1 for a Mirror); 0 / 0 is NaN
  bookkeeping  rendering.rs:19-71         black at a hit with depth <= 1; the background of the PRIMARY ray (:67);
                                          emit on every hit; time carried on; att = (att * a) * prob

Draws.  The five samplers come from oracle/pyref.Xoro as f32 values (gen_f32, gen_range_f32, gen_bool, unit_sphere,
unit_ball; pinned by tests/test_distributions.py, tests/test_rng.py and, against include/rtw_scalar.h, by
tests/test_path_host.py::test_the_draws); everything after a draw is float64.

Out of scope.  Volume leaves and Isotropic: the caster refuses volume leaves, S4 (tests/analytic_scenes.py) pins the
free path, and the isotropic direction is the UnitSphere draw itself.  `step` raises on an Isotropic hit.

Tolerances.  |q32 - q64| <= K_q U S_q as in tests/first_hit_ref.py: U = 2^-24, S_q built per step from the step's
own magnitudes (where `S` is filled below; S_normal and S_position are the caster's).  A refracted direction
carries 1 / sqrt|1 - |perp|^2| (the root's derivative near the critical angle), prob carries light_value's
conditioning: t^2 / (cos area) has the relative error 2 dt / t + d(cos) / cos, weighed by the light's share of p.
K_q is the next power of two at or above 4 x the worst compared step of the oracle against this stepper on the
CPU over the worlds of tests/path_worlds.py; the figures stand beside K below and in profiles/r25/path_ref.txt.

Margins.  Every decision q > 0 the stepper takes has an error scale E_q (in units of U) built like the S_q; the
margin is |q| / (U E_q) and a step is compared only if it exceeds THRESHOLDS[name], and if the segment's cast is
compared.
"""
import numpy as np

from oracle import pyref
from raytracinginaweekend_amd import _native as N
from tests import first_hit_ref as F

U = F.U
INF = np.inf
CONTINUES, END_MISS, END_DEPTH, END_ABSORBED = 0, 1, 2, 3  # oracle/rtw_oracle.h RTW_PATH_*

# ---- thresholds: |q| / (U E_q) of a decision q against 0, E_q its f32 error scale ------------------------------
# One derivation for all: the f32 value of q differs from this module's by at most K U E_q, K the constant of the
# kindred float quantity (at most 8 below, 16 for the caster's t); 64 is four times the largest, so the f32 sign is
# ours.  That the choice holds is asserted, not assumed: every decision is exact on every compared step.
THRESHOLDS = {
    "tir": 64.0,       # ratio sin - 1: E from d(cos) = |d| (S_normal + |n|) through sin = sqrt(1 - cos^2)
    "coin": 64.0,      # reflectance - draw: E from d(cos) through 5 (1 - cos)^4, plus the polynomial's own rounding
    "absorb": 64.0,    # dot(direction, n) of a metal: E = |n| S_direction + |direction| (S_normal + |n|)
    "lobe_len": 64.0,  # |n + s|^2 - 1e-8: E = 2 |n + s| (S_normal + |n| + 1)
    "lobe_max": 64.0,  # dot(n, direction) of a Lambert against 0 (the max): E = |n| S_direction + S_normal + |n|
    "light_border": 64.0,  # distance of light_value's plane hit to the rect's border: E from the position, t and direction
    "light_facing": 64.0,  # the direction's component along the light's axis (the sign of t): E = S_direction
    "light_start": 64.0,   # t - 0.001 of light_value: E = t (relative error of t)
}

# ---- tolerance constants: the next power of two at or above 4 x the measured worst (units of U S_q) -------------
# Measured: rtw_oracle_path against step() on the CPU (tests/test_path_host.py legs a and d, all worlds of
# tests/path_worlds.py, camera and vertex rays).  Worst compared step per quantity (profiles/r25/path_ref.txt):
#   direction 0.679 (P-lambert)   prob 0.192 (P-mix)   a 0.494 (P-lambert: a texel / 255 rounded to f32)
#   e 1.216 (the sky's lerp, S_e = 1)   colour (leg d) 0.603 (P-lambert sky)
# 4 x: 2.72, 0.77, 1.98, 4.86, 2.41.  (The scales are generous where they carry the caster's S_normal and S_position
# whole; the mutations of profiles/r25/path_ref.txt exceed these constants by three orders of magnitude and more.)
K = {"direction": 4.0, "prob": 1.0, "a": 2.0, "e": 8.0, "colour": 4.0}

DECISIONS = ("miss", "depth", "emit", "absorbed", "reflect", "refract", "tir", "light_branch", "lobe_branch")


def _dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def _norm(a):
    return np.sqrt(_dot(a, a))


def background(raw, direction):
    """background_color.rs:9-19 along `direction` (R, 3): the sky's lerp of white and (0.5, 0.7, 1.0), or the colour."""
    d = np.asarray(direction, np.float64).reshape(-1, 3)
    if raw.background.kind == N.BG_SOLID:
        return np.tile(np.array(list(raw.background.color), np.float64), (len(d), 1))
    k = 0.5 * (d[:, 1] + 1.0)
    return (1.0 - k)[:, None] * np.ones(3) + k[:, None] * np.array([0.5, 0.7, 1.0])


def light_value(rect, origin, direction):
    """rect_geometry.rs:68-85 for (R, 3) origins and directions: (value, t, cos, inside, along): the pdf (0 where the
    ray (origin, direction) does not hit the rect over [0.001, inf)), and what decided it: the plane's t, |dir_n|,
    the signed distance to the border (>= 0 inside) and the direction's component along the axis."""
    p0, p1, n = F.RECT_AXES[rect.plane]
    k, a0, a1, b0, b1 = float(rect.dist), float(rect.r0[0]), float(rect.r0[1]), float(rect.r1[0]), float(rect.r1[1])
    along = direction[:, n]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (k - origin[:, n]) / along
    inr = np.isfinite(t) & (t >= F.T_START)
    tt = np.where(inr, t, 0.0)
    x, y = origin[:, p0] + tt * direction[:, p0], origin[:, p1] + tt * direction[:, p1]
    inside = np.minimum(np.minimum(x - a0, a1 - x), np.minimum(y - b0, b1 - y))
    hit = inr & (inside >= 0)
    area = (a1 - a0) * (b1 - b0)
    cos = np.abs(along)  # the rect's normal is -axis, flipped or not: |dot| is |dir_n|
    with np.errstate(divide="ignore", invalid="ignore"):
        value = np.where(hit, t * t / (cos * area), 0.0)
    return value, t, cos, np.where(inr, inside, INF), along


def step(world, origin, direction, time, state, depth, primary_direction):
    """One segment of ray_color for every ray (module docstring).  origin, direction, primary_direction (R, 3) and
    time (R,) of any float type, taken as exact; state (R, 2) uint64; depth an int or (R,) ints.  Returns a dict of
    per-ray arrays; `margins` and `S` are dicts name -> (R,), `compared` the steps whose margins all pass."""
    tb = world if isinstance(world, F.Tables) else F.Tables(world)
    raw = tb.raw
    o = np.asarray(origin, np.float64).reshape(-1, 3)
    d = np.asarray(direction, np.float64).reshape(-1, 3)
    tm = np.asarray(time, np.float64).reshape(-1)
    R = len(o)
    depth = np.broadcast_to(np.asarray(depth, np.int64), (R,))
    state = np.array(state, np.uint64).reshape(R, 2)
    res = F.cast(tb, o, d, tm)
    hit, n, pos, front = res["hit"], res["normal"], res["position"], res["front_face"]
    Sn, Sp = res["S"]["normal"], res["S"]["position"]
    nl, dl = _norm(n), _norm(d)

    end = np.full(R, END_MISS)
    scatters = np.zeros(R, bool)
    decision = np.full(R, "miss", dtype="<U12")
    fallback = np.zeros(R, bool)
    out_dir = np.zeros((R, 3))
    a = np.zeros((R, 3))
    e = np.zeros((R, 3))
    prob = np.zeros(R)
    state_after = state.copy()
    margins = {k: np.full(R, INF) for k in THRESHOLDS}
    S = {"direction": np.ones(R), "prob": np.ones(R), "a": np.ones(R), "e": np.ones(R)}

    # ---- a miss: the background along the primary ray (rendering.rs:67) ---------------------------------------
    e[~hit] = background(raw, np.asarray(primary_direction, np.float64).reshape(-1, 3)[~hit])
    # ---- a hit at depth <= 1: black (rendering.rs:26-27), nothing drawn ------------------------------------------
    shallow = hit & (depth <= 1)
    end[shallow], decision[shallow] = END_DEPTH, "depth"
    live = hit & ~shallow
    kind = np.full(R, -1)
    for mi in np.unique(res["material"][live]):
        kind[live & (res["material"] == mi)] = raw.materials[mi].kind
    if (kind[live] == N.MAT_ISOTROPIC).any():
        raise ValueError("an Isotropic hit is out of the stepper's scope")

    # ---- DiffuseLight: no scatter, emit on either face (material.rs:112, 132-137) ------------------------------
    m = live & (kind == N.MAT_DIFFUSE_LIGHT)
    end[m], decision[m] = END_ABSORBED, "emit"
    e[m] = res["albedo"][m]
    S["e"][m] = res["S"]["albedo"][m]

    def draws(idx, fn):
        """fn(rng, i) for every ray of idx on its own stream; the stream's end goes to state_after."""
        for i in idx:
            rng = pyref.Xoro(int(state[i, 0]), int(state[i, 1]))
            fn(rng, i)
            state_after[i] = (rng.s0, rng.s1)

    def reflect(v, nn):  # vec3.rs:232-234
        return v - 2.0 * _dot(v, nn)[:, None] * nn

    # ---- Metal (material.rs:65-79) ---------------------------------------------------------------------------------
    m = live & (kind == N.MAT_METAL)
    if m.any():
        idx = np.nonzero(m)[0]
        fuzz = np.array([float(raw.materials[res["material"][i]].fuzz) for i in idx])
        ball = np.zeros((len(idx), 3))
        where = {int(i): j for j, i in enumerate(idx)}

        def draw_ball(rng, i):
            ball[where[int(i)]] = [float(x) for x in rng.unit_ball()]

        draws(idx[fuzz > 0], draw_ball)
        raw_dir = reflect(d[idx], n[idx]) + fuzz[:, None] * ball
        q = _dot(raw_dir, n[idx])
        rl = _norm(raw_dir)
        # the f32 direction before unit(): d - 2 (d.n) n carries |d| + 4 |d| |n| (|n| + S_normal), the fuzz its own size
        s_raw = dl[idx] + 4.0 * dl[idx] * nl[idx] * (nl[idx] + Sn[idx]) + fuzz
        margins["absorb"][idx] = np.abs(q) / (U * (nl[idx] * s_raw + rl * (Sn[idx] + nl[idx])))
        ok = q > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            out_dir[idx] = np.where(ok[:, None], raw_dir / rl[:, None], 0.0)
            S["direction"][idx] = np.where(ok, s_raw / rl + 1.0, 1.0)
        scatters[idx] = ok
        end[idx] = np.where(ok, CONTINUES, END_ABSORBED)
        decision[idx] = np.where(ok, "reflect", "absorbed")
        a[idx] = np.where(ok[:, None], res["albedo"][idx], 0.0)
        S["a"][idx] = res["S"]["albedo"][idx]
        prob[idx] = np.where(ok, 1.0, 0.0)

    # ---- Dielectric (material.rs:80-105) ------------------------------------------------------------------------
    m = live & (kind == N.MAT_DIELECTRIC)
    if m.any():
        idx = np.nonzero(m)[0]
        ior = np.array([float(raw.materials[res["material"][i]].index_of_refraction) for i in idx])
        ratio = np.where(front[idx], 1.0 / ior, ior)
        nn, dd = n[idx], d[idx]
        cos = np.minimum(_dot(-dd, nn), 1.0)
        sin = np.sqrt(np.maximum(1.0 - cos * cos, 0.0))
        cannot = ratio * sin > 1.0
        dcos = dl[idx] * (Sn[idx] + nl[idx])  # the f32 cos: |d| d(n) and the dot's own rounding
        with np.errstate(divide="ignore"):
            margins["tir"][idx] = np.abs(ratio * sin - 1.0) / (U * (ratio * cos * dcos / np.maximum(sin, 1e-6) + ratio * sin + 1.0))
        r0 = (1.0 - ratio) / (1.0 + ratio)
        rs = r0 * r0
        x = 1.0 - cos
        refl = rs + (1.0 - rs) * x ** 5
        coin = np.zeros(len(idx))
        where = {int(i): j for j, i in enumerate(idx)}

        def draw_coin(rng, i):
            coin[where[int(i)]] = float(rng.gen_f32())

        draws(idx[~cannot], draw_coin)
        margins["coin"][idx] = np.where(cannot, INF, np.abs(refl - coin) / (U * (5.0 * (1.0 - rs) * x ** 4 * dcos + 8.0)))
        mirror = cannot | (refl > coin)
        # refract (vec3.rs:235-240)
        perp = ratio[:, None] * (dd + cos[:, None] * nn)
        pp = _dot(perp, perp)
        root = np.sqrt(np.abs(1.0 - pp))
        refr = perp - root[:, None] * nn
        refl_dir = reflect(dd, nn)
        raw_dir = np.where(mirror[:, None], refl_dir, refr)
        rl = _norm(raw_dir)
        out_dir[idx] = raw_dir / rl[:, None]
        s_reflect = dl[idx] + 4.0 * dl[idx] * nl[idx] * (nl[idx] + Sn[idx])
        dperp = ratio * (dcos * nl[idx] + np.abs(cos) * Sn[idx] + dl[idx] + np.abs(cos) * nl[idx]) + _norm(perp)
        with np.errstate(divide="ignore"):
            droot = (2.0 * _norm(perp) * dperp + np.maximum(1.0, pp)) / (2.0 * np.maximum(root, 1e-30)) + root
        s_refract = dperp + droot * nl[idx] + root * Sn[idx]
        S["direction"][idx] = np.where(mirror, s_reflect, s_refract) / rl + 1.0
        scatters[idx] = True
        end[idx] = CONTINUES
        decision[idx] = np.where(cannot, "tir", np.where(mirror, "reflect", "refract"))
        a[idx] = 1.0
        prob[idx] = 1.0

    # ---- Lambert (material.rs:59-63) and the mixture (rendering.rs:73-92) --------------------------------------
    m = live & (kind == N.MAT_LAMBERT)
    if m.any():
        idx = np.nonzero(m)[0]
        k = len(idx)
        nn, pp = n[idx], pos[idx]
        has_light = bool(raw.has_light)
        g = raw.light
        light = np.zeros(k, bool)
        sphere = np.zeros((k, 3))
        target = np.zeros((k, 3))
        where = {int(i): j for j, i in enumerate(idx)}
        if has_light:
            p0, p1, ax = F.RECT_AXES[g.plane]

        def draw(rng, i):
            j = where[int(i)]
            if has_light and rng.gen_bool(0.5):
                light[j] = True
                target[j, p0] = float(rng.gen_range_f32(g.r0[0], g.r0[1]))  # p0 first (rect_geometry.rs:63-64)
                target[j, p1] = float(rng.gen_range_f32(g.r1[0], g.r1[1]))
                target[j, ax] = float(g.dist)
            else:
                sphere[j] = [float(x) for x in rng.unit_sphere()]

        draws(idx, draw)
        # the lobe: unit_or_else(n + s, n)
        v = nn + sphere
        len_sq = _dot(v, v)
        fb = ~light & ~(len_sq > 1e-8)
        vl = np.sqrt(len_sq)
        margins["lobe_len"][idx] = np.where(light, INF, np.abs(len_sq - 1e-8) / (U * (2.0 * vl * (Sn[idx] + nl[idx] + 1.0) + 1e-8)))
        with np.errstate(divide="ignore", invalid="ignore"):
            lobe_dir = np.where(fb[:, None], nn, v / vl[:, None])
            s_lobe = np.where(fb, Sn[idx], (Sn[idx] + nl[idx] + 1.0) / vl + 1.0)
        # the light: unit(e - position)
        to = target - pp
        tl = _norm(to)
        with np.errstate(divide="ignore", invalid="ignore"):
            light_dir = to / tl[:, None]
            s_light = (Sp[idx] + _norm(target) + _norm(pp)) / tl + 1.0
        dr = np.where(light[:, None], light_dir, lobe_dir)
        s_dir = np.where(light, s_light, s_lobe)
        cosine = _dot(nn, dr)
        e_cos = nl[idx] * s_dir + Sn[idx] + nl[idx]
        margins["lobe_max"][idx] = np.abs(cosine) / (U * e_cos)
        spdf = np.maximum(cosine, 0.0) / np.pi
        if has_light:
            lv, t, cos_l, inside, along = light_value(g, pp, dr)
            p = 0.5 * lv + 0.5 * spdf
            with np.errstate(divide="ignore", invalid="ignore"):
                gap = np.abs(float(g.dist) - pp[:, ax])
                rel_t = (Sp[idx] + abs(float(g.dist)) + np.abs(pp[:, ax])) / gap + s_dir / cos_l + 2.0
                ahead = np.isfinite(t) & (t > 0)
                tt = np.where(ahead, t, 0.0)
                e_border = Sp[idx] + _norm(pp) + tt * s_dir + tt * rel_t + np.abs(pp).max(axis=1) + tt
                margins["light_border"][idx] = np.where(ahead & np.isfinite(inside), np.abs(inside) / (U * e_border), INF)
                margins["light_facing"][idx] = np.abs(along) / (U * s_dir)
                margins["light_start"][idx] = np.where(np.isfinite(t), np.abs(t - F.T_START) / (U * np.abs(t) * rel_t), INF)
                rel_lv = 2.0 * rel_t + s_dir / cos_l + 4.0
        else:
            lv = np.zeros(k)
            p = spdf
            rel_lv = np.zeros(k)
        with np.errstate(divide="ignore", invalid="ignore"):
            pr = spdf / p  # 0 / 0: NaN, as the reference's
            share = np.where(lv > 0, 0.5 * lv / p, 0.0)  # the light's share of p
            rel_spdf = e_cos / np.abs(cosine)
            S["prob"][idx] = np.where(np.isfinite(pr) & (pr > 0), pr * (share * (rel_spdf + rel_lv) + 4.0), 1.0)
        out_dir[idx], prob[idx], fallback[idx] = dr, pr, fb
        S["direction"][idx] = s_dir
        scatters[idx] = True
        end[idx] = CONTINUES
        decision[idx] = np.where(light, "light_branch", "lobe_branch")
        a[idx] = res["albedo"][idx]
        S["a"][idx] = res["S"]["albedo"][idx]

    compared = res["compared"].copy()
    for k, thr in THRESHOLDS.items():
        compared &= margins[k] > thr
    out = dict(res)
    out.update(cast_compared=res["compared"], cast_margins=res["margins"], end=end, scatters=scatters,
               decision=decision, fallback_normal=fallback, direction=out_dir, a=a, e=e, prob=prob,
               state_after=state_after, margins=margins, S={**res["S"], **S}, compared=compared, mat_kind=kind)
    return out


def left_out_by(res):
    """{margin name: steps it alone or with others leaves out}, the cast's margins under "cast"."""
    out = {k: int((res["margins"][k] <= thr).sum()) for k, thr in THRESHOLDS.items()}
    out["cast"] = int((~res["cast_compared"]).sum())
    return out


# ------------------------------------------------------------------------------------------------------------
# the bookkeeping, numpy f32 (rendering.rs:19-71): a replay of recorded (a, e, prob) per vertex
# ------------------------------------------------------------------------------------------------------------
def replay(vertices, counts, max_depth, verify=False):
    """ray_color's colour from the records of rtw_oracle_path (a structured array (n, capacity), counts (n,)) cut at
    `max_depth`: acc += att * e; att = (att * a) * prob per scattering vertex; black at a hit with depth <= 1;
    acc + att * e at an absorber and at a miss (e holds the background along the primary ray there).  f32, one
    operation at a time, in the reference's order.  The records must come from a path of at least max_depth.
    verify: also assert the records' own att and acc after every scattering segment, bit for bit."""
    f32 = np.float32
    n = len(counts)
    att = np.ones((n, 3), f32)
    acc = np.zeros((n, 3), f32)
    out = np.zeros((n, 3), f32)
    done = np.zeros(n, bool)
    depth = max_depth
    with np.errstate(all="ignore"):
        for k in range(vertices.shape[1]):
            v = vertices[:, k]
            here = ~done & (k < counts)
            assert (done | here).all(), "a path's records ran out before it ended"
            hit = v["hit"] == 1
            black = here & hit & (depth <= 1)
            out[black] = 0
            done |= black
            here &= ~black
            final = here & (~hit | (v["scatters"] == 0))
            term = acc + att * v["e"]
            out[final] = term[final]
            done |= final
            go = here & ~final
            acc = np.where(go[:, None], term, acc)
            att = np.where(go[:, None], (att * v["a"]) * v["prob"][:, None], att)
            if verify:  # the records' own att and acc after a scattering segment
                for mine, theirs, what in ((att, v["att"], "att"), (acc, v["acc"], "acc")):
                    same = np.ascontiguousarray(mine[go]).view(np.uint32) == np.ascontiguousarray(theirs[go]).view(np.uint32)
                    both_nan = np.isnan(mine[go]) & np.isnan(theirs[go])
                    assert (same | both_nan).all(), f"segment {k}: the recorded {what} differs from the replay's"
            depth -= 1
            if done.all():
                break
    assert done.all(), "a path did not end within its records"
    assert out.dtype == f32
    return out
