"""What the path-step tests share (tests/test_path_host.py on the CPU, tests/test_gpu_path.py on the device): the
oracle's recorded paths of a world's camera rays, the stepper's answer to every recorded vertex, the vertex rays
taken as query rays, the one-bounce prediction of leg d and the comparisons, under the margins and constants of
tests/path_ref.py.  Everything is cached per (world, copy) and left unchanged."""
import numpy as np

from oracle import pyoracle as O
from tests import aov_ref as A
from tests import first_hit_ref as F
from tests import path_ref as P
from tests import path_worlds as PW

f32 = np.float32
SEED = 1
DEPTH = 6
QUERY_SAMPLES = 4
QUERY_RAYS = 2000
MAX_LEFT_OUT = 0.10

_paths, _steps, _queries, _predictions = {}, {}, {}, {}


def camera_paths(name, copy):
    """(rays (o, d, t), vertices (n, DEPTH), counts, colors) of rtw_oracle_path at max_depth DEPTH for sample 0 of
    every pixel, each on the stream its camera ray left behind."""
    key = (name, copy)
    if key not in _paths:
        world = PW.world(name, copy)
        W = PW.SIZE.width
        n = PW.SIZE.count()
        o, d, t = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, f32)
        states = np.zeros((n, 2), np.uint64)
        for pix in range(n):
            ro, rd, rt, st, _ = A.primary_ray(world, PW.SIZE, SEED, pix % W, pix // W, 0)
            o[pix], d[pix], t[pix], states[pix] = list(ro), list(rd), rt.value, list(st)
        vertices, counts, colors, _ = O.paths(world, o, d, t, states, DEPTH)
        for a in (vertices, counts, colors, states):
            a.setflags(write=False)
        _paths[key] = ((o, d, t, states), vertices, counts, colors)
    return _paths[key]


def flat_vertices(name, copy):
    """Every recorded vertex of camera_paths: (records (m,), path index (m,), segment index (m,))."""
    _, vertices, counts, _ = camera_paths(name, copy)
    k = np.arange(vertices.shape[1])[None, :]
    path, seg = np.nonzero(k < counts[:, None])
    return vertices[path, seg], path, seg


def vertex_steps(name, copy):
    """step() of every recorded vertex, started from the oracle's own f32 segment ray and stream, at the depth the
    oracle's loop had there, the primary direction its path's first."""
    key = (name, copy)
    if key not in _steps:
        V, path, seg = flat_vertices(name, copy)
        rays, _, _, _ = camera_paths(name, copy)
        _steps[key] = P.step(PW.world(name, copy), V["origin"], V["dir"], V["time"], V["state_before"], DEPTH - seg,
                             rays[1][path])
    return _steps[key]


class Mismatch(AssertionError):
    pass


def _describe(res, i, V=None):
    lines = [f"step {i}: decision {res['decision'][i]} end {res['end'][i]} hit {res['hit'][i]} leaf {res['leaf'][i]} "
             f"front {res['front_face'][i]} material {res['material'][i]}",
             f"  stepper: direction {res['direction'][i]} a {res['a'][i]} e {res['e'][i]} prob {res['prob'][i]} "
             f"state {res['state_after'][i]}",
             "  margins: " + ", ".join(f"{k} {v[i]:.3g}" for k, v in res["margins"].items()),
             "  scales:  " + ", ".join(f"{k} {v[i]:.3g}" for k, v in res["S"].items())]
    if V is not None:
        v = V[i]
        lines.append(f"  oracle:  ray {v['origin']} {v['dir']} {v['time']} hit {v['hit']} leaf {v['leaf']} end {v['end']} "
                     f"scattered {v['scattered']} a {v['a']} e {v['e']} prob {v['prob']} state {v['state_after']}")
    return "\n".join(lines)


def compare_steps(res, V, what):
    """The oracle's records V against the stepper's res on the compared steps: hit or miss, leaf, material, face, the
    end of the segment, scatters, the stream's end state and prob's NaN-ness exactly; direction, prob, a and e within
    K U S.  Returns the worst error of each float quantity in units of U S."""
    m = res["compared"]

    def exact(key, have, want, mask):
        bad = mask & (np.asarray(have) != np.asarray(want))
        if bad.ndim == 2:
            bad = bad.any(axis=1)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise Mismatch(f"{what}: {key} differs on {int(bad.sum())} compared steps\n" + _describe(res, i, V))

    exact("hit", V["hit"] == 1, res["hit"], m)
    mh = m & res["hit"]
    exact("leaf", V["leaf"], res["leaf"], mh)
    exact("material", V["material"], res["material"], mh)
    exact("front_face", V["front_face"] == 1, res["front_face"], mh)
    exact("end", V["end"], res["end"], m)
    exact("scatters", V["scatters"] == 1, res["scatters"], m)
    exact("the stream's end state", V["state_after"], res["state_after"], m[:, None])
    sc = m & res["scatters"]
    exact("NaN-ness of prob", np.isnan(V["prob"]), np.isnan(res["prob"]), sc)
    worst = {}

    def floats(key, have, want, mask):
        err = np.abs(np.asarray(have, np.float64) - want)
        if err.ndim == 2:
            err = err.max(axis=1)
        with np.errstate(invalid="ignore"):
            rel = np.where(mask, err / (P.U * res["S"][key]), 0.0)
        rel = np.where(np.isnan(rel), np.inf, rel)
        worst[key] = float(rel.max()) if len(rel) else 0.0
        if (rel > P.K[key]).any():
            i = int(np.argmax(rel))
            raise Mismatch(f"{what}: {key} is off by {rel[i]:.3g} U S (allowed {P.K[key]}) on {int((rel > P.K[key]).sum())} "
                           f"compared steps\n" + _describe(res, i, V))

    floats("direction", V["scattered"], res["direction"], sc)
    floats("prob", V["prob"], res["prob"], sc & ~np.isnan(res["prob"]))
    floats("a", V["a"], res["a"], sc)
    floats("e", V["e"], res["e"], m)
    return worst


def assert_caps(name, res, what, cases=True):
    """Leg e: at most MAX_LEFT_OUT of the steps left out, every listed case with its MIN_STEPS compared steps."""
    left = 1.0 - res["compared"].mean()
    assert left <= MAX_LEFT_OUT, f"{what}: {100 * left:.2f} % of the steps left out: {P.left_out_by(res)}"
    counts = PW.case_counts(res, PW.world(name, "sky").raw)
    if cases:
        for c in PW.CASES[name]:
            assert counts.get(c, 0) >= PW.MIN_STEPS, f"{what}: case {c} has {counts.get(c, 0)} compared steps: {counts}"
    return left, counts


# ---- leg b -------------------------------------------------------------------------------------------------------
def assert_chained(name, copy):
    """Vertex k + 1's ray is (position_k, direction_k, time_0) and its stream vertex k's end state, bit for bit."""
    _, vertices, counts, _ = camera_paths(name, copy)
    links = 0
    for k in range(vertices.shape[1] - 1):
        m = counts > k + 1
        a, b = vertices[m, k], vertices[m, k + 1]
        assert (a["end"] == O.PATH_CONTINUES).all() and (a["scatters"] == 1).all()
        for have, want in ((b["origin"], a["position"]), (b["dir"], a["scattered"]), (b["time"], vertices[m, 0]["time"])):
            assert np.array_equal(have.view(np.uint32), want.view(np.uint32)), f"{name} {copy}: segment {k + 1}'s ray"
        assert np.array_equal(b["state_before"], a["state_after"]), f"{name} {copy}: segment {k + 1}'s stream"
        links += int(m.sum())
    last = vertices[np.arange(len(counts)), counts - 1]
    assert ((last["end"] != O.PATH_CONTINUES) | (counts == vertices.shape[1])).all()
    return links


# ---- leg d -------------------------------------------------------------------------------------------------------
def query_rays(name, copy):
    """The vertex rays: the segments 1.. of the camera paths, thinned to about QUERY_RAYS, as (n, 8) rtw_ray records
    (origin, time, direction, t_end = inf)."""
    key = (name, copy)
    if key not in _queries:
        V, _, seg = flat_vertices(name, copy)
        V = V[seg >= 1]
        # those that meet the subject again come first (a ray that ends on the detector or the sky draws nothing); the
        # others are a fifth of the set, or what the first kind leaves of it
        again = (V["hit"] == 1) & ((V["scatters"] == 1) | (V["end"] == O.PATH_END_DEPTH) | (V["e"] == 0).all(axis=1))
        def thin(X, want):
            return X[np.linspace(0, len(X) - 1, min(len(X), want)).astype(np.int64)]

        A_ = thin(V[again], QUERY_RAYS * 4 // 5)
        V = np.concatenate([A_, thin(V[~again], QUERY_RAYS - len(A_))])
        rays = np.zeros((len(V), 8), f32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = V["origin"], V["time"], V["dir"], np.inf
        rays.setflags(write=False)
        _queries[key] = rays
    return _queries[key]


def query_streams(n, seed=SEED, samples=QUERY_SAMPLES, first_ray=0, first_sample=0):
    return np.array([A.sample_stream(seed, first_ray + i, first_sample + k) for i in range(n) for k in range(samples)],
                    np.uint64)


def one_bounce(name, copy):
    """The stepper's prediction of the radiance of the query rays' samples (n * QUERY_SAMPLES, ray-major) at
    max_depth 2 (sky copy: black if the scattered ray hits, else e0 + a0 prob0 background(query ray)) or 3 (detector
    copy: e0 + a0 prob0 texel if the scattered ray ends on the detector, else black).  A dict: colour (m, 3) f64, S
    (m,), compared (m,), first (the step), second (the scattered ray's cast)."""
    key = (name, copy)
    if key not in _predictions:
        world = PW.world(name, copy)
        tb = F.Tables(world)
        rays = query_rays(name, copy)
        o, d, t = (np.repeat(a, QUERY_SAMPLES, axis=0) for a in (rays[:, 0:3], rays[:, 4:7], rays[:, 3]))
        first = P.step(tb, o, d, t, query_streams(len(rays)), 3, d)
        sc = first["scatters"]
        second = F.cast(tb, first["position"][sc], first["direction"][sc], t[sc])
        m = len(o)
        hit2 = np.zeros(m, bool)
        hit2[sc] = second["hit"]
        compared = first["compared"].copy()
        compared[sc] &= second["compared"]
        x = np.zeros((m, 3))
        Sx = np.zeros(m)
        if copy == "sky":
            x[sc & ~hit2] = P.background(world.raw, d)[sc & ~hit2]
            Sx[sc & ~hit2] = 1.0
        else:
            light = np.zeros(m, bool)
            kinds = np.array([world.raw.materials[i].kind if i >= 0 else -1 for i in second["material"]])
            light[sc] = second["hit"] & (kinds == P.N.MAT_DIFFUSE_LIGHT)
            x[light] = second["albedo"][light[sc]]
            Sx[light] = second["S"]["albedo"][light[sc]]
        a, e, p = first["a"], first["e"], first["prob"]
        with np.errstate(invalid="ignore"):
            lit = np.abs(x).max(axis=1) > 0
            colour = np.where((sc & lit)[:, None], e + a * p[:, None] * x, np.where(sc[:, None], 0.0, e))
            amax, xmax, pa = np.abs(a).max(axis=1), np.abs(x).max(axis=1), np.abs(p)
            S = np.where(sc & lit, first["S"]["e"] + pa * xmax * first["S"]["a"] + amax * xmax * first["S"]["prob"]
                         + amax * pa * Sx + 3.0 * np.abs(colour).max(axis=1), first["S"]["e"] + 1.0)
        # a NaN weight times a black texel is still NaN: the prediction above keeps it only where the texel is lit,
        # so such samples (prob NaN, the scattered ray on a hit that ends black) are predicted black -- as ray_color
        # returns at depth <= 1 before the weight is ever used
        _predictions[key] = dict(colour=colour, S=np.where(np.isnan(S), 1.0, S), compared=compared, first=first,
                                 second=second)
    return _predictions[key]


def compare_one_bounce(name, copy, samples, what):
    """Radiance samples (n, QUERY_SAMPLES, 3) f32 of the query rays (the oracle's or the device's) against
    one_bounce's prediction on the compared samples: the zero / non-zero pattern and NaN-ness exactly, the value within
    K["colour"] U S.  Returns (worst error in U S, left-out share)."""
    pred = one_bounce(name, copy)
    got = np.asarray(samples, np.float64).reshape(-1, 3)
    want, m = pred["colour"], pred["compared"]
    assert got.shape == want.shape
    for key, have, expect in (("NaN-ness", np.isnan(got).any(axis=1), np.isnan(want).any(axis=1)),
                              ("the zero / non-zero pattern", (got != 0).any(axis=1), (want != 0).any(axis=1))):
        bad = m & (have != expect)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise Mismatch(f"{what}: {key} differs on {int(bad.sum())} compared samples; sample {i} (ray {i // QUERY_SAMPLES}): "
                           f"got {got[i]} predicted {want[i]}\n" + _describe(pred["first"], i))
    ok = m & ~np.isnan(want).any(axis=1)
    rel = np.where(ok, np.abs(np.where(ok[:, None], got - want, 0.0)).max(axis=1) / (P.U * pred["S"]), 0.0)
    if (rel > P.K["colour"]).any():
        i = int(np.argmax(rel))
        raise Mismatch(f"{what}: the colour is off by {rel[i]:.3g} U S (allowed {P.K['colour']}) on "
                       f"{int((rel > P.K['colour']).sum())} compared samples; sample {i}: got {got[i]} predicted {want[i]}\n"
                       + _describe(pred["first"], i))
    return float(rel.max()), 1.0 - m.mean()


def oracle_query_samples(name, copy, max_depth, seed=SEED):
    """rtw_oracle_ray_color of the query rays' samples: (n, QUERY_SAMPLES, 3) f32."""
    rays = query_rays(name, copy)
    o, d, t = (np.repeat(a, QUERY_SAMPLES, axis=0) for a in (rays[:, 0:3], rays[:, 4:7], rays[:, 3]))
    colors, _ = O.ray_colors(PW.world(name, copy), o, d, t, query_streams(len(rays), seed), max_depth)
    return colors.reshape(len(rays), QUERY_SAMPLES, 3)


BOUNCE_DEPTH = {"sky": 2, "detector": 3}
