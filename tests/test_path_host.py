"""What a path does at a hit, oracle against plain f64 mathematics (second axis, U13).

The oracle's recorded vertices (oracle/rtw_oracle.c: rtw_oracle_path, the loop rtw_oracle_ray_color runs) on one side,
tests/path_ref.step on the other: a numpy float64 restatement of one segment of ray_color that shares with it only
the stream of draws.  Over the worlds of tests/path_worlds.py, each in its detector and its sky copy:

  a. step by step   every recorded vertex, the stepper started from the oracle's own f32 segment ray and stream (errors
                    do not compound): hit or miss, leaf, the segment's end, scatters, the stream's end state and prob's
                    NaN-ness exactly, direction, prob, a and e within K U S
  b. chaining       vertex k + 1's ray is (position_k, direction_k, time_0), its stream vertex k's end state, bit for bit
  c. bookkeeping    a numpy-f32 replay of the recorded (a, e, prob) equals rtw_oracle_path's colour and
                    rtw_oracle_ray_color's bit for bit at max_depth 0, 1, 2, 3 and 6
  d. one bounce     the vertex rays as query rays from fresh streams (seed, i, k): the stepper predicts
                    rtw_oracle_ray_color at max_depth 2 (sky) and 3 (detector); tests/test_gpu_path.py asserts the same
                    of the kernels under the same constants
  e. caps           at most 10 % of the steps of any world and leg left out, every listed case with its 200 steps

and first of all the five samplers the stepper draws with (oracle/pyref.Xoro) against include/rtw_scalar.h's."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from oracle import pyref
from tests import path_check as Pc
from tests import path_ref as P
from tests import path_worlds as PW
from tests.parity import assert_bit_identical

HERE = os.path.dirname(os.path.abspath(__file__))
BOTH = [(n, c) for n in PW.NAMES for c in PW.COPIES]
IDS = [f"{n} {c}" for n, c in BOTH]
DRAW_STATES = 100000
RECORD = np.dtype([("start", "<u8", 2), ("gen", "<f4"), ("range_a", "<f4"), ("range_b", "<f4"), ("coin", "<u4"),
                   ("sphere", "<f4", 3), ("ball", "<f4", 3), ("end", "<u8", 2)])


def test_the_draws(tmp_path):
    """gen_f32, gen_range_f32, gen_bool, unit_sphere and unit_ball of oracle/pyref.Xoro against include/rtw_scalar.h's
    (tests/native/draws_check.c) on 10^5 start states: every value and the stream's end state."""
    exe = tmp_path / "draws_check"
    subprocess.run(["gcc", "-O2", "-std=c11", "-march=x86-64-v3", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "native", "draws_check.c"), "-lm"], check=True)
    out = subprocess.run([str(exe), str(DRAW_STATES)], capture_output=True, timeout=120, check=True).stdout
    rec = np.frombuffer(out, RECORD)
    assert len(rec) == DRAW_STATES and len(np.unique(rec["start"], axis=0)) == DRAW_STATES
    mine = np.zeros(DRAW_STATES, RECORD)
    for i, r in enumerate(rec):
        rng = pyref.Xoro(int(r["start"][0]), int(r["start"][1]))
        mine[i] = (r["start"], rng.gen_f32(), rng.gen_range_f32(213.0, 343.0), rng.gen_range_f32(-0.375, 0.0625),
                   rng.gen_bool(0.5), rng.unit_sphere(), rng.unit_ball(), (rng.s0, rng.s1))
    for key in RECORD.names:
        bad = np.nonzero(rec[key].view(np.uint32 if rec[key].dtype.itemsize == 4 else np.uint64).reshape(DRAW_STATES, -1)
                         != mine[key].view(np.uint32 if rec[key].dtype.itemsize == 4 else np.uint64).reshape(DRAW_STATES, -1))[0]
        assert len(bad) == 0, f"{key}: {len(bad)} of {DRAW_STATES} differ, first at state {rec['start'][bad[0]]}: " \
                              f"{rec[key][bad[0]]} (rtw_scalar.h) against {mine[key][bad[0]]} (pyref)"
    assert 0.49 < rec["coin"].mean() < 0.51 and set(np.unique(rec["coin"])) == {0, 1}


@pytest.mark.parametrize("name, copy", BOTH, ids=IDS)
def test_step_by_step(name, copy):
    """Legs a and e."""
    V, _, seg = Pc.flat_vertices(name, copy)
    res = Pc.vertex_steps(name, copy)
    worst = Pc.compare_steps(res, V, f"{name} {copy}")
    left, counts = Pc.assert_caps(name, res, f"{name} {copy}, leg a")
    print(f"{name} {copy}: {len(V)} steps ({int((seg >= 1).sum())} past the camera ray), left out {100 * left:.2f} % "
          f"{P.left_out_by(res)}, worst (U S) {worst}\n  cases {counts}")
    assert (seg >= 1).sum() >= 2000 and not res["fallback_normal"][res["compared"]].any()


@pytest.mark.parametrize("name, copy", BOTH, ids=IDS)
def test_chaining(name, copy):
    """Leg b."""
    links = Pc.assert_chained(name, copy)
    assert links >= 2000
    if name == "P-lambert":  # the shutter is open: the times differ from ray to ray, and every segment keeps its path's
        assert len(np.unique(Pc.camera_paths(name, copy)[0][2])) > 1000


@pytest.mark.parametrize("name, copy", BOTH, ids=IDS)
def test_bookkeeping(name, copy):
    """Leg c.  The replay (tests/path_ref.replay) works from the records of the depth-6 paths: a path at a smaller
    max_depth is a prefix of them, cut where depth reaches 1."""
    world = PW.world(name, copy)
    (o, d, t, states), vertices, counts, colors = Pc.camera_paths(name, copy)
    for max_depth in (0, 1, 2, 3, 6):
        want = P.replay(vertices, counts, max_depth, verify=max_depth == Pc.DEPTH)
        _, _, path_colors, after = O.paths(world, o, d, t, states, max_depth, capacity=Pc.DEPTH)
        ray_colors, after2 = O.ray_colors(world, o, d, t, states, max_depth)
        assert_bit_identical(path_colors, want, f"{name} {copy}, max_depth {max_depth}: rtw_oracle_path against the replay")
        assert_bit_identical(ray_colors, want, f"{name} {copy}, max_depth {max_depth}: rtw_oracle_ray_color against the replay")
        assert np.array_equal(after, after2)
        if max_depth == Pc.DEPTH:
            assert_bit_identical(path_colors, colors, "the cached paths")
    # the quirks are exercised: paths that end on a miss after a scatter (the PRIMARY ray's background, sky copy),
    # on an emitter after a scatter (emit, seen from inside the detector: a back face), on a hit at depth <= 1 (no
    # material that scatters emits, so accum_emitted is still black there: that it is dropped cannot be observed)
    last = vertices[np.arange(len(counts)), counts - 1]
    if copy == "sky":
        far = (last["end"] == O.PATH_END_MISS) & (counts >= 2)
        assert far.sum() >= 200
        moved = np.abs(last["dir"][far, 1] - d[far, 1]) > 0.05  # the sky reads y: the two rays' backgrounds differ
        assert moved.sum() >= 200
    else:
        lit = (last["end"] == O.PATH_END_ABSORBED) & (counts >= 2) & (last["front_face"] == 0) & (last["e"] > 0).any(axis=1)
        assert lit.sum() >= 200
    assert (vertices[counts >= 3, 2]["hit"] == 1).sum() >= 200  # black at max_depth 3, not at 6: `depth <= 1` cuts them


@pytest.mark.parametrize("name, copy", BOTH, ids=IDS)
def test_one_bounce(name, copy):
    """Legs d and e on the oracle: the constants the device is held to in tests/test_gpu_path.py."""
    depth = Pc.BOUNCE_DEPTH[copy]
    got = Pc.oracle_query_samples(name, copy, depth)
    assert 1500 <= len(got) <= 2 * Pc.QUERY_RAYS
    worst, left = Pc.compare_one_bounce(name, copy, got, f"{name} {copy}, max_depth {depth}")
    pred = Pc.one_bounce(name, copy)
    m = pred["compared"]
    nonzero = (pred["colour"][m] != 0).any(axis=1)
    print(f"{name} {copy}: {len(got)} query rays x {Pc.QUERY_SAMPLES}, left out {100 * left:.2f} %, worst (U S) {worst:.3f}, "
          f"non-zero {100 * nonzero.mean():.1f} %, NaN {int(np.isnan(pred['colour'][m]).any(axis=1).sum())}")
    assert left <= Pc.MAX_LEFT_OUT, f"{name} {copy}, leg d: {100 * left:.2f} % of the samples left out"
    assert 0.05 <= nonzero.mean() <= 0.95  # both outcomes of the scattered ray are there
    # the samples of a ray are samples: fresh streams give other draws (where there is a draw: glass tosses one coin
    # at most, a ray that ends on the detector or the sky none, and the sky's value does not depend on the direction)
    assert (got[:, 0] != got[:, 1]).any(axis=1).mean() > 0.02


def test_an_isotropic_hit_is_refused(worlds):
    from tests import first_hit_worlds as FW

    with pytest.raises(ValueError, match="volume"):
        P.step(worlds("cornell_box_smoke"), np.zeros((1, 3)), np.ones((1, 3)), np.zeros(1), np.ones((1, 2), np.uint64), 6,
               np.ones((1, 3)))
    assert FW.N.MAT_ISOTROPIC not in {PW.world(n, c).raw.materials[i].kind for n, c in BOTH
                                      for i in range(PW.world(n, c).raw.material_count)}
