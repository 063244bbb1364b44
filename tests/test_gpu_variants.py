"""Every render-kernel variant and every LDS / HBM table placement against the oracle, bit for bit.

launch_render dispatches the product megakernel to fns[wp][tx][lk][mode] (60 kernels) or fns_gen[tx][lk - 3]
[mode - 1] (8 GEN kernels), and puts five blocks of device data (shading tables, texture table, proof boxes,
generic leaf tables, the shared drain's mailbox) in LDS or leaves them in HBM / L2.  The demo worlds reach few of
those cells.  Here ten small worlds (tests/variant_worlds.py, checked on the CPU by tests/test_variant_worlds.py),
one for each native (leaf kinds, texture kinds) pair, are steered through every reachable cell with the audit
knobs; each cell asserts the exact kernel name, then where the tables went (rtw_world_last_launch_lds), then the
oracle's bits.  Worlds of a chosen size take the fallbacks with no knob set.  No tolerances anywhere.

The camera-batch and leaf-list kernels (render_kernel_pl) have their own tests: RTW_PRIMARY_LISTS=0 here."""
import contextlib

import pytest

import raytracinginaweekend_amd as R
from oracle import pyoracle as O
from tests import variant_worlds as V
from tests.parity import assert_bit_identical

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT, SPP, DEPTH, SEED = 160, 90, 4, 50, 17  # 57 600 samples: 57 blocks of 1024 lanes

KNOBS = ("RTW_LDS_MODE", "RTW_WHOLE_PIXEL", "RTW_NO_GEN_LDS", "RTW_NO_SHADE_LDS", "RTW_NO_PROOF_LDS",
         "RTW_NO_COOP_SHARE", "RTW_NO_SAH", "RTW_LEAF_KINDS", "RTW_TEX_KINDS", "RTW_TRACE_MIN", "RTW_NO_REORDER",
         "RTW_COOP_MAX", "RTW_COOP_TIES", "RTW_MB_CAP", "RTW_NO_MARKSTEIN", "RTW_CHUNK", "RTW_TUNE_SPHERES")

# world -> (LDS mode, whole-pixel items, generic tables in LDS, the kernel's name)
CELLS = {
    "spheres-solid": [
        (0, 0, False, "render_kernel<false, 0, 0, 0, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 0, 0, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 0, 0, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 0, 0, false, true>"),
    ],
    "spheres-textured": [
        (0, 0, False, "render_kernel<false, 0, 0, 1, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 0, 1, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 0, 1, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 0, 1, false, true>"),
    ],
    "tris-solid": [
        (0, 0, False, "render_kernel<false, 0, 1, 0, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 1, 0, false, false>"),
        (2, 0, False, "render_kernel<false, 2, 1, 0, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 1, 0, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 1, 0, false, true>"),
        (2, 1, False, "render_kernel<false, 2, 1, 0, false, true>"),
    ],
    "tris-textured": [
        (0, 0, False, "render_kernel<false, 0, 1, 1, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 1, 1, false, false>"),
        (2, 0, False, "render_kernel<false, 2, 1, 1, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 1, 1, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 1, 1, false, true>"),
        (2, 1, False, "render_kernel<false, 2, 1, 1, false, true>"),
    ],
    "plain-solid": [
        (0, 0, False, "render_kernel<false, 0, 2, 0, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 2, 0, false, false>"),
        (2, 0, False, "render_kernel<false, 2, 2, 0, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 2, 0, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 2, 0, false, true>"),
        (2, 1, False, "render_kernel<false, 2, 2, 0, false, true>"),
    ],
    "plain-textured": [
        (0, 0, False, "render_kernel<false, 0, 2, 1, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 2, 1, false, false>"),
        (2, 0, False, "render_kernel<false, 2, 2, 1, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 2, 1, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 2, 1, false, true>"),
        (2, 1, False, "render_kernel<false, 2, 2, 1, false, true>"),
    ],
    "wrapped-solid": [
        (0, 0, False, "render_kernel<false, 0, 3, 0, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 3, 0, false, false>"),
        (2, 0, False, "render_kernel<false, 2, 3, 0, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 3, 0, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 3, 0, false, true>"),
        (2, 1, False, "render_kernel<false, 2, 3, 0, false, true>"),
        (1, 0, True, "render_kernel<false, 1, 3, 0, true, false>"),
        (2, 0, True, "render_kernel<false, 2, 3, 0, true, false>"),
        (1, 1, True, "render_kernel<false, 1, 3, 0, true, false>"),
        (2, 1, True, "render_kernel<false, 2, 3, 0, true, false>"),
    ],
    "wrapped-textured": [
        (0, 0, False, "render_kernel<false, 0, 3, 1, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 3, 1, false, false>"),
        (2, 0, False, "render_kernel<false, 2, 3, 1, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 3, 1, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 3, 1, false, true>"),
        (2, 1, False, "render_kernel<false, 2, 3, 1, false, true>"),
        (1, 0, True, "render_kernel<false, 1, 3, 1, true, false>"),
        (2, 0, True, "render_kernel<false, 2, 3, 1, true, false>"),
        (1, 1, True, "render_kernel<false, 1, 3, 1, true, false>"),
        (2, 1, True, "render_kernel<false, 2, 3, 1, true, false>"),
    ],
    "any-solid": [
        (0, 0, False, "render_kernel<false, 0, 4, 0, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 4, 0, false, false>"),
        (2, 0, False, "render_kernel<false, 2, 4, 0, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 4, 0, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 4, 0, false, true>"),
        (2, 1, False, "render_kernel<false, 2, 4, 0, false, true>"),
        (1, 0, True, "render_kernel<false, 1, 4, 0, true, false>"),
        (2, 0, True, "render_kernel<false, 2, 4, 0, true, false>"),
        (1, 1, True, "render_kernel<false, 1, 4, 0, true, false>"),
        (2, 1, True, "render_kernel<false, 2, 4, 0, true, false>"),
    ],
    "any-textured": [
        (0, 0, False, "render_kernel<false, 0, 4, 1, false, false>"),
        (1, 0, False, "render_kernel<false, 1, 4, 1, false, false>"),
        (2, 0, False, "render_kernel<false, 2, 4, 1, false, false>"),
        (0, 1, False, "render_kernel<false, 0, 4, 1, false, true>"),
        (1, 1, False, "render_kernel<false, 1, 4, 1, false, true>"),
        (2, 1, False, "render_kernel<false, 2, 4, 1, false, true>"),
        (1, 0, True, "render_kernel<false, 1, 4, 1, true, false>"),
        (2, 0, True, "render_kernel<false, 2, 4, 1, true, false>"),
        (1, 1, True, "render_kernel<false, 1, 4, 1, true, false>"),
        (2, 1, True, "render_kernel<false, 2, 4, 1, true, false>"),
    ],
}

# world -> (knob, the leaf kinds and texture kinds the launch then runs, the kernel's name in the world's default
# mode: 1 without triangles, else 2; leaf kinds 3 and 4 of these small worlds take the GEN kernels)
FORCED = {
    "spheres-solid": [
        ({"RTW_LEAF_KINDS": "1"}, 1, 0, "render_kernel<false, 1, 1, 0, false, false>"),
        ({"RTW_LEAF_KINDS": "2"}, 2, 0, "render_kernel<false, 1, 2, 0, false, false>"),
        ({"RTW_LEAF_KINDS": "3"}, 3, 0, "render_kernel<false, 1, 3, 0, true, false>"),
        ({"RTW_LEAF_KINDS": "4"}, 4, 0, "render_kernel<false, 1, 4, 0, true, false>"),
        ({"RTW_TEX_KINDS": "1"}, 0, 1, "render_kernel<false, 1, 0, 1, false, false>"),
    ],
    "spheres-textured": [
        ({"RTW_LEAF_KINDS": "1"}, 1, 1, "render_kernel<false, 1, 1, 1, false, false>"),
        ({"RTW_LEAF_KINDS": "2"}, 2, 1, "render_kernel<false, 1, 2, 1, false, false>"),
        ({"RTW_LEAF_KINDS": "3"}, 3, 1, "render_kernel<false, 1, 3, 1, true, false>"),
        ({"RTW_LEAF_KINDS": "4"}, 4, 1, "render_kernel<false, 1, 4, 1, true, false>"),
    ],
    "tris-solid": [
        ({"RTW_LEAF_KINDS": "2"}, 2, 0, "render_kernel<false, 2, 2, 0, false, false>"),
        ({"RTW_LEAF_KINDS": "3"}, 3, 0, "render_kernel<false, 2, 3, 0, true, false>"),
        ({"RTW_LEAF_KINDS": "4"}, 4, 0, "render_kernel<false, 2, 4, 0, true, false>"),
        ({"RTW_TEX_KINDS": "1"}, 1, 1, "render_kernel<false, 2, 1, 1, false, false>"),
    ],
    "tris-textured": [
        ({"RTW_LEAF_KINDS": "2"}, 2, 1, "render_kernel<false, 2, 2, 1, false, false>"),
        ({"RTW_LEAF_KINDS": "3"}, 3, 1, "render_kernel<false, 2, 3, 1, true, false>"),
        ({"RTW_LEAF_KINDS": "4"}, 4, 1, "render_kernel<false, 2, 4, 1, true, false>"),
    ],
    "plain-solid": [
        ({"RTW_LEAF_KINDS": "3"}, 3, 0, "render_kernel<false, 2, 3, 0, true, false>"),
        ({"RTW_LEAF_KINDS": "4"}, 4, 0, "render_kernel<false, 2, 4, 0, true, false>"),
        ({"RTW_TEX_KINDS": "1"}, 2, 1, "render_kernel<false, 2, 2, 1, false, false>"),
    ],
    "plain-textured": [
        ({"RTW_LEAF_KINDS": "3"}, 3, 1, "render_kernel<false, 2, 3, 1, true, false>"),
        ({"RTW_LEAF_KINDS": "4"}, 4, 1, "render_kernel<false, 2, 4, 1, true, false>"),
    ],
    "wrapped-solid": [
        ({"RTW_LEAF_KINDS": "4"}, 4, 0, "render_kernel<false, 2, 4, 0, true, false>"),
        ({"RTW_TEX_KINDS": "1"}, 3, 1, "render_kernel<false, 2, 3, 1, true, false>"),
    ],
    "wrapped-textured": [
        ({"RTW_LEAF_KINDS": "4"}, 4, 1, "render_kernel<false, 2, 4, 1, true, false>"),
    ],
    "any-solid": [
        ({"RTW_TEX_KINDS": "1"}, 4, 1, "render_kernel<false, 2, 4, 1, true, false>"),
    ],
    "any-textured": [],
}

# launch_render's dispatch table, fns[wp][tx][lk][mode]: render_kernel<STATS, LDS, LK, TX, GEN, WP> ...
NON_GEN_NAMES = {
    "render_kernel<false, 0, 0, 0, false, false>", "render_kernel<false, 1, 0, 0, false, false>",
    "render_kernel<false, 2, 0, 0, false, false>",
    "render_kernel<false, 0, 1, 0, false, false>", "render_kernel<false, 1, 1, 0, false, false>",
    "render_kernel<false, 2, 1, 0, false, false>",
    "render_kernel<false, 0, 2, 0, false, false>", "render_kernel<false, 1, 2, 0, false, false>",
    "render_kernel<false, 2, 2, 0, false, false>",
    "render_kernel<false, 0, 3, 0, false, false>", "render_kernel<false, 1, 3, 0, false, false>",
    "render_kernel<false, 2, 3, 0, false, false>",
    "render_kernel<false, 0, 4, 0, false, false>", "render_kernel<false, 1, 4, 0, false, false>",
    "render_kernel<false, 2, 4, 0, false, false>",
    "render_kernel<false, 0, 0, 1, false, false>", "render_kernel<false, 1, 0, 1, false, false>",
    "render_kernel<false, 2, 0, 1, false, false>",
    "render_kernel<false, 0, 1, 1, false, false>", "render_kernel<false, 1, 1, 1, false, false>",
    "render_kernel<false, 2, 1, 1, false, false>",
    "render_kernel<false, 0, 2, 1, false, false>", "render_kernel<false, 1, 2, 1, false, false>",
    "render_kernel<false, 2, 2, 1, false, false>",
    "render_kernel<false, 0, 3, 1, false, false>", "render_kernel<false, 1, 3, 1, false, false>",
    "render_kernel<false, 2, 3, 1, false, false>",
    "render_kernel<false, 0, 4, 1, false, false>", "render_kernel<false, 1, 4, 1, false, false>",
    "render_kernel<false, 2, 4, 1, false, false>",
    "render_kernel<false, 0, 0, 0, false, true>", "render_kernel<false, 1, 0, 0, false, true>",
    "render_kernel<false, 2, 0, 0, false, true>",
    "render_kernel<false, 0, 1, 0, false, true>", "render_kernel<false, 1, 1, 0, false, true>",
    "render_kernel<false, 2, 1, 0, false, true>",
    "render_kernel<false, 0, 2, 0, false, true>", "render_kernel<false, 1, 2, 0, false, true>",
    "render_kernel<false, 2, 2, 0, false, true>",
    "render_kernel<false, 0, 3, 0, false, true>", "render_kernel<false, 1, 3, 0, false, true>",
    "render_kernel<false, 2, 3, 0, false, true>",
    "render_kernel<false, 0, 4, 0, false, true>", "render_kernel<false, 1, 4, 0, false, true>",
    "render_kernel<false, 2, 4, 0, false, true>",
    "render_kernel<false, 0, 0, 1, false, true>", "render_kernel<false, 1, 0, 1, false, true>",
    "render_kernel<false, 2, 0, 1, false, true>",
    "render_kernel<false, 0, 1, 1, false, true>", "render_kernel<false, 1, 1, 1, false, true>",
    "render_kernel<false, 2, 1, 1, false, true>",
    "render_kernel<false, 0, 2, 1, false, true>", "render_kernel<false, 1, 2, 1, false, true>",
    "render_kernel<false, 2, 2, 1, false, true>",
    "render_kernel<false, 0, 3, 1, false, true>", "render_kernel<false, 1, 3, 1, false, true>",
    "render_kernel<false, 2, 3, 1, false, true>",
    "render_kernel<false, 0, 4, 1, false, true>", "render_kernel<false, 1, 4, 1, false, true>",
    "render_kernel<false, 2, 4, 1, false, true>",
}
# ... and fns_gen[tx][lk - 3][mode - 1] (whole-pixel items are a run-time choice inside them)
GEN_NAMES = {
    "render_kernel<false, 1, 3, 0, true, false>", "render_kernel<false, 2, 3, 0, true, false>",
    "render_kernel<false, 1, 4, 0, true, false>", "render_kernel<false, 2, 4, 0, true, false>",
    "render_kernel<false, 1, 3, 1, true, false>", "render_kernel<false, 2, 3, 1, true, false>",
    "render_kernel<false, 1, 4, 1, true, false>", "render_kernel<false, 2, 4, 1, true, false>",
}
# Instantiated, never launched: LDS mode 2 holds the triangle records, and launch_render takes it only with
# g->tri_count > 0.  A world with a triangle has a leaf of class LK_TRIS or above (a triangle leaf is LK_TRIS when
# plain, LK_WRAPPED or LK_ANY when wrapped), and RTW_LEAF_KINDS only raises lk, so lk == LK_SPHERES never meets
# mode 2.  (A plain-sphere world beyond 2^14 leaves is promoted to LK_TRIS at upload: lk 1, not 0.)
UNREACHABLE = {
    "render_kernel<false, 2, 0, 0, false, false>", "render_kernel<false, 2, 0, 1, false, false>",
    "render_kernel<false, 2, 0, 0, false, true>", "render_kernel<false, 2, 0, 1, false, true>",
}

SEEN = set()  # the kernel names test_matrix_cell's cells launched (asserted, with bits) in this session


@pytest.fixture(autouse=True)
def _knobs_off(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RTW_PRIMARY_LISTS", "0")  # the plain render_kernel cells, not render_kernel_pl


@pytest.fixture(scope="module")
def variants():
    """pair -> (world, oracle frame), one oracle frame per world for the whole module."""
    cache = {}

    def get(pair):
        if pair not in cache:
            world = V.variant_world(*pair)
            ref = O.render(world, R.render_params(R.Size2i(WIDTH, HEIGHT), SPP, DEPTH, seed=SEED))
            ref.setflags(write=False)
            cache[pair] = (world, ref)
        return cache[pair]

    return get


def _render(world, env: dict, monkeypatch, size=(WIDTH, HEIGHT), spp=SPP, seed=SEED, frames=1):
    """`frames` frames of a fresh DeviceWorld under the knobs `env`: (images, kernel_variant(), last_frame())."""
    import torch

    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        dw = R.DeviceWorld(world, 0)  # (the upload reads RTW_NO_SAH)
        p = R.render_params(R.Size2i(*size), spp, DEPTH, seed=seed)
        images = []
        for _ in range(frames):
            out = torch.empty(size[0] * size[1] * 3, dtype=torch.float32, device="cuda:0")
            dw.render_into(p, out.data_ptr(), 0)
            torch.cuda.synchronize()
            images.append(out.cpu().numpy().reshape(-1, 3))
        v, lf = dw.kernel_variant(), dw.last_frame()
        dw.release()
    return images, v, lf


FLAGS = ("shade_lds", "tex_lds", "proof_lds", "gen_lds", "mailbox", "tri_prefix", "sah")


def _intended(world, native_lk: int, lk: int, tx: int, mode: int, env: dict) -> dict:
    """Where a launch of one of the small worlds (every table fits the LDS) is meant to put its tables: the cell's
    intention, from launch_render's rules and the knobs, never from the launch's reply."""
    on = lambda k: env.get(k, "0") != "0"  # noqa: E731
    # the SAH walk: not the LK_ANY loop, and a plain-sphere world's folded records serve the LK_SPHERES loop only
    sah = not on("RTW_NO_SAH") and lk <= V.LK_WRAPPED and (native_lk == V.LK_SPHERES) == (lk == V.LK_SPHERES)
    shade = mode >= 1 and not on("RTW_NO_SHADE_LDS")
    gen_wanted = lk >= V.LK_WRAPPED and not on("RTW_NO_GEN_LDS")
    return {
        "shade_lds": int(shade),
        # (a launch that wants a GEN kernel with non-solid textures keeps the texture table out: those kernels
        # compile no LDS texture path)
        "tex_lds": int(shade and not (gen_wanted and tx == V.TX_ANY)),
        "proof_lds": int(shade and sah and not on("RTW_NO_PROOF_LDS")),
        "gen_lds": int(shade and gen_wanted),
        "mailbox": int(mode >= 1 and sah and lk == V.LK_TRIS and not on("RTW_NO_COOP_SHARE")),
        "tri_prefix": V.tri_prefix(world) if lk == V.LK_TRIS else 0,
        "sah": int(sah),
    }


@contextlib.contextmanager
def _cell(failed: list, tag: str):
    """One cell of a test's loop: a failed assertion is noted and the loop goes on, so that a test reports every
    cell that disagrees (an error of the library, a HIP fault among them, still ends the test at once)."""
    try:
        yield
    except AssertionError as e:
        failed.append(f"{tag}: {e}"[:600])


def _check(v: dict, name: str, want: dict, tag: str):
    assert v["name"] == name, (tag, v)
    assert {k: v[k] for k in FLAGS} == want, (tag, v)
    assert v["tree"] == ("sah" if want["sah"] else "reference"), (tag, v)
    assert 0 < v["lds_bytes"] <= 160 * 1024, (tag, v)


@pytest.mark.parametrize("pair", V.PAIRS, ids=V.pair_id)
def test_matrix_cell(pair, variants, monkeypatch):
    """Every reachable cell of the world's (lk, tx): LDS modes {0, 1} (and 2 with triangles) x both item kinds of
    the non-GEN kernels (RTW_NO_GEN_LDS=1 where lk >= 3), modes {1, 2} x both item kinds of the GEN kernels."""
    world, ref = variants(pair)
    lk, tx = pair
    failed = []
    for mode, wp, gen, name in CELLS[V.pair_id(pair)]:
        env = {"RTW_LDS_MODE": str(mode), "RTW_WHOLE_PIXEL": str(wp)}
        if lk >= V.LK_WRAPPED and not gen:
            env["RTW_NO_GEN_LDS"] = "1"
        tag = f"{V.pair_id(pair)} mode {mode} wp {wp} gen {gen}"
        with _cell(failed, tag):
            (img,), v, lf = _render(world, env, monkeypatch)
            want = _intended(world, lk, lk, tx, mode, env)
            assert want["gen_lds"] == int(gen)
            _check(v, name, want, tag)
            assert v["lds_mode"] == mode and lf["whole_pixel"] == bool(wp), (tag, v, lf)
            assert_bit_identical(img, ref, tag)
            SEEN.add(name)
    assert not failed, "\n".join(failed)


def test_matrix_covers_the_dispatch_table():
    """The names the matrix launched (this session's test_matrix_cell runs, above in this file) and the four
    unreachable cells are the whole dispatch table, 60 + 8 names written out."""
    assert len(NON_GEN_NAMES) == 60 and len(GEN_NAMES) == 8 and len(UNREACHABLE) == 4
    assert UNREACHABLE <= NON_GEN_NAMES and not (SEEN & UNREACHABLE)
    table = {name for cells in CELLS.values() for *_, name in cells}
    assert table | UNREACHABLE == NON_GEN_NAMES | GEN_NAMES
    assert SEEN | UNREACHABLE == NON_GEN_NAMES | GEN_NAMES, sorted((NON_GEN_NAMES | GEN_NAMES) - SEEN - UNREACHABLE)


@pytest.mark.parametrize("pair", [p for p in V.PAIRS if FORCED[V.pair_id(p)]], ids=V.pair_id)
def test_generic_code_on_specialised_worlds(pair, variants, monkeypatch):
    """RTW_LEAF_KINDS above the world's own and RTW_TEX_KINDS=1 on a solid-texture world: the more generic loop
    and texture code give the oracle's bits on a world that would not select them."""
    world, ref = variants(pair)
    mode = 1 if pair[0] == V.LK_SPHERES else 2
    failed = []
    for env, lk, tx, name in FORCED[V.pair_id(pair)]:
        tag = f"{V.pair_id(pair)} {env}"
        with _cell(failed, tag):
            (img,), v, _ = _render(world, env, monkeypatch)
            _check(v, name, _intended(world, pair[0], lk, tx, mode, env), tag)
            assert_bit_identical(img, ref, tag)
    assert not failed, "\n".join(failed)


def _name(mode: int, lk: int, tx: int, gen: int) -> str:
    return f"render_kernel<false, {mode}, {lk}, {tx}, {'true' if gen else 'false'}, false>"


@pytest.mark.parametrize("pair", V.PAIRS, ids=V.pair_id)
def test_table_placement(pair, variants, monkeypatch):
    """Each table out of LDS on its own, all of them together, and the reference tree (RTW_NO_SAH=1) in modes 0
    and 1: only the intended flags move (a table that sits behind another one leaves with it: without the
    shading tables nothing else is staged, and the launch takes the non-GEN kernel), the LDS allocation shrinks,
    and the bits stay the oracle's.  The prefix world with its tables out reads leaf_info from HBM behind the
    made-up prefix records (leaf_info_of)."""
    world, ref = variants(pair)
    lk, tx = pair
    mode = 1 if lk == V.LK_SPHERES else 2
    (img,), base, _ = _render(world, {}, monkeypatch)
    want0 = _intended(world, lk, lk, tx, mode, {})
    _check(base, _name(mode, lk, tx, want0["gen_lds"]), want0, "default")
    assert base["lds_mode"] == mode
    assert_bit_identical(img, ref, f"{V.pair_id(pair)} default")
    knobs = [{"RTW_NO_SHADE_LDS": "1"}]
    if lk <= V.LK_WRAPPED:
        knobs.append({"RTW_NO_PROOF_LDS": "1"})
    if lk >= V.LK_WRAPPED:
        knobs.append({"RTW_NO_GEN_LDS": "1"})
    if lk == V.LK_TRIS:
        knobs.append({"RTW_NO_COOP_SHARE": "1"})
    knobs.append({k: "1" for k in ("RTW_NO_SHADE_LDS", "RTW_NO_PROOF_LDS", "RTW_NO_GEN_LDS", "RTW_NO_COOP_SHARE")})
    failed = []
    for env in knobs:
        tag = f"{V.pair_id(pair)} {sorted(env)}"
        with _cell(failed, tag):
            (img,), v, _ = _render(world, env, monkeypatch)
            want = _intended(world, lk, lk, tx, mode, env)
            assert want != want0, tag  # the knob is meant to move something in this world
            _check(v, _name(mode, lk, tx, want["gen_lds"]), want, tag)
            assert v["lds_mode"] == mode and v["lds_bytes"] < base["lds_bytes"], (tag, v, base)
            assert_bit_identical(img, ref, tag)
    for m in (0, 1):
        env = {"RTW_NO_SAH": "1", "RTW_LDS_MODE": str(m)}
        tag = f"{V.pair_id(pair)} reference tree, mode {m}"
        with _cell(failed, tag):
            (img,), v, _ = _render(world, env, monkeypatch)
            want = _intended(world, lk, lk, tx, m, env)
            _check(v, _name(m, lk, tx, want["gen_lds"]), want, tag)
            assert v["lds_mode"] == m and want["sah"] == 0 and want["proof_lds"] == 0
            assert_bit_identical(img, ref, tag)
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------------
# natural overflows: the fallbacks a caller's larger scene selects, no knob set
# ------------------------------------------------------------------------------------------------
SMALL = (40, 24)


def _probe(world, monkeypatch) -> dict:
    return _render(world, {}, monkeypatch, size=(16, 16), spp=1)[1]


def _small_frame(world, monkeypatch) -> tuple:
    """(kernel_variant(), the GPU's 40 x 24 x 4 frame, the oracle's) with no knob set."""
    (img,), v, _ = _render(world, {}, monkeypatch, size=SMALL, seed=13)
    return v, img, O.render(world, R.render_params(R.Size2i(*SMALL), SPP, DEPTH, seed=13))


def test_soup_too_large_for_lds_runs_mode0(monkeypatch):
    """big_soup(2377): 2378 leaves (ground sphere first: no triangle prefix), a SAH tree of N nodes and depth 15.
    launch_render's scene_bytes = 16 (2 N + L + (N + 1) / 2) and mode 1's 16-bit stack of 15 x 1024 x 2 = 30 720 B
    must fit 160 KiB = 163 840 B: at 2376 triangles they take 163 792 B, one triangle more does not fit (and mode
    2 adds 64 B per triangle), so the scene stays in HBM / L2 with a 15 x 1024 x 4 = 61 440 B stack: LDS mode 0
    on the SAH tree.  2378 leaves are below RTW_COOP_LEAVES, so the cooperative trace stays on."""
    v = _probe(V.big_soup(2376), monkeypatch)
    assert v["lds_mode"] == 1 and v["shade_lds"] == 0 and v["lds_bytes"] == 163792, v
    world = V.big_soup(2377)
    v, img, ref = _small_frame(world, monkeypatch)
    assert v["name"] == "render_kernel<false, 0, 1, 0, false, false>", v
    assert {k: v[k] for k in FLAGS} == dict(shade_lds=0, tex_lds=0, proof_lds=0, gen_lds=0, mailbox=0, tri_prefix=0, sah=1), v
    assert v["lds_bytes"] == 61440, v
    assert_bit_identical(img, ref, "soup 2377, mode 0")


def test_wrapped_too_large_for_lds_runs_mode0(monkeypatch):
    """big_wrapped(2377), by the same arithmetic as the soup (56 B of scene per leaf and node): mode 0, where no
    GEN kernel exists -- the product route to the non-GEN LK_WRAPPED kernel, every table read from HBM / L2."""
    v = _probe(V.big_wrapped(2376), monkeypatch)
    assert v["lds_mode"] == 1 and v["shade_lds"] == 0 and v["gen_lds"] == 0, v
    world = V.big_wrapped(2377)
    v, img, ref = _small_frame(world, monkeypatch)
    assert v["name"] == "render_kernel<false, 0, 3, 0, false, false>", v
    assert {k: v[k] for k in FLAGS} == dict(shade_lds=0, tex_lds=0, proof_lds=0, gen_lds=0, mailbox=0, tri_prefix=0, sah=1), v
    assert_bit_identical(img, ref, "wrapped 2377, mode 0")


@pytest.mark.parametrize("textured", [False, True], ids=["solid", "textured"])
def test_wrapped_generic_tables_overflow_in_mode1(textured, monkeypatch):
    """big_wrapped(782), the smallest n whose generic tables stay out while the shading tables are in: L = 783
    leaves, 392 spheres, 391 boxes.  Scene, stack (15 x 1024 x 2 B), shading tables (16 B x (L + materials +
    textures)) and proof boxes (32 B x L) take 108 128 B; the gen_bytes line asks 16 (3 L + spheres + 2 boxes) =
    16 x 3523 = 56 368 B more: 164 496 B > 163 840 B.  At n = 781 (16 x 3519 = 56 304 B) the launch fits in
    162 288 B and takes the GEN kernel.  So 782 runs the non-GEN LK_WRAPPED kernel in mode 1 with the transforms,
    spheres and boxes read from HBM / L2 and everything else in LDS.
    textured: the same world with image textures.  A launch that wants a GEN kernel with non-solid textures keeps
    the texture table out of LDS (16 B less); when the generic tables then do not fit, the non-GEN kernel runs
    with its textures in HBM / L2 as well (final_scene2's placement, here on the LK_WRAPPED kernel)."""
    tx = int(textured)
    v = _probe(V.big_wrapped(781, textured=textured), monkeypatch)
    assert v["name"] == f"render_kernel<false, 1, 3, {tx}, true, false>" and v["gen_lds"] == 1, v
    assert v["lds_bytes"] == 162288 - 16 * tx, v
    world = V.big_wrapped(782, textured=textured)
    v, img, ref = _small_frame(world, monkeypatch)
    assert v["name"] == f"render_kernel<false, 1, 3, {tx}, false, false>", v
    assert {k: v[k] for k in FLAGS} == dict(shade_lds=1, tex_lds=1 - tx, proof_lds=1, gen_lds=0, mailbox=0, tri_prefix=0,
                                            sah=1), v
    assert v["lds_bytes"] == 108128 - 16 * tx, v
    assert_bit_identical(img, ref, "wrapped 782, mode 1, generic tables in HBM")


def test_textured_soup_falls_back_to_mode1(monkeypatch):
    """big_soup(n, textured): the image-textured mesh comes first, so all n triangles are the prefix, whose leaf
    records and leaf_info the kernel makes up.  Mode 2 needs the triangle records (64 B each) beside the scene,
    the 16-bit stack and the mailbox: 1286 triangles still fit (without the shading tables), 1287 do not, and the
    launch falls back to mode 1 -- the textured LK_TRIS mode-1 kernel -- with every table and the mailbox in
    LDS."""
    v = _probe(V.big_soup(1286, textured=True), monkeypatch)
    assert v["lds_mode"] == 2 and v["tri_prefix"] == 1286 and v["shade_lds"] == 0, v
    world = V.big_soup(1287, textured=True)
    v, img, ref = _small_frame(world, monkeypatch)
    assert v["name"] == "render_kernel<false, 1, 1, 1, false, false>", v
    assert {k: v[k] for k in FLAGS} == dict(shade_lds=1, tex_lds=1, proof_lds=1, gen_lds=0, mailbox=1, tri_prefix=1287, sah=1), v
    assert_bit_identical(img, ref, "textured soup 1287, mode 1")


def test_textured_soup_mode2_without_shading_tables(monkeypatch):
    """The size just below: 1286 textured triangles in mode 2 whose shading tables no longer fit, so the made-up
    prefix records meet leaf_info, materials and the texture table in HBM / L2 with no knob set."""
    world = V.big_soup(1286, textured=True)
    v, img, ref = _small_frame(world, monkeypatch)
    assert v["name"] == "render_kernel<false, 2, 1, 1, false, false>", v
    assert {k: v[k] for k in FLAGS} == dict(shade_lds=0, tex_lds=0, proof_lds=0, gen_lds=0, mailbox=1, tri_prefix=1286, sah=1), v
    assert_bit_identical(img, ref, "textured soup 1286, mode 2, shading tables in HBM")


# ------------------------------------------------------------------------------------------------
# scheduling knobs: they move work between lanes and frames, never bits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(V.LK_SPHERES, V.TX_ANY), (V.LK_PLAIN, V.TX_SOLID)], ids=V.pair_id)
def test_scheduling_knobs_keep_bits(pair, variants, monkeypatch):
    """RTW_TRACE_MIN in {1, 8, 64} (the dynamic-fetch threshold, compared with a 64-lane popcount: 1 never
    leaves the walk early, 64 leaves whenever a lane waits) and RTW_NO_REORDER=1 (chunk-major order) against two
    successive frames of one resident world without it (the second in learned cost order): the oracle's bits
    every time, and last_frame() reports the forced threshold."""
    world, ref = variants(pair)
    for tm in (1, 8, 64):
        (img,), _, lf = _render(world, {"RTW_TRACE_MIN": str(tm)}, monkeypatch)
        assert lf["trace_min"] == tm, lf
        assert_bit_identical(img, ref, f"{V.pair_id(pair)} RTW_TRACE_MIN={tm}")
    (first, second), _, _ = _render(world, {}, monkeypatch, frames=2)
    assert_bit_identical(first, ref, f"{V.pair_id(pair)} first frame")
    assert_bit_identical(second, ref, f"{V.pair_id(pair)} second frame, cost order")
    (a, b), _, _ = _render(world, {"RTW_NO_REORDER": "1"}, monkeypatch, frames=2)
    assert_bit_identical(a, ref, f"{V.pair_id(pair)} RTW_NO_REORDER=1")
    assert_bit_identical(b, ref, f"{V.pair_id(pair)} RTW_NO_REORDER=1, second frame")
