"""rtw_world_check (csrc/rtw_check.cpp, contract in include/rtw.h): the validator between a caller's flat rtw_world
and every table read of the upload, the kernel and the oracle.  CPU only.

Every builder world is accepted unchanged with its tree's depth; every mutant below is a deep copy of a builder
world (tests/world_copy.py) with one field wrong, and must be refused with the code and a message that names
the table and the field.  The list follows the structs of rtw.h (rtw_bvh_node .. rtw_world) field by field.

Decided for refusal, because the reference cannot express them (its builder makes one binary tree over all the
leaves, rect planes are an enum, and a leaf's wrappers are the three flags):
  - a rect plane outside RTW_PLANE_* in rects[] or in the light (the device and the oracle would both read it as
    YZ, rect_axes, so they agree -- on a world nobody meant), and a light whose ranges are empty (the reference
    samples it with gen_range, which panics);
  - leaf flag bits above RTW_LEAF_ANIMATION (`flags == 0` selects the plain-sphere record);
  - a leaf or a node that the tree references twice or never (the per-tile leaf lists are built from the leaf
    table, so camera rays could hit a leaf the reference's walk never reaches).

The stand-alone fuzz (tests/native/world_check_fuzz.c, built plain and with ASan + UBSan, nothing preloaded) then
throws seeded one- and two-field mutations at the validator and, for every mutant it accepts, renders an 8 x 8
frame at 2 spp, depth 8 with the oracle.  The oracle indexes the same tables with the same indices as the kernel,
so a clean sanitized run is a proxy -- not a proof -- for "accepted => every device read is in bounds".  The host
sources need only `g++ -I<rocm>/include -D__HIP_PLATFORM_AMD__` (rtw_common.h includes hip_runtime_api.h for
declarations that rtw_check.cpp, scene_builder.cpp and demo_worlds.cpp never call)."""
import ctypes as C
import math
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from raytracinginaweekend_amd import _native as N
from raytracinginaweekend_amd.world import check_world
from tests import variant_worlds as V
from tests.world_copy import COUNTS, TABLES, OwnedWorld, add_chain, chain_world, row_world, tree_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = N.RTW_ERR_INVALID_ARGUMENT, N.RTW_ERR_UNSUPPORTED
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
WILD = 10 ** 6
MAX_DEPTH, MAX_CHAIN = 32, 64  # RTW_MAX_BVH_DEPTH, RTW_MAX_TEXTURE_CHAIN
DEMOS = ["final_scene1", "final_scene2", "cornell_box", "cornell_box_smoke", "cornell_cube", "suzanne", "earth_mapped",
         "earth_motion", "moving_spheres", "perlin_spheres", "simple_plane", "defocus_blur"]


def test_header_constants():
    text = open(os.path.join(ROOT, "include", "rtw.h")).read()
    assert int(re.search(r"#define RTW_MAX_BVH_DEPTH (\d+)", text).group(1)) == MAX_DEPTH
    assert int(re.search(r"#define RTW_MAX_TEXTURE_CHAIN (\d+)", text).group(1)) == MAX_CHAIN
    device = open(os.path.join(ROOT, "raytracinginaweekend_amd", "csrc", "rtw_device.hip")).read()
    assert int(re.search(r"#define RTW_STACK (\d+)", device).group(1)) == MAX_DEPTH
    assert f"guard < {MAX_CHAIN};" in device  # texture_sample's loop: one texture per step


# ---- accepted unchanged ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEMOS)
def test_demo_worlds_are_accepted(worlds, name):
    w = worlds(name)
    assert w.check() == tree_depth(w.raw)
    assert check_world(OwnedWorld(w).raw) == tree_depth(w.raw)  # the deep copy is the same world
    fp = [C.c_uint64(), C.c_uint64()]
    N.check(N.lib().rtw_world_fingerprint(w.ptr(), C.byref(fp[0])))
    N.check(N.lib().rtw_world_fingerprint(OwnedWorld(w).ptr(), C.byref(fp[1])))
    assert fp[0].value == fp[1].value


@pytest.mark.parametrize("pair", V.PAIRS, ids=V.pair_id)
def test_variant_worlds_are_accepted(pair):
    w = V.variant_world(*pair)
    assert w.check() == tree_depth(w.raw)


@pytest.mark.parametrize("make", [lambda: V.soup_world(40), lambda: V.soup_world(40, textured=True), lambda: V.sphere_cloud(50),
                                  lambda: V.big_wrapped(21), lambda: V.big_wrapped(21, textured=True)],
                         ids=["soup", "soup_textured", "cloud", "wrapped", "wrapped_textured"])
def test_sized_worlds_are_accepted(make):
    w = make()
    assert w.check() == tree_depth(w.raw)


def test_null_world_and_null_depth():
    assert N.lib().rtw_world_check(None, None) == INVALID
    assert N.lib().rtw_world_check(V.sphere_cloud(5).ptr(), None) == N.RTW_OK


# ---- the base of the mutants: every table in use -------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return V.variant_world(V.LK_ANY, V.TX_ANY)  # every geometry, wrapper, material and texture kind, a light


def first(raw, table, pred):
    return next(i for i in range(getattr(raw, COUNTS[table])) if pred(getattr(raw, table)[i]))


def refused(world, code, *names):
    depth = C.c_int32(-77)
    rc = N.lib().rtw_world_check(world.ptr(), C.byref(depth))
    msg = N.lib().rtw_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith("invalid world: "), msg
    for n in names:
        assert n in msg, (n, msg)
    assert depth.value == -77  # left alone


def accepted(world):
    return check_world(world.raw)


# One entry per field per fault: (id, mutation, code, what the message must name).  A mutation gets the OwnedWorld
# and may return the names itself (when the index is found in the world).
def m_set(table, index, field, value):
    def f(w):
        setattr(w.arrays[table][index(w.raw) if callable(index) else index], field, value)
    return f


def leaf_of_kind(kind):
    return lambda raw: first(raw, "leaves", lambda l: l.geom_kind == kind)


def tex_of_kind(kind):
    return lambda raw: first(raw, "textures", lambda t: t.kind == kind)


def mat_not(kind):
    return lambda raw: first(raw, "materials", lambda m: m.kind != kind)


def m_root(value):
    def f(w):
        w.raw.root = value(w.raw) if callable(value) else value
    return f


def m_self_reference(w):
    k = w.raw.root
    w.arrays["nodes"][k].left = k
    return [f"nodes[{k}].left"]


def m_node_twice(w):
    k = first(w.raw, "nodes", lambda n: n.left >= 0 and n.right >= 0)
    w.arrays["nodes"][k].right = w.arrays["nodes"][k].left
    return [f"nodes[{k}].right", "a second time"]


def m_cycle(w):
    raw = w.raw
    k = first(raw, "nodes", lambda n: n.left >= 0 and raw.nodes[n.left].left >= 0)
    child = raw.nodes[k].left
    w.arrays["nodes"][child].left = k  # grandchild edge back to k
    return [f"nodes[{child}].left", "a second time"]


def m_leaf_twice(w):
    raw = w.raw
    k = first(raw, "nodes", lambda n: n.left < 0 and n.right < 0)
    w.arrays["nodes"][k].right = raw.nodes[k].left
    return [f"nodes[{k}].right", "a second time"]


def m_leaf_by_no_node(w):
    n = w.raw.leaf_count
    leaves = w.resize("leaves", n + 1)
    C.memmove(C.byref(leaves[n]), C.byref(leaves[0]), C.sizeof(N.Leaf))
    return [f"leaves[{n}]", "no node"]


def m_node_by_no_node(w):
    n = w.raw.node_count
    nodes = w.resize("nodes", n + 1)
    C.memmove(C.byref(nodes[n]), C.byref(nodes[0]), C.sizeof(N.BvhNode))
    nodes[n].left = nodes[n].right = n  # (whatever it holds: nothing leads to it)
    return [f"nodes[{n}]", "no node"]


def m_root_is_a_leaf(w):
    w.raw.root = -1  # a valid leaf, but the other leaves and every node hang in the air
    return ["leaves[1]", "no node"]


def m_wild_texture(kind):
    def f(w):
        t = w.arrays["textures"][0]
        t.kind, t.perlin, t.image, t.even, t.odd = kind, WILD, WILD, WILD, WILD
        return ["textures[0].kind"]
    return f


def m_solid_with_wild_fields(w):
    i = tex_of_kind(N.TEX_SOLID)(w.raw)
    t = w.arrays["textures"][i]
    t.perlin, t.image, t.even, t.odd = WILD, -WILD, I32_MIN, I32_MAX


def m_checker_self(w):
    t0 = add_chain(w, 2, close_on=0)
    return [f"textures[{t0}].odd", "cycle"]


def m_checker_two_cycle(w):
    t0 = add_chain(w, 3, close_on=0)
    return [f"textures[{t0 + 1}].odd", "cycle"]


def m_chain_too_long(w):
    t0 = add_chain(w, MAX_CHAIN + 1)
    return [f"textures[{t0}]", "chain"]


def m_perlin(field, index, value, bits=None):
    def f(w):
        p = w.arrays["perlins"][0]
        if bits is not None:  # a smaller lattice: true permutations of 0 .. 2^bits - 1 in the entries that are read
            p.bits = bits
            for a in ("perm_x", "perm_y", "perm_z"):
                for k in range(256):
                    getattr(p, a)[k] %= 1 << bits
        idx = index(p) if callable(index) else index
        getattr(p, field)[idx] = value(p) if callable(value) else value
        return [f"perlins[0].{field}[{idx}]"]
    return f


def m_null(table):
    def f(w):
        setattr(w.raw, table, C.POINTER(dict((t, ty) for t, _, ty in TABLES)[table])())
    return f


def m_count(table, value):
    def f(w):
        setattr(w.raw, COUNTS[table], value)
    return f


def m_light(field, value):
    def f(w):
        assert w.raw.has_light == 1
        setattr(w.raw.light, field, value)
    return f


def m_light_never_filled(w):
    C.memset(C.byref(w.raw.light), 0, C.sizeof(N.Rect))
    w.raw.has_light = 1


REFUSALS = [
    # rtw_world.root
    ("root=node_count", m_root(lambda raw: raw.node_count), INVALID, ["root"]),
    ("root=~leaf_count", m_root(lambda raw: -1 - raw.leaf_count), INVALID, ["root"]),
    ("root=INT32_MIN", m_root(I32_MIN), INVALID, ["root"]),
    ("root=INT32_MAX", m_root(I32_MAX), INVALID, ["root"]),
    ("root=a_leaf_of_many", m_root_is_a_leaf, INVALID, None),
]
for side in ("left", "right"):
    REFUSALS += [
        # rtw_bvh_node
        (f"node.{side}=node_count", lambda w, s=side: setattr(w.arrays["nodes"][1], s, w.raw.node_count), INVALID, [f"nodes[1].{side}"]),
        (f"node.{side}=~leaf_count", lambda w, s=side: setattr(w.arrays["nodes"][1], s, -1 - w.raw.leaf_count), INVALID, [f"nodes[1].{side}"]),
        (f"node.{side}=INT32_MIN", m_set("nodes", 1, side, I32_MIN), INVALID, [f"nodes[1].{side}"]),
        (f"node.{side}=INT32_MAX", m_set("nodes", 1, side, I32_MAX), INVALID, [f"nodes[1].{side}"]),
    ]
REFUSALS += [
    ("node.axis=-1", m_set("nodes", 2, "axis", -1), INVALID, ["nodes[2].axis"]),
    ("node.axis=3", m_set("nodes", 2, "axis", 3), INVALID, ["nodes[2].axis"]),
    ("node.self_reference", m_self_reference, INVALID, None),
    ("node.reached_twice", m_node_twice, INVALID, None),
    ("node.cycle", m_cycle, INVALID, None),
    ("node.referenced_by_no_node", m_node_by_no_node, INVALID, None),
    # rtw_leaf
    ("leaf.geom_kind=-1", m_set("leaves", 3, "geom_kind", -1), INVALID, ["leaves[3].geom_kind"]),
    ("leaf.geom_kind=4", m_set("leaves", 3, "geom_kind", 4), INVALID, ["leaves[3].geom_kind"]),
    ("leaf.material=-1", m_set("leaves", 3, "material", -1), INVALID, ["leaves[3].material"]),
    ("leaf.material=count", lambda w: setattr(w.arrays["leaves"][3], "material", w.raw.material_count), INVALID, ["leaves[3].material"]),
    ("leaf.flags=8", m_set("leaves", 3, "flags", 8), INVALID, ["leaves[3].flags"]),
    ("leaf.flags=bit31", m_set("leaves", 3, "flags", 0x80000000), INVALID, ["leaves[3].flags"]),
    ("leaf.referenced_twice", m_leaf_twice, INVALID, None),
    ("leaf.referenced_by_no_node", m_leaf_by_no_node, INVALID, None),
]
for kind, table in enumerate(("spheres", "rects", "boxes", "triangles")):
    def geom_index(value, kind=kind, table=table):
        def f(w):
            i = leaf_of_kind(kind)(w.raw)
            w.arrays["leaves"][i].geom_index = getattr(w.raw, COUNTS[table]) if value == "count" else value
            return [f"leaves[{i}].geom_index"]
        return f
    REFUSALS += [(f"leaf.geom_index=-1({table})", geom_index(-1), INVALID, None),
                 (f"leaf.geom_index=count({table})", geom_index("count"), INVALID, None)]
REFUSALS += [
    # rtw_material
    ("material.kind=-1", m_set("materials", 0, "kind", -1), INVALID, ["materials[0].kind"]),
    ("material.kind=5", m_set("materials", 0, "kind", 5), INVALID, ["materials[0].kind"]),
    ("material.texture=-1", lambda w: [setattr(w.arrays["materials"][mat_not(N.MAT_DIELECTRIC)(w.raw)], "texture", -1)] and None,
     INVALID, ["materials[", "].texture"]),
    ("material.texture=count", lambda w: [setattr(w.arrays["materials"][mat_not(N.MAT_DIELECTRIC)(w.raw)], "texture",
                                                    w.raw.texture_count)] and None, INVALID, ["materials[", "].texture"]),
    # rtw_texture
    ("texture.kind=-1", m_wild_texture(-1), INVALID, None),
    ("texture.kind=4", m_wild_texture(4), INVALID, None),
    ("texture.kind=7", m_wild_texture(7), INVALID, None),
    ("texture.checker_self_reference", m_checker_self, INVALID, None),
    ("texture.checker_two_cycle", m_checker_two_cycle, INVALID, None),
    ("texture.checker_chain_one_too_long", m_chain_too_long, INVALID, None),
]
for kind, field, count in ((N.TEX_CHECKER, "even", "texture_count"), (N.TEX_CHECKER, "odd", "texture_count"),
                           (N.TEX_IMAGE, "image", "image_count"), (N.TEX_MARBLE, "perlin", "perlin_count")):
    def tex_index(value, kind=kind, field=field, count=count):
        def f(w):
            i = tex_of_kind(kind)(w.raw)
            setattr(w.arrays["textures"][i], field, getattr(w.raw, count) if value == "count" else value)
            return [f"textures[{i}].{field}"]
        return f
    REFUSALS += [(f"texture.{field}=-1", tex_index(-1), INVALID, None), (f"texture.{field}=count", tex_index("count"), INVALID, None),
                 (f"texture.{field}=INT32_MAX", tex_index(I32_MAX), INVALID, None)]
REFUSALS += [
    # rtw_perlin
    ("perlin.bits=0", m_set("perlins", 0, "bits", 0), INVALID, ["perlins[0].bits"]),
    ("perlin.bits=9", m_set("perlins", 0, "bits", 9), INVALID, ["perlins[0].bits"]),
    ("perlin.bits=-1", m_set("perlins", 0, "bits", -1), INVALID, ["perlins[0].bits"]),
]
for a in ("perm_x", "perm_y", "perm_z"):
    REFUSALS += [
        (f"perlin.{a}[0]=2^bits", m_perlin(a, 0, lambda p: 1 << p.bits), INVALID, None),
        (f"perlin.{a}[last]=2^bits", m_perlin(a, lambda p: (1 << p.bits) - 1, lambda p: 1 << p.bits), INVALID, None),
        (f"perlin.{a}[3]=16,bits=4", m_perlin(a, 3, 16, bits=4), INVALID, None),  # inside the 768 floats, outside the reference's 16 vectors
        (f"perlin.{a}[3]=2^32-1", m_perlin(a, 3, 2 ** 32 - 1), INVALID, None),
    ]
REFUSALS += [
    # rtw_image
    ("image.width=0", m_set("images", 0, "width", 0), INVALID, ["images[0].width"]),
    ("image.width=-1", m_set("images", 0, "width", -1), INVALID, ["images[0].width"]),
    ("image.height=0", m_set("images", 0, "height", 0), INVALID, ["images[0].height"]),
    ("image.height=-1", m_set("images", 0, "height", -1), INVALID, ["images[0].height"]),
    ("image.rgb=null", m_set("images", 1, "rgb", C.POINTER(C.c_uint8)()), INVALID, ["images[1].rgb"]),
    # rtw_rect: the table and the light
    ("rect.plane=-1", m_set("rects", 1, "plane", -1), INVALID, ["rects[1].plane"]),
    ("rect.plane=3", m_set("rects", 1, "plane", 3), INVALID, ["rects[1].plane"]),
    ("light.plane=-1", m_light("plane", -1), INVALID, ["light.plane"]),
    ("light.plane=3", m_light("plane", 3), INVALID, ["light.plane"]),
    ("light.never_filled_in", m_light_never_filled, INVALID, ["light.r0"]),
    ("has_light=2", lambda w: setattr(w.raw, "has_light", 2), INVALID, ["has_light"]),
    ("light.r0_reversed", lambda w: w.raw.light.r0.__setitem__(slice(0, 2), [1.0, -1.0]), INVALID, ["light.r0"]),
    ("light.r1_empty", lambda w: w.raw.light.r1.__setitem__(slice(0, 2), [0.5, 0.5]), INVALID, ["light.r1"]),
    ("light.r1_nan", lambda w: w.raw.light.r1.__setitem__(1, math.nan), INVALID, ["light.r1"]),
    ("light.r0_past_2^30", lambda w: w.raw.light.r0.__setitem__(1, 2.0 ** 31), INVALID, ["light.r0"]),
    ("light.dist=nan", m_light("dist", math.nan), INVALID, ["light.dist"]),
    ("leaf_count=0", m_count("leaves", 0), INVALID, ["leaf_count"]),
    # rtw_camera: the shutter interval (the ray-time sampler redraws for ever on a reversed or non-finite one)
    ("camera.time0>time1", lambda w: setattr(w.raw.camera, "time0", 2.0), INVALID, ["camera.time0", "camera.time1"]),
    ("camera.time0=nan", lambda w: setattr(w.raw.camera, "time0", math.nan), INVALID, ["camera.time0"]),
    ("camera.time1=inf", lambda w: setattr(w.raw.camera, "time1", math.inf), INVALID, ["camera.time1"]),
    ("camera.time1-time0=inf", lambda w: (setattr(w.raw.camera, "time0", -3e38), setattr(w.raw.camera, "time1", 3e38)) and None,
     INVALID, ["camera.time0", "camera.time1"]),
]
for table, count, _ in TABLES:
    REFUSALS += [(f"{table}=null", m_null(table), INVALID, [table, count]),
                 (f"{count}=-1", m_count(table, -1), INVALID, [count]),
                 (f"{count}=INT32_MIN", m_count(table, I32_MIN), INVALID, [count])]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_one_wrong_field_is_refused(base, case):
    _, mutate, code, names = case
    w = OwnedWorld(base)
    accepted(w)
    found = mutate(w)
    refused(w, code, *(names if names is not None else found))


# ---- accepted on purpose ----------------------------------------------------------------------------------------
def test_a_dielectric_ignores_its_texture(base):
    w = OwnedWorld(base)
    i = first(w.raw, "materials", lambda m: m.kind == N.MAT_DIELECTRIC)
    assert w.raw.materials[i].texture == -1  # the builder's convention
    for v in (-1, WILD, I32_MIN):
        w.arrays["materials"][i].texture = v
        accepted(w)


def test_fields_a_texture_kind_does_not_use_are_ignored(base):
    w = OwnedWorld(base)
    m_solid_with_wild_fields(w)
    accepted(w)


def test_perm_entries_beyond_the_lattice_are_never_read(base):
    w = OwnedWorld(base)
    m_perlin("perm_x", 3, 0, bits=4)(w)
    for a in ("perm_x", "perm_y", "perm_z"):
        getattr(w.arrays["perlins"][0], a)[16] = 2 ** 32 - 1
    accepted(w)


def test_empty_tables_may_be_null():
    w = OwnedWorld(V.sphere_cloud(6))
    for table in ("rects", "boxes", "triangles", "images", "perlins"):
        assert getattr(w.raw, COUNTS[table]) == 0 and not getattr(w.raw, table)
    accepted(w)


def test_longest_checker_chain_is_accepted_and_shared_links_are_no_cycle(base):
    w = OwnedWorld(base)
    add_chain(w, MAX_CHAIN)  # even and odd of every link name the same next texture: reached twice, no cycle
    accepted(w)


# ---- the 2^30 bound: every coordinate it covers --------------------------------------------------------------------
LIM = 2.0 ** 30
PAST = float(np.nextafter(np.float32(LIM), np.float32(np.inf)))


def _coords():
    out = [("nodes", lambda raw: 1, f, k) for f in ("min", "max") for k in range(3)]
    out += [("spheres", lambda raw: 2, "center", k) for k in range(3)] + [("spheres", lambda raw: 2, "radius", None)]
    out += [("rects", lambda raw: 1, "dist", None)]
    out += [("leaves", lambda raw: 4, "offset", k) for k in range(3)]
    out += [("leaves", lambda raw: first(raw, "leaves", lambda l: l.flags & N.LEAF_ANIMATION), "velocity", k) for k in range(3)]
    out += [("camera", None, "position", k) for k in range(3)]
    return out


COORDS = _coords()


@pytest.mark.parametrize("coord", COORDS, ids=[f"{t}.{f}{'' if k is None else k}" for t, _, f, k in COORDS])
def test_coordinate_bound(base, coord):
    table, index, field, k = coord
    w = OwnedWorld(base)
    assert w.raw.camera.time0 == 0.0 and w.raw.camera.time1 == 1.0  # velocity x 1: the bound is the velocity's own
    holder = w.raw.camera if table == "camera" else w.arrays[table][index(w.raw)]
    name = "camera.position" if table == "camera" else f"{table}[{index(w.raw)}].{field}"

    def put(v):
        if k is None:
            setattr(holder, field, v)
        else:
            getattr(holder, field)[k] = v

    for v in (LIM, -LIM):
        put(v)
        accepted(w)
    for v in (math.nan, math.inf, -math.inf, PAST, -PAST):
        put(v)
        refused(w, INVALID, name, "2^30")


# ---- the depth bound ------------------------------------------------------------------------------------------------
def test_depth_bound():
    w = chain_world(MAX_DEPTH)
    assert tree_depth(w.raw) == MAX_DEPTH and accepted(w) == MAX_DEPTH
    assert accepted(chain_world(MAX_DEPTH, extra_rect=True)) == MAX_DEPTH
    w = chain_world(MAX_DEPTH + 1)
    assert tree_depth(w.raw) == MAX_DEPTH + 1
    refused(w, UNSUPPORTED, "nodes", "depth 33")


def test_one_leaf_world_has_depth_zero():
    w = OwnedWorld(row_world(1))
    assert (w.raw.root, w.raw.node_count, w.raw.leaf_count) == (-1, 0, 1)
    assert accepted(w) == 0


# ---- the stand-alone fuzz: the validator and the oracle, plain and under ASan + UBSan ----------------------------------
@pytest.fixture(scope="module")
def fuzz_programs(tmp_path_factory):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    d = tmp_path_factory.mktemp("world_check_fuzz")
    csrc = os.path.join(ROOT, "raytracinginaweekend_amd", "csrc")
    cxx = [os.path.join(csrc, f) for f in ("rtw_check.cpp", "rtw_common.cpp", "scene_builder.cpp", "demo_worlds.cpp")]
    c = [os.path.join(ROOT, "tests", "native", "world_check_fuzz.c"), os.path.join(ROOT, "oracle", "rtw_oracle.c")]
    variants = (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    jobs, objs = [], {tag: [] for tag, _ in variants}
    for tag, flags in variants:
        for src in c + cxx:
            obj = str(d / f"{tag}_{os.path.basename(src)}.o")
            objs[tag].append(obj)
            cc = (["gcc", "-std=c11"] if src.endswith(".c") else ["g++", "-std=c++17", f"-I{rocm}/include", "-D__HIP_PLATFORM_AMD__"])
            jobs.append([*cc, "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-function", *flags, "-c", src, "-o", obj])
    with ThreadPoolExecutor(4) as pool:  # twelve small translation units
        list(pool.map(lambda cmd: subprocess.run(cmd, check=True), jobs))
    out = []
    for tag, flags in variants:
        out.append(str(d / f"world_check_fuzz_{tag}"))
        subprocess.run(["g++", *flags, "-o", out[-1], *objs[tag], "-lm", "-lpthread"], check=True)
    return out


FUZZ_MUTANTS = 40000


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_fuzz_accepted_worlds_render_in_bounds(fuzz_programs, sanitized):
    """Seeded one- and two-field mutants: the validator answers each without a sanitizer report, and every mutant it
    accepts renders 8 x 8 x 2 spp at depth 8 in the oracle without one (a proxy for the device's reads: the oracle
    indexes the same tables with the same indices).  The time limit is the oracle's hang detector: a timeout fails."""
    out = subprocess.run([fuzz_programs[1 if sanitized else 0], str(FUZZ_MUTANTS), "20261020"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stderr == "", out.stderr[-3000:]
    m = re.search(r"mutants (\d+) refused (\d+) accepted (\d+) rendered (\d+)", out.stdout)
    assert m, out.stdout[-2000:]
    tried, no, yes, rendered = map(int, m.groups())
    print(out.stdout.strip().split("\n")[-1])
    assert tried == FUZZ_MUTANTS and no + yes == tried and no > 0 and yes > 0 and rendered == yes
