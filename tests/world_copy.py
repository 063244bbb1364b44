"""A flat rtw_world that owns its memory (plain helpers, no fixtures): deep copies of a builder world's tables in
ctypes arrays, so a test can change any field, grow a table or null a pointer without touching the builder's
world.  Quacks like a World for the package and for oracle/pyoracle.py (`raw`, `ptr()`).
tests/test_world_check.py mutates such copies; tests/test_gpu_world_edges.py renders the ones the validator accepts."""
import ctypes as C

import raytracinginaweekend_amd as R
from raytracinginaweekend_amd import _native as N

# (table, its count, element type) in rtw.h's order
TABLES = [("nodes", "node_count", N.BvhNode), ("leaves", "leaf_count", N.Leaf), ("spheres", "sphere_count", N.Sphere),
          ("rects", "rect_count", N.Rect), ("boxes", "box_count", N.Box), ("triangles", "triangle_count", N.Triangle),
          ("materials", "material_count", N.Material), ("textures", "texture_count", N.Texture),
          ("images", "image_count", N.Image), ("perlins", "perlin_count", N.Perlin)]
TYPES = {name: typ for name, _, typ in TABLES}
COUNTS = {name: count for name, count, _ in TABLES}


class OwnedWorld:
    def __init__(self, src):
        src = getattr(src, "raw", src)
        self.raw = N.World()
        C.memmove(C.byref(self.raw), C.byref(src), C.sizeof(N.World))
        self.arrays, self.pixels = {}, []
        for name, count, typ in TABLES:
            n = getattr(src, count)
            self._set(name, n, getattr(src, name), n)
        for i in range(self.raw.image_count):  # the texels too
            im = self.raw.images[i]
            self.set_image(i, bytes(C.string_at(im.rgb, im.width * im.height * 3)), im.width, im.height)

    def _set(self, name, n, src, n_copy):
        typ = TYPES[name]
        arr = (typ * max(n, 1))()
        if n_copy:
            C.memmove(arr, src, n_copy * C.sizeof(typ))
        self.arrays[name] = arr
        setattr(self.raw, name, C.cast(arr, C.POINTER(typ)) if n else C.POINTER(typ)())
        setattr(self.raw, COUNTS[name], n)

    def resize(self, name: str, n: int):
        """Table `name` with n entries: the first min(old, n) kept, new ones zeroed.  Returns the array."""
        old = self.arrays[name]
        self._set(name, n, old, min(n, getattr(self.raw, COUNTS[name])))
        return self.arrays[name]

    def set_image(self, i: int, rgb: bytes, width: int, height: int):
        buf = (C.c_uint8 * max(1, len(rgb))).from_buffer_copy(rgb or b"\0")
        self.pixels.append(buf)
        im = self.arrays["images"][i]
        im.width, im.height, im.rgb = width, height, C.cast(buf, C.POINTER(C.c_uint8))

    def ptr(self):
        return C.byref(self.raw)


def tree_depth(raw) -> int:
    """Nodes on the longest root-to-leaf path of a well-formed tree (0: a one-leaf world)."""
    depth, todo = 0, [(raw.root, 1)]
    while todo:
        n, d = todo.pop()
        if n >= 0:
            depth = max(depth, d)
            todo += [(raw.nodes[n].left, d + 1), (raw.nodes[n].right, d + 1)]
    return depth


def chain_tree(world: OwnedWorld, boxes, axis: int = 1) -> None:
    """Replace the world's tree by a left-deep chain over its L leaves (L - 1 nodes, that many levels deep): node i
    holds leaf i on the right and node i + 1 on the left, the last node leaves L - 1 (left) and L - 2 (right); node
    i's box is the union of boxes[i:] (boxes: per leaf (min[3], max[3])), so the boxes nest.  Every node splits on
    `axis`: a ray whose direction is positive there takes the left child first and pushes the right one, so it
    holds one stack entry per level when it stands on the last node; the other rays take the leaf first."""
    L = world.raw.leaf_count
    nodes = world.resize("nodes", L - 1)
    lo, hi = list(boxes[L - 1][0]), list(boxes[L - 1][1])
    for i in range(L - 2, -1, -1):
        lo = [min(a, b) for a, b in zip(lo, boxes[i][0])]
        hi = [max(a, b) for a, b in zip(hi, boxes[i][1])]
        nodes[i].min[:], nodes[i].max[:] = lo, hi
        nodes[i].axis = axis
        nodes[i].left = i + 1 if i < L - 2 else -1 - (L - 1)
        nodes[i].right = -1 - i
    world.raw.root = 0


def add_chain(w, n_textures, close_on=None):
    """Append a checker chain of n_textures (the last a solid, not black) and hang it on material 0 (a Lambertian or
    whatever the world has first that is no dielectric).  close_on = k: the last checker points back at link k."""
    raw = w.raw
    t0 = raw.texture_count
    tex = w.resize("textures", t0 + n_textures)
    for k in range(n_textures - 1):
        tex[t0 + k].kind, tex[t0 + k].inv_frequency = N.TEX_CHECKER, 0.5 + 0.01 * k
        tex[t0 + k].even = tex[t0 + k].odd = t0 + k + 1
    last = tex[t0 + n_textures - 1]
    last.kind = N.TEX_SOLID
    last.color[:] = [0.9, 0.4, 0.2]
    if close_on is not None:
        tex[t0 + n_textures - 2].odd = t0 + close_on
    m = next(i for i in range(raw.material_count) if raw.materials[i].kind != N.MAT_DIELECTRIC)
    w.arrays["materials"][m].texture = t0
    return t0


def row_world(n: int, extra_rect: bool = False):
    """n small plain spheres in a row along -z, the camera on the row's axis looking down it through a narrow lens
    (6 degrees: the far end of a 33-sphere row is a dozen pixels wide at 48 x 27, and the rays towards it cross every
    nested box of chain_tree); with extra_rect, a rect behind the row as the last leaf."""
    wb = R.WorldBuilder()
    mats = [wb.material_lambert_solid((0.7, 0.3, 0.2)), wb.material_metal_solid((0.8, 0.8, 0.8), 0.1),
            wb.material_dielectric(1.5)]
    g = wb.new_group()
    for i in range(n):  # off the axis by turns, so that rays pass the near ones and reach the far ones
        g.add(wb.new_obj_sphere(0.3, mats[i % 3]).translate((0.55 * (1 if i % 2 else -1), 0.2 * ((i // 2) % 3 - 1), -1.0 * i)))
    if extra_rect:
        g.add(wb.new_obj_rect_xy((0.0, 0.0, -1.0 * n), 6.0, 6.0, wb.material_lambert_solid((0.3, 0.6, 0.3))))
    cam = R.Camera.build().vertical_fov(6.0, 9.0 / 16.0).position((0.0, 0.0, 4.0)).look_at((0, 1, 0), (0.0, 0.0, -1.0)).build()
    return g.build().finish(wb, R.BackgroundColor.sky(), cam)


def leaf_boxes(raw):
    """Per leaf (min, max) of a world of plain spheres and plain xy rects (a rect's box: 1e-4 thick, as the reference pads it)."""
    out = []
    for i in range(raw.leaf_count):
        l = raw.leaves[i]
        assert l.flags == 0
        if l.geom_kind == N.GEOM_SPHERE:
            s = raw.spheres[l.geom_index]
            out.append(([c - s.radius for c in s.center], [c + s.radius for c in s.center]))
        else:
            r = raw.rects[l.geom_index]
            assert l.geom_kind == N.GEOM_RECT and r.plane == N.PLANE_XY
            out.append(([r.r0[0], r.r1[0], r.dist - 1e-4], [r.r0[1], r.r1[1], r.dist + 1e-4]))
    return out


def chain_world(depth: int, extra_rect: bool = False) -> OwnedWorld:
    """row_world under a hand-made left-deep tree `depth` levels deep (depth + 1 leaves)."""
    w = OwnedWorld(row_world(depth + 1 - (1 if extra_rect else 0), extra_rect))
    assert w.raw.leaf_count == depth + 1
    chain_tree(w, leaf_boxes(w.raw))
    return w
