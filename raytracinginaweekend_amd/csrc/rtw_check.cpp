// rtw_check.cpp -- rtw_world_check: the validator between a caller's flat rtw_world and everything that
// indexes its tables (the upload, the SAH builder, the primary lists, the oracle).  Host code only: it
// needs no device, so tests and a sanitized stand-alone build reach it directly.  The contract is rtw.h's.
//
// Order matters: counts and pointers first, then each table's own fields, then what follows indices
// (the texture chains, the tree) -- nothing is dereferenced or followed before it has been checked.
#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>

#include "rtw_common.h"
#include "../../include/rtw_cull.h"

namespace {

int bad(const std::string& what) { return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "invalid world: " + what); }
std::string at(const char* table, int64_t i, const char* field) {
    return std::string(table) + "[" + std::to_string(i) + "]." + field;
}
bool in_table(int32_t i, int32_t count) { return i >= 0 && i < count; }

// coordinate bound behind the exact fast division of the slab test (|a| <= 2^40 there):
// every coordinate the device sees stays at or below 2^30 in magnitude (a NaN fails the comparison)
const float LIM = 1073741824.0f;
bool big(const float* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!(v[k] >= -LIM && v[k] <= LIM)) return true;
    return false;
}

int check_rect(const rtw_rect& r, const std::string& name) {
    if (r.plane < RTW_PLANE_XY || r.plane > RTW_PLANE_YZ) return bad(name + ".plane " + std::to_string(r.plane) + " is no RTW_PLANE_*");
    if (big(&r.dist, 1)) return bad(name + ".dist beyond 2^30");
    return RTW_OK;
}

}  // namespace

extern "C" RTW_API int rtw_world_check(const rtw_world* w, int32_t* depth_out) {
    if (!w) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null world");
    // ---- counts and pointers
    const struct {
        const char* count_name;
        const char* table;
        int32_t count;
        const void* data;
    } tables[] = {
        {"node_count", "nodes", w->node_count, w->nodes},
        {"leaf_count", "leaves", w->leaf_count, w->leaves},
        {"sphere_count", "spheres", w->sphere_count, w->spheres},
        {"rect_count", "rects", w->rect_count, w->rects},
        {"box_count", "boxes", w->box_count, w->boxes},
        {"triangle_count", "triangles", w->triangle_count, w->triangles},
        {"material_count", "materials", w->material_count, w->materials},
        {"texture_count", "textures", w->texture_count, w->textures},
        {"image_count", "images", w->image_count, w->images},
        {"perlin_count", "perlins", w->perlin_count, w->perlins},
    };
    for (const auto& t : tables) {
        if (t.count < 0) return bad(std::string(t.count_name) + " " + std::to_string(t.count) + " is negative");
        if (t.count > 0 && !t.data) return bad(std::string(t.table) + " is null with " + t.count_name + " " + std::to_string(t.count));
    }
    if (w->leaf_count < 1) return bad("leaf_count 0: world has no leaves");
    // root: a node, or ~leaf (in 64 bits: -1 - INT32_MIN does not fit 32)
    if (w->root >= 0 ? w->root >= w->node_count : -1 - (int64_t)w->root >= w->leaf_count)
        return bad("root " + std::to_string(w->root) + " out of range");
    if (w->has_light != 0 && w->has_light != 1) return bad("has_light " + std::to_string(w->has_light) + " is neither 0 nor 1");
    if (w->has_light) {
        if (const int v = check_rect(w->light, "light")) return v;
        // the reference samples the light with gen_range(r[0], r[1]), which panics on an empty or overflowing range
        const float* rs[2] = {w->light.r0, w->light.r1};
        for (int k = 0; k < 2; ++k)
            if (!(rs[k][0] < rs[k][1]) || big(rs[k], 2))
                return bad(std::string("light.r") + (k ? "1" : "0") + " is no increasing range within 2^30");
    }
    // the shutter: the reference draws a ray's time with gen_range(time0, time1) unless they are equal, which panics
    // on a reversed or non-finite interval (the restated sampler would redraw for ever, on the device too)
    if (!std::isfinite(w->camera.time0)) return bad("camera.time0 is not finite");
    if (!std::isfinite(w->camera.time1)) return bad("camera.time1 is not finite");
    if (!(w->camera.time0 <= w->camera.time1) || !std::isfinite(w->camera.time1 - w->camera.time0))
        return bad("camera.time0 .. camera.time1 is no finite interval in order");
    // ---- each table's own fields
    for (int i = 0; i < w->leaf_count; ++i) {
        const rtw_leaf& L = w->leaves[i];
        const int counts[4] = {w->sphere_count, w->rect_count, w->box_count, w->triangle_count};
        if (L.geom_kind < 0 || L.geom_kind > 3) return bad(at("leaves", i, "geom_kind") + " " + std::to_string(L.geom_kind) + " is no RTW_GEOM_*");
        if (!in_table(L.geom_index, counts[L.geom_kind])) return bad(at("leaves", i, "geom_index") + " " + std::to_string(L.geom_index) + " out of range");
        if (!in_table(L.material, w->material_count)) return bad(at("leaves", i, "material") + " " + std::to_string(L.material) + " out of range");
        if (L.flags & ~(RTW_LEAF_VOLUME | RTW_LEAF_TRANSFORM | RTW_LEAF_ANIMATION)) return bad(at("leaves", i, "flags") + " has bits above RTW_LEAF_ANIMATION");
    }
    for (int i = 0; i < w->material_count; ++i) {
        const rtw_material& m = w->materials[i];
        if (m.kind < 0 || m.kind > 4) return bad(at("materials", i, "kind") + " " + std::to_string(m.kind) + " is no RTW_MAT_*");
        if (m.kind != RTW_MAT_DIELECTRIC && !in_table(m.texture, w->texture_count))
            return bad(at("materials", i, "texture") + " " + std::to_string(m.texture) + " out of range");
    }
    for (int i = 0; i < w->texture_count; ++i) {
        const rtw_texture& t = w->textures[i];
        // every kind the device and the oracle do not know would be sampled as a marble (their last arm)
        if (t.kind < RTW_TEX_SOLID || t.kind > RTW_TEX_IMAGE) return bad(at("textures", i, "kind") + " " + std::to_string(t.kind) + " is no RTW_TEX_*");
        if (t.kind == RTW_TEX_CHECKER && !in_table(t.even, w->texture_count)) return bad(at("textures", i, "even") + " " + std::to_string(t.even) + " out of range");
        if (t.kind == RTW_TEX_CHECKER && !in_table(t.odd, w->texture_count)) return bad(at("textures", i, "odd") + " " + std::to_string(t.odd) + " out of range");
        if (t.kind == RTW_TEX_IMAGE && !in_table(t.image, w->image_count)) return bad(at("textures", i, "image") + " " + std::to_string(t.image) + " out of range");
        if (t.kind == RTW_TEX_MARBLE && !in_table(t.perlin, w->perlin_count)) return bad(at("textures", i, "perlin") + " " + std::to_string(t.perlin) + " out of range");
    }
    for (int i = 0; i < w->perlin_count; ++i) {
        const rtw_perlin& P = w->perlins[i];
        if (P.bits < 1 || P.bits > 8) return bad(at("perlins", i, "bits") + " " + std::to_string(P.bits) + " outside 1..8");
        // perlin_noise reads ranvec[perm_x[..] ^ perm_y[..] ^ perm_z[..]] at indices masked to bits: entries below
        // 2^bits keep the xor below 2^bits, inside the vectors the reference generated (perlin.rs:20-35)
        const uint32_t n = 1u << P.bits;
        const uint32_t* perms[3] = {P.perm_x, P.perm_y, P.perm_z};
        const char* names[3] = {"perm_x", "perm_y", "perm_z"};
        for (int a = 0; a < 3; ++a)
            for (uint32_t k = 0; k < n; ++k)
                if (perms[a][k] >= n)
                    return bad(at("perlins", i, names[a]) + "[" + std::to_string(k) + "] " + std::to_string(perms[a][k]) + " is not below 2^bits");
    }
    for (int i = 0; i < w->image_count; ++i) {
        const rtw_image& im = w->images[i];
        if (im.width < 1) return bad(at("images", i, "width") + " " + std::to_string(im.width) + " below 1");
        if (im.height < 1) return bad(at("images", i, "height") + " " + std::to_string(im.height) + " below 1");
        if (!im.rgb) return bad(at("images", i, "rgb") + " is null");
    }
    for (int i = 0; i < w->rect_count; ++i)
        if (const int v = check_rect(w->rects[i], "rects[" + std::to_string(i) + "]")) return v;
    for (int i = 0; i < w->node_count; ++i) {
        const rtw_bvh_node& nd = w->nodes[i];
        if (nd.axis < 0 || nd.axis > 2) return bad(at("nodes", i, "axis") + " " + std::to_string(nd.axis) + " outside 0..2");
        if (big(nd.min, 3)) return bad(at("nodes", i, "min") + " beyond 2^30");
        if (big(nd.max, 3)) return bad(at("nodes", i, "max") + " beyond 2^30");
    }
    for (int i = 0; i < w->sphere_count; ++i) {
        if (big(w->spheres[i].center, 3)) return bad(at("spheres", i, "center") + " beyond 2^30");
        if (big(&w->spheres[i].radius, 1)) return bad(at("spheres", i, "radius") + " beyond 2^30");
    }
    // an Animation offset is velocity x ray time, the rolling shutter's pace included (rtw_ray_time_range)
    float rt0 = 0.0f, rt1 = 0.0f;
    const float tmax = rtw_ray_time_range(&w->camera, &rt0, &rt1) ? std::max(std::fabs(rt0), std::fabs(rt1))
                                                                   : std::numeric_limits<float>::infinity();
    for (int i = 0; i < w->leaf_count; ++i) {
        const rtw_leaf& L = w->leaves[i];
        float vt[3];
        for (int k = 0; k < 3; ++k)
            vt[k] = (L.flags & RTW_LEAF_ANIMATION) && L.velocity[k] != 0.0f ? L.velocity[k] * tmax : 0.0f;
        if (big(L.offset, 3)) return bad(at("leaves", i, "offset") + " beyond 2^30");
        if (big(vt, 3)) return bad(at("leaves", i, "velocity") + " x ray time beyond 2^30");
    }
    if (big(w->camera.position, 3)) return bad("camera.position beyond 2^30");
    // ---- checker chains: no cycle, and no path longer than the device's loop finishes (texture_sample gives
    // up after RTW_MAX_TEXTURE_CHAIN textures and returns black; the oracle, like the reference, never gives up).
    // chain[t] = textures on the longest path from t, itself included; 0 = not yet known, -1 = on the stack.
    {
        std::vector<int32_t> chain((size_t)w->texture_count, 0);
        std::vector<int32_t> stack;
        for (int32_t s = 0; s < w->texture_count; ++s) {
            if (chain[(size_t)s]) continue;
            stack.push_back(s);
            while (!stack.empty()) {
                const int32_t t = stack.back();
                const rtw_texture& T = w->textures[t];
                if (chain[(size_t)t] > 0) {  // reached a second time, from another parent
                    stack.pop_back();
                    continue;
                }
                if (T.kind != RTW_TEX_CHECKER) {
                    chain[(size_t)t] = 1;
                    stack.pop_back();
                    continue;
                }
                const int32_t ce = chain[(size_t)T.even], co = chain[(size_t)T.odd];
                if (chain[(size_t)t] == -1 && ce > 0 && co > 0) {  // both children done
                    chain[(size_t)t] = 1 + std::max(ce, co);
                    if (chain[(size_t)t] > RTW_MAX_TEXTURE_CHAIN)
                        return bad(at("textures", t, "even") + " / odd start a checker chain of more than " +
                                   std::to_string(RTW_MAX_TEXTURE_CHAIN) + " textures");
                    stack.pop_back();
                    continue;
                }
                chain[(size_t)t] = -1;
                for (const int32_t c : {T.even, T.odd}) {
                    if (chain[(size_t)c] == -1)
                        return bad(at("textures", t, c == T.even ? "even" : "odd") + " " + std::to_string(c) + " closes a checker cycle");
                    if (chain[(size_t)c] == 0) stack.push_back(c);
                }
            }
        }
    }
    // ---- the tree: every node and every leaf referenced exactly once, and its depth (the per-lane stack
    // holds one entry per level)
    std::vector<std::pair<int32_t, int>> todo;
    int maxd = 0;
    std::vector<uint8_t> seen_node((size_t)w->node_count, 0), seen_leaf((size_t)w->leaf_count, 0);
    auto visit = [&](int32_t c, const std::string& name) {
        if (c < 0) {
            const int64_t leaf = -1 - (int64_t)c;
            if (leaf >= w->leaf_count) return bad(name + " " + std::to_string(c) + " names no leaf");
            if (seen_leaf[(size_t)leaf]) return bad(name + " " + std::to_string(c) + " references leaf " + std::to_string(leaf) + " a second time");
            seen_leaf[(size_t)leaf] = 1;
            return (int)RTW_OK;
        }
        if (c >= w->node_count) return bad(name + " " + std::to_string(c) + " names no node");
        if (seen_node[(size_t)c]) return bad(name + " " + std::to_string(c) + " references node " + std::to_string(c) + " a second time");
        seen_node[(size_t)c] = 1;
        return (int)RTW_OK;
    };
    if (const int v = visit(w->root, "root")) return v;
    if (w->root >= 0) todo.emplace_back(w->root, 1);
    while (!todo.empty()) {
        const auto [n, d] = todo.back();
        todo.pop_back();
        maxd = std::max(maxd, d);
        const rtw_bvh_node& nd = w->nodes[n];
        if (const int v = visit(nd.left, at("nodes", n, "left"))) return v;
        if (const int v = visit(nd.right, at("nodes", n, "right"))) return v;
        if (nd.left >= 0) todo.emplace_back(nd.left, d + 1);
        if (nd.right >= 0) todo.emplace_back(nd.right, d + 1);
    }
    for (int32_t i = 0; i < w->leaf_count; ++i)
        if (!seen_leaf[(size_t)i]) return bad("leaves[" + std::to_string(i) + "] is referenced by no node: the tree never reaches it");
    for (int32_t i = 0; i < w->node_count; ++i)
        if (!seen_node[(size_t)i]) return bad("nodes[" + std::to_string(i) + "] is referenced by no node: the tree never reaches it");
    if (maxd > RTW_MAX_BVH_DEPTH)
        return rtw::fail(RTW_ERR_UNSUPPORTED, "invalid world: nodes: BVH of depth " + std::to_string(maxd) + " is deeper than the device stack (" +
                                                  std::to_string(RTW_MAX_BVH_DEPTH) + ")");
    if (depth_out) *depth_out = maxd;
    return RTW_OK;
}
