/* world_check_fuzz.c -- seeded mutants of small worlds against rtw_world_check and the oracle.
 *
 * Stand-alone (its own main; tests/test_world_check.py builds it plain and with ASan + UBSan and runs it alone,
 * nothing preloaded).  Links csrc/rtw_check.cpp, rtw_common.cpp, scene_builder.cpp, demo_worlds.cpp and
 * oracle/rtw_oracle.c.
 *
 *   world_check_fuzz <mutants> <seed> [trace]      (trace: each mutant's number and verdict before it renders)
 *
 * Every mutant is a fresh deep copy of one of three builder worlds in heap blocks of the exact size (so a read one
 * element past a table is a sanitizer report) with one or two fields changed:
 *   integers   value - 1, value + 1, 0, -1, a count of the world, that count + 1, INT32_MIN, INT32_MAX;
 *   floats     one to three random bits flipped, or a special value (NaN, +-inf, +-2^30, the float after 2^30);
 *   pointers   a table pointer nulled.
 * Counts and image sizes only shrink (0, -1, value - 1, INT32_MIN): a caller who claims more elements than it
 * allocated is beyond any validator.
 * 1. rtw_world_check must answer without a sanitizer report.
 * 2. If it accepts, the oracle renders 8 x 8 at 2 spp, depth 8 of the mutant without one (the driver's time limit
 *    catches a walk or a texture chain that never ends).
 * Prints "mutants N refused R accepted A rendered A" and the refusals per table; exit 0. */
#include <inttypes.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rtw.h"
#include "../../oracle/rtw_oracle.h"

/* ---- splitmix64 --------------------------------------------------------------------------------- */
static uint64_t g_state;
static uint64_t rnd(void) {
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

static void die(const char* what) {
    fprintf(stdout, "fuzz: %s: %s\n", what, rtw_last_error());
    exit(2);
}

/* ---- the three worlds ----------------------------------------------------------------------------- */
static rtw_world_handle* demo(const char* name) {
    rtw_world_handle* h = NULL;
    rtw_assets none;
    memset(&none, 0, sizeof none);
    if (rtw_demo_world(name, &none, &h) != RTW_OK) die(name);
    return h;
}

/* a leading image-textured mesh (the triangle prefix), a checker over an image and a solid, a marble, a dielectric,
 * a light rect, a rotated box, a moving sphere and a volume: every table, few leaves */
static rtw_world_handle* prefix_world(void) {
    rtw_builder* b = rtw_builder_new();
    static uint8_t texels[5 * 3 * 3];
    for (size_t i = 0; i < sizeof texels; ++i) texels[i] = (uint8_t)(40 + 13 * i);
    const uint8_t seed[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    rtw_rng* rng = rtw_rng_from_seed(seed);
    const int32_t img = rtw_texture_image_rgb8(b, texels, 5, 3);
    const int32_t solid = rtw_texture_solid(b, 0.8f, 0.7f, 0.2f);
    const int32_t chk = rtw_texture_checker(b, 0.7f, img, solid);
    const int32_t chk2 = rtw_texture_checker(b, 1.3f, chk, solid);
    const int32_t marble = rtw_texture_marble(b, 3.0f, rng);
    const int32_t white = rtw_texture_solid(b, 4.0f, 4.0f, 4.0f);
    float tris[4][24];
    for (int t = 0; t < 4; ++t) {
        const float x = -1.5f + 0.8f * (float)t;
        const float p[9] = {x, 0.1f, 0.0f, x + 0.7f, 0.1f, 0.1f, x + 0.3f, 1.2f, -0.2f};
        const float uv[6] = {0.0f, 0.0f, 1.0f, 0.0f, 0.5f, 1.0f};
        memcpy(tris[t], p, sizeof p);
        for (int v = 0; v < 3; ++v) {
            tris[t][9 + 3 * v] = 0.0f;
            tris[t][10 + 3 * v] = 0.0f;
            tris[t][11 + 3 * v] = 1.0f;
        }
        memcpy(tris[t] + 18, uv, sizeof uv);
    }
    const int32_t g = rtw_node_group(b);
    rtw_node_add(b, g, rtw_node_mesh(b, &tris[0][0], 4, rtw_material_lambert(b, img)));
    int32_t n = rtw_node_sphere(b, 100.0f, rtw_material_lambert(b, chk2));
    rtw_node_translate(b, n, 0.0f, -100.0f, 0.0f);
    rtw_node_add(b, g, n);
    n = rtw_node_sphere(b, 0.4f, rtw_material_metal(b, marble, 0.1f));
    rtw_node_translate(b, n, -0.8f, 0.4f, 1.2f);
    rtw_node_add(b, g, n);
    n = rtw_node_sphere(b, 0.4f, rtw_material_dielectric(b, 1.5f));
    rtw_node_translate(b, n, 0.2f, 0.4f, 1.4f);
    rtw_node_add(b, g, n);
    const float at[3] = {0.0f, 2.5f, 0.5f};
    n = rtw_node_rect(b, RTW_PLANE_XZ, at, 1.5f, 1.5f, rtw_material_diffuse_light(b, white));
    rtw_node_set_all_geo_as_poi(b, n);
    rtw_node_add(b, g, n);
    n = rtw_node_box(b, 0.5f, 0.5f, 0.5f, rtw_material_lambert(b, solid));
    rtw_node_rotate_around_up(b, n, 20.0f);
    rtw_node_translate(b, n, 1.2f, 0.25f, 1.0f);
    rtw_node_add(b, g, n);
    n = rtw_node_sphere(b, 0.25f, rtw_material_lambert(b, solid));
    rtw_node_translate(b, n, -1.6f, 0.25f, 1.8f);
    rtw_node_animate_moving(b, n, 0.0f, 0.3f, 0.0f);
    rtw_node_add(b, g, n);
    n = rtw_node_sphere(b, 0.35f, rtw_material_isotropic(b, solid));
    rtw_node_translate(b, n, 1.9f, 0.35f, 1.9f);
    rtw_node_set_all_geo_density(b, n, 0.8f);
    rtw_node_add(b, g, n);
    rtw_camera_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.fov_mode = 1;
    spec.fov_a = 60.0f;
    spec.fov_b = 1.0f;
    spec.position[0] = 0.2f, spec.position[1] = 1.5f, spec.position[2] = 5.0f;
    spec.look_mode = 1;
    spec.up[1] = 1.0f;
    spec.target[1] = 0.5f;
    spec.time0 = 0.0f, spec.time1 = 1.0f;
    rtw_camera cam;
    if (rtw_camera_build(&spec, &cam) != RTW_OK) die("camera");
    rtw_background bg;
    memset(&bg, 0, sizeof bg);
    bg.kind = RTW_BG_SKY;
    rtw_world_handle* h = NULL;
    if (rtw_builder_finish(b, g, &bg, &cam, &h) != RTW_OK) die("prefix world");
    rtw_rng_free(rng);
    rtw_builder_free(b);
    return h;
}

/* ---- deep copies in exact-size blocks ---------------------------------------------------------------- */
static void* dup_block(const void* p, size_t bytes) {
    if (!bytes) return NULL;
    void* q = malloc(bytes);
    if (!q) exit(3);
    memcpy(q, p, bytes);
    return q;
}
typedef struct copy {
    rtw_world w;
    void* blocks[10];
    uint8_t** texels;
    int32_t n_images; /* allocated, whatever w.image_count becomes */
} copy;
#define TABLE_LIST(X)                                                                                                     \
    X(0, nodes, node_count, rtw_bvh_node) X(1, leaves, leaf_count, rtw_leaf) X(2, spheres, sphere_count, rtw_sphere)      \
    X(3, rects, rect_count, rtw_rect) X(4, boxes, box_count, rtw_box) X(5, triangles, triangle_count, rtw_triangle)      \
    X(6, materials, material_count, rtw_material) X(7, textures, texture_count, rtw_texture)                             \
    X(8, images, image_count, rtw_image) X(9, perlins, perlin_count, rtw_perlin)
static void copy_world(const rtw_world* src, copy* c) {
    c->w = *src;
#define X(i, tab, cnt, typ)                                                           \
    c->blocks[i] = dup_block(src->tab, (size_t)src->cnt * sizeof(typ));               \
    c->w.tab = (const typ*)c->blocks[i];
    TABLE_LIST(X)
#undef X
    c->n_images = src->image_count;
    c->texels = (uint8_t**)calloc((size_t)(c->n_images > 0 ? c->n_images : 1), sizeof(uint8_t*));
    for (int32_t i = 0; i < c->n_images; ++i) {
        rtw_image* im = &((rtw_image*)c->blocks[8])[i];
        c->texels[i] = (uint8_t*)dup_block(im->rgb, (size_t)im->width * (size_t)im->height * 3);
        im->rgb = c->texels[i];
    }
}
static void free_copy(copy* c) {
    for (int i = 0; i < 10; ++i) free(c->blocks[i]);
    for (int32_t i = 0; i < c->n_images; ++i) free(c->texels[i]);
    free(c->texels);
}

/* ---- mutations ----------------------------------------------------------------------------------------- */
static int32_t any_count(const rtw_world* w) {
    const int32_t counts[10] = {w->node_count,     w->leaf_count,     w->sphere_count,  w->rect_count,  w->box_count,
                                w->triangle_count, w->material_count, w->texture_count, w->image_count, w->perlin_count};
    return counts[below(10)];
}
/* the base world's counts: what the blocks hold */
static int32_t mutate_i32(int32_t v, const rtw_world* base) {
    const int32_t c = any_count(base);
    switch (below(8)) {
        case 0: return (int32_t)((uint32_t)v - 1u);
        case 1: return (int32_t)((uint32_t)v + 1u);
        case 2: return 0;
        case 3: return -1;
        case 4: return c;
        case 5: return c + 1;
        case 6: return INT32_MIN;
        default: return INT32_MAX;
    }
}
static int32_t shrink_i32(int32_t v) {
    switch (below(4)) {
        case 0: return 0;
        case 1: return -1;
        case 2: return v > 0 ? v - 1 : v;
        default: return INT32_MIN;
    }
}
static float mutate_f32(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    if (below(4) == 0) {
        const float special[7] = {NAN, INFINITY, -INFINITY, 1073741824.0f, -1073741824.0f, 1073741952.0f, 0.0f};
        return special[below(7)];
    }
    for (int n = 1 + (int)below(3); n > 0; --n) u ^= 1u << below(32);
    memcpy(&v, &u, 4);
    return v;
}
#define MI(field) (field) = mutate_i32((field), base)
#define MF(field) (field) = mutate_f32(field)

/* one random field of the copy; returns the table it touched (0..9, 10: the world's own fields) */
static int mutate(copy* c, const rtw_world* base) {
    rtw_world* w = &c->w;
    const uint32_t t = below(13);
    if (t == 10 || t == 11) { /* the world's own integers, its light, its camera */
        switch (below(10)) {
            case 0: MI(w->root); break;
            case 1: w->root = -1 - (int32_t)below((uint32_t)base->leaf_count + 2u); break;
            case 2: MI(w->has_light); break;
            case 3: MI(w->light.plane); break;
            case 4: MF(w->light.dist); break;
            case 5: MF(w->light.r0[below(2)]); break;
            case 6: MF(w->light.r1[below(2)]); break;
            case 7: MF(w->camera.position[below(3)]); break;
            case 8:
                if (below(2)) MF(w->camera.time0);
                else MF(w->camera.time1);
                break;
            default: MF(w->camera.shutter_pace[below(2)]); break;
        }
        return 10;
    }
    if (t == 12) { /* a count shrinks, or a pointer goes */
        const uint32_t k = below(10);
        const int null_it = (int)below(3) == 0;
        switch (k) {
#define X(i, tab, cnt, typ)                     \
    case i:                                     \
        if (null_it) w->tab = NULL;             \
        else w->cnt = shrink_i32(w->cnt);       \
        break;
            TABLE_LIST(X)
#undef X
        }
        return (int)k;
    }
    /* a field of a random element of table t (an empty table: the root instead) */
    switch (t) {
        case 0: {
            if (base->node_count < 1) break;
            rtw_bvh_node* n = &((rtw_bvh_node*)c->blocks[0])[below((uint32_t)base->node_count)];
            switch (below(5)) {
                case 0: MI(n->axis); break;
                case 1: MI(n->left); break;
                case 2: MI(n->right); break;
                case 3: MF(n->min[below(3)]); break;
                default: MF(n->max[below(3)]); break;
            }
            return 0;
        }
        case 1: {
            rtw_leaf* l = &((rtw_leaf*)c->blocks[1])[below((uint32_t)base->leaf_count)];
            switch (below(9)) {
                case 0: MI(l->geom_kind); break;
                case 1: MI(l->geom_index); break;
                case 2: MI(l->material); break;
                case 3: l->flags = (uint32_t)mutate_i32((int32_t)l->flags, base); break;
                case 4: l->flags ^= 1u << below(4); break;
                case 5: MF(l->neg_inv_density); break;
                case 6: MF(l->offset[below(3)]); break;
                case 7:
                    if (below(2)) MF(l->y_sin);
                    else MF(l->y_cos);
                    break;
                default: MF(l->velocity[below(3)]); break;
            }
            return 1;
        }
        case 2: {
            if (base->sphere_count < 1) break;
            rtw_sphere* s = &((rtw_sphere*)c->blocks[2])[below((uint32_t)base->sphere_count)];
            if (below(4) == 0) MF(s->radius);
            else MF(s->center[below(3)]);
            return 2;
        }
        case 3: {
            if (base->rect_count < 1) break;
            rtw_rect* r = &((rtw_rect*)c->blocks[3])[below((uint32_t)base->rect_count)];
            switch (below(4)) {
                case 0: MI(r->plane); break;
                case 1: MF(r->dist); break;
                case 2: MF(r->r0[below(2)]); break;
                default: MF(r->r1[below(2)]); break;
            }
            return 3;
        }
        case 4: {
            if (base->box_count < 1) break;
            rtw_box* b = &((rtw_box*)c->blocks[4])[below((uint32_t)base->box_count)];
            if (below(2)) MF(b->min[below(3)]);
            else MF(b->max[below(3)]);
            return 4;
        }
        case 5: {
            if (base->triangle_count < 1) break;
            rtw_triangle* tr = &((rtw_triangle*)c->blocks[5])[below((uint32_t)base->triangle_count)];
            switch (below(3)) {
                case 0: MF(tr->positions[below(3)][below(3)]); break;
                case 1: MF(tr->normals[below(3)][below(3)]); break;
                default: MF(tr->uvs[below(3)][below(2)]); break;
            }
            return 5;
        }
        case 6: {
            rtw_material* m = &((rtw_material*)c->blocks[6])[below((uint32_t)base->material_count)];
            switch (below(4)) {
                case 0: MI(m->kind); break;
                case 1: MI(m->texture); break;
                case 2: MF(m->fuzz); break;
                default: MF(m->index_of_refraction); break;
            }
            return 6;
        }
        case 7: {
            rtw_texture* x = &((rtw_texture*)c->blocks[7])[below((uint32_t)base->texture_count)];
            switch (below(9)) {
                case 0: MI(x->kind); break;
                case 1: x->kind = (int32_t)below(4); break; /* a valid kind over the other kinds' fields */
                case 2: MI(x->even); break;
                case 3: MI(x->odd); break;
                case 4: MI(x->perlin); break;
                case 5: MI(x->image); break;
                case 6: MF(x->color[below(3)]); break;
                case 7: MF(x->inv_frequency); break;
                default: MF(x->scale); break;
            }
            return 7;
        }
        case 8: {
            if (base->image_count < 1) break;
            rtw_image* im = &((rtw_image*)c->blocks[8])[below((uint32_t)base->image_count)];
            switch (below(3)) {
                case 0: im->width = shrink_i32(im->width); break;
                case 1: im->height = shrink_i32(im->height); break;
                default: im->rgb = NULL; break;
            }
            return 8;
        }
        default: {
            if (base->perlin_count < 1) break;
            rtw_perlin* p = &((rtw_perlin*)c->blocks[9])[below((uint32_t)base->perlin_count)];
            uint32_t* perms[3] = {p->perm_x, p->perm_y, p->perm_z};
            switch (below(4)) {
                case 0: MI(p->bits); break;
                case 1: p->bits = 1 + (int32_t)below(8); break; /* a smaller lattice over the same entries */
                case 2: perms[below(3)][below(256)] = (uint32_t)mutate_i32((int32_t)perms[0][below(256)], base); break;
                default: MF(p->ranvec[below(256)][below(3)]); break;
            }
            return 9;
        }
    }
    MI(w->root);
    return 10;
}

int main(int argc, char** argv) {
    const long mutants = argc > 1 ? atol(argv[1]) : 1000;
    g_state = argc > 2 ? (uint64_t)strtoull(argv[2], NULL, 10) : 1u;
    rtw_world_handle* handles[3] = {demo("cornell_box_smoke"), demo("perlin_spheres"), prefix_world()};
    rtw_render_params p;
    memset(&p, 0, sizeof p);
    p.width = 8, p.height = 8, p.samples_per_pixel = 2, p.max_depth = 8, p.seed = 5;
    float image[8 * 8 * 3];
    for (int k = 0; k < 3; ++k) { /* the worlds themselves are accepted and render */
        int32_t depth = -1;
        if (rtw_world_check(rtw_world_get(handles[k]), &depth) != RTW_OK) die("a base world is refused");
        if (rtw_oracle_render(rtw_world_get(handles[k]), &p, RTW_ORACLE_RNG_CTR, 1, image, NULL) != RTW_OK) die("oracle");
    }
    long refused = 0, accepted = 0, rendered = 0, unsupported = 0;
    long refused_by[11] = {0}, accepted_by[11] = {0};
    for (long i = 0; i < mutants; ++i) {
        const rtw_world* base = rtw_world_get(handles[i % 3]);
        copy c;
        copy_world(base, &c);
        int where = mutate(&c, base);
        if (below(3) == 0) mutate(&c, base); /* a second field */
        int32_t depth = -1;
        const int rc = rtw_world_check(&c.w, &depth);
        if (argc > 3) {
            printf("%ld world %ld table %d: %s\n", i, i % 3, where, rc == RTW_OK ? "accepted" : rtw_last_error());
            fflush(stdout);
        }
        if (rc == RTW_OK) {
            ++accepted;
            ++accepted_by[where];
            if (rtw_oracle_render(&c.w, &p, RTW_ORACLE_RNG_CTR, 1, image, NULL) == RTW_OK) ++rendered;
        } else {
            if (rc != RTW_ERR_INVALID_ARGUMENT && rc != RTW_ERR_UNSUPPORTED) die("an unexpected code");
            if (strncmp(rtw_last_error(), "invalid world: ", 15) != 0) die("a refusal without its message");
            unsupported += rc == RTW_ERR_UNSUPPORTED;
            ++refused;
            ++refused_by[where];
        }
        free_copy(&c);
    }
    static const char* names[11] = {"nodes",     "leaves",   "spheres", "rects",   "boxes", "triangles",
                                    "materials", "textures", "images",  "perlins", "world"};
    for (int k = 0; k < 11; ++k) printf("%-10s refused %5ld accepted %5ld\n", names[k], refused_by[k], accepted_by[k]);
    printf("unsupported %ld\n", unsupported);
    printf("mutants %ld refused %ld accepted %ld rendered %ld\n", mutants, refused, accepted, rendered);
    for (int k = 0; k < 3; ++k) rtw_world_free(handles[k]);
    return 0;
}
