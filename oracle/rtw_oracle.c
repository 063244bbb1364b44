/*
 * rtw_oracle.c -- TEST INFRASTRUCTURE: plain-C restatement of the reference render loop.
 *
 * Follows /root/reference/src/lib line by line (cited per function), in the reference's own
 * structure: AoS records, recursive BVH descent, hit records built eagerly for every candidate.
 * The device kernel (raytracinginaweekend_amd/csrc/rtw_device.hip) is a separate, iterative,
 * SoA implementation; the GPU parity tests require both to produce identical f32 images in the
 * "ctr" RNG mode.  Numerics shared by both sides are in include/rtw_scalar.h.
 *
 * Build: oracle/Makefile (gcc -O2 -ffp-contract=off, no fast-math).
 * Parity unpinned against the Rust binary (see rtw_oracle.h).
 */
#include "rtw_oracle.h"

#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "../include/rtw_scalar.h"
#include "../include/rtw_cull.h"

#define F32_PI 3.14159274101257324219f  /* std::f32::consts::PI */
#define F32_TAU 6.28318548202514648438f /* std::f32::consts::TAU */
#define F32_INF (__builtin_inff())

/* ------------------------------------------------------------------------------------------ */
/* vec3.rs / math.rs / color.rs                                                                */
/* ------------------------------------------------------------------------------------------ */
typedef struct V3 {
    float e[3];
} V3;

static inline V3 v3(float x, float y, float z) {
    V3 r = {{x, y, z}};
    return r;
}
static inline V3 vadd(V3 a, V3 b) { return v3(a.e[0] + b.e[0], a.e[1] + b.e[1], a.e[2] + b.e[2]); }
static inline V3 vsub(V3 a, V3 b) { return v3(a.e[0] - b.e[0], a.e[1] - b.e[1], a.e[2] - b.e[2]); }
static inline V3 vneg(V3 a) { return v3(-a.e[0], -a.e[1], -a.e[2]); }
/* vec3.rs:60-66: v * f (also f * v, vec3.rs:300-305, which forwards to v * f) */
static inline V3 vmul(V3 a, float s) { return v3(a.e[0] * s, a.e[1] * s, a.e[2] * s); }
/* vec3.rs:76-82 */
static inline V3 vdiv(V3 a, float s) { return v3(a.e[0] / s, a.e[1] / s, a.e[2] / s); }
/* color.rs:58-64 convolution */
static inline V3 vconv(V3 a, V3 b) { return v3(a.e[0] * b.e[0], a.e[1] * b.e[1], a.e[2] * b.e[2]); }
/* vec3.rs:191-193 */
static inline float vdot(V3 a, V3 b) { return a.e[0] * b.e[0] + a.e[1] * b.e[1] + a.e[2] * b.e[2]; }
/* vec3.rs:195-203 */
static inline V3 vcross(V3 a, V3 b) {
    return v3(a.e[1] * b.e[2] - a.e[2] * b.e[1], a.e[2] * b.e[0] - a.e[0] * b.e[2],
              a.e[0] * b.e[1] - a.e[1] * b.e[0]);
}
static inline float vlength(V3 a) { return sqrtf(vdot(a, a)); }
/* vec3.rs:205-210: unit() = with_length(1.0) = self * (length / self.length()) */
static inline V3 vwith_length(V3 a, float len) { return vmul(a, len / vlength(a)); }
static inline V3 vunit(V3 a) { return vwith_length(a, 1.0f); }
/* vec3.rs:223-230 */
static inline V3 vunit_or_else(V3 a, V3 def) {
    const float len_sq = vdot(a, a);
    if (len_sq > 1e-8f) return vdiv(a, sqrtf(len_sq));
    return def;
}
/* vec3.rs:232-234 */
static inline V3 vreflect(V3 ray, V3 n) { return vsub(ray, vmul(n, 2.0f * vdot(ray, n))); }
/* vec3.rs:235-240 */
static inline V3 vrefract(V3 ray, V3 n, float eta) {
    const float cos_theta = rtw_minr(vdot(vneg(ray), n), 1.0f);
    const V3 perp = vmul(vadd(ray, vmul(n, cos_theta)), eta);
    const float k = -sqrtf(fabsf(1.0f - vdot(perp, perp)));
    const V3 par = vmul(n, k);
    return vadd(perp, par);
}
/* vec3.rs:241-249 to_radian -> (phi/TAU, theta/PI) */
static inline void vto_radian(V3 a, float* u, float* v) {
    const float theta = rtw_acosf(a.e[1]);
    const float phi = rtw_atan2f(-a.e[2], a.e[0]) + F32_PI;
    *u = phi / F32_TAU;
    *v = theta / F32_PI;
}
static inline V3 vload(const float* p) { return v3(p[0], p[1], p[2]); }

typedef struct Ray {
    V3 origin, dir;
    float time;
} Ray;
/* ray.rs:21-23 */
static inline V3 ray_at(const Ray* r, float t) { return vadd(r->origin, vmul(r->dir, t)); }
/* Range<f32>::contains */
static inline int contains(float start, float end, float t) { return start <= t && t < end; }

/* ------------------------------------------------------------------------------------------ */
/* statistics                                                                                 */
/* ------------------------------------------------------------------------------------------ */
typedef struct Stats {
    uint64_t rays, node_visits, tests[4], hits[4], material_reads, texel_reads, samples;
} Stats;

typedef struct Ctx {
    const rtw_world* w;
    rtw_xoro* rng;
    Stats* st; /* may be NULL */
    const float* km; /* proximity-cull node constants (rtw_cull.h), NULL = reference traversal */
} Ctx;

/* ------------------------------------------------------------------------------------------ */
/* hit records (hittable.rs:24-102)                                                            */
/* ------------------------------------------------------------------------------------------ */
typedef struct Hit {
    V3 position, normal;
    float u, v, t;
    int front_face;
    int material;
} Hit;

/* GeoHitInteraction::new_from_ray (hittable.rs:34-54) */
static inline void hit_from_ray(Hit* h, const Ray* r, V3 pos, V3 sn, float t, float u, float v) {
    h->front_face = vdot(sn, r->dir) < 0.0f;
    h->normal = h->front_face ? sn : vneg(sn);
    h->position = pos;
    h->t = t;
    h->u = u;
    h->v = v;
}

/* sphere_geometry.rs:21-54 */
static int sphere_hit(const rtw_sphere* s, const Ray* r, float ts, float te, Hit* h) {
    const V3 center = vload(s->center);
    const V3 oc = vsub(r->origin, center);
    const float half_b = vdot(oc, r->dir);
    const float c = vdot(oc, oc) - s->radius * s->radius;
    const float disc = half_b * half_b - c;
    if (disc < 0.0f) return 0;
    const float sqrtd = sqrtf(disc);
    const float root_small = -half_b - sqrtd;
    float t;
    if (contains(ts, te, root_small)) {
        t = root_small;
    } else {
        const float root_large = -half_b + sqrtd;
        if (contains(ts, te, root_large)) t = root_large;
        else return 0;
    }
    const V3 pos = ray_at(r, t);
    const V3 sn = vdiv(vsub(pos, center), s->radius);
    float u, v;
    vto_radian(sn, &u, &v); /* get_sphere_uv, sphere_geometry.rs:56-59 */
    hit_from_ray(h, r, pos, sn, t, u, v);
    return 1;
}

static inline void rect_axes(int plane, int* p0, int* p1, int* n) {
    /* rect_geometry.rs:14-21 */
    if (plane == RTW_PLANE_XY) { *p0 = 0; *p1 = 1; *n = 2; }
    else if (plane == RTW_PLANE_XZ) { *p0 = 0; *p1 = 2; *n = 1; }
    else { *p0 = 1; *p1 = 2; *n = 0; }
}

/* rect_geometry.rs:33-59 (uv.y denominator typo `r0.1 - r1.0` kept, :45) */
static int rect_hit(const rtw_rect* g, const Ray* r, float ts, float te, Hit* h) {
    int p0, p1, n;
    rect_axes(g->plane, &p0, &p1, &n);
    const float t = (g->dist - r->origin.e[n]) / r->dir.e[n];
    if (!contains(ts, te, t)) return 0;
    const V3 pos = vadd(r->origin, vmul(r->dir, t));
    if (pos.e[p0] >= g->r0[0] && pos.e[p0] <= g->r0[1] && pos.e[p1] >= g->r1[0] &&
        pos.e[p1] <= g->r1[1]) {
        const float u = (pos.e[p0] - g->r0[0]) / (g->r0[1] - g->r0[0]);
        const float v = (pos.e[p1] - g->r1[0]) / (g->r0[1] - g->r1[0]);
        V3 sn = v3(0.0f, 0.0f, 0.0f);
        sn.e[n] = -1.0f;
        hit_from_ray(h, r, pos, sn, t, u, v);
        return 1;
    }
    return 0;
}

/* aabb.rs:103-167 */
static int box_intersections_line(const rtw_box* b, V3 origin, V3 dir, float* near_t,
                                  int* near_plane, float* far_t, int* far_plane) {
    const V3 mn = vsub(vload(b->min), origin);
    const V3 mx = vsub(vload(b->max), origin);
    float near = -F32_INF, far = F32_INF;
    int np = 0, fp = 0;
    for (int a = 0; a < 3; ++a) {
        const float t1 = mn.e[a] / dir.e[a];
        const float t2 = mx.e[a] / dir.e[a];
        const float t_min = rtw_minr(t1, t2);
        const float t_max = rtw_maxr(t1, t2);
        if (t_min > near) { near = t_min; np = a; }
        if (t_max < far) { far = t_max; fp = a; }
        if (near > far || far < 0.0f) return 0;
    }
    *near_t = near; *near_plane = np; *far_t = far; *far_plane = fp;
    return 1;
}

/* aabb.rs:80-102 */
static int box_hit(const rtw_box* b, const Ray* r, float ts, float te, Hit* h) {
    float nt, ft;
    int np, fp;
    if (!box_intersections_line(b, r->origin, r->dir, &nt, &np, &ft, &fp)) return 0;
    float t;
    int plane;
    if (contains(ts, te, nt)) { t = nt; plane = np; }
    else if (contains(ts, te, ft)) { t = ft; plane = fp; }
    else return 0;
    const V3 pos = vadd(r->origin, vmul(r->dir, t));
    const float center = (b->max[plane] + b->min[plane]) * 0.5f;
    V3 sn = v3(0.0f, 0.0f, 0.0f);
    sn.e[plane] = rtw_signum(pos.e[plane] - center);
    hit_from_ray(h, r, pos, sn, t, 0.0f, 0.0f);
    return 1;
}

/* triangle_geometry.rs:13-45 (normal is the un-normalised barycentric interpolation) */
static int triangle_hit(const rtw_triangle* g, const Ray* r, float ts, float te, Hit* h) {
    const V3 p0 = vload(g->positions[0]), p1 = vload(g->positions[1]), p2 = vload(g->positions[2]);
    const V3 dir1 = vsub(p1, p0);
    const V3 dir2 = vsub(p2, p0);
    const V3 normal = vunit(vcross(dir1, dir2));
    const float denom = vdot(r->dir, normal);
    if (fabsf(denom) > 0.0001f) {
        const float t = vdot(vsub(p0, r->origin), normal) / denom;
        if (contains(ts, te, t)) {
            const V3 pos = ray_at(r, t);
            const V3 q = vsub(pos, p0);
            V3 vt = vcross(normal, dir2);
            const float w1 = vdot(q, vt) / vdot(dir1, vt);
            if (w1 > 0.0f && w1 < 1.0f) {
                vt = vcross(normal, dir1);
                const float w2 = vdot(q, vt) / vdot(dir2, vt);
                const float w0 = 1.0f - w1 - w2;
                if (w2 > 0.0f && w0 > 0.0f) {
                    /* math.rs:9-16 interpolate: v0*w0 + v1*w1 + v2*w2 */
                    const float u = g->uvs[0][0] * w0 + g->uvs[1][0] * w1 + g->uvs[2][0] * w2;
                    const float v = g->uvs[0][1] * w0 + g->uvs[1][1] * w1 + g->uvs[2][1] * w2;
                    const V3 sn = vadd(vadd(vmul(vload(g->normals[0]), w0),
                                            vmul(vload(g->normals[1]), w1)),
                                       vmul(vload(g->normals[2]), w2));
                    hit_from_ray(h, r, pos, sn, t, u, v);
                    return 1;
                }
            }
        }
    }
    return 0;
}

/* Geometry::hit (hittable.rs:141-148) */
static int geometry_hit(const Ctx* c, int kind, int idx, const Ray* r, float ts, float te, Hit* h) {
    const rtw_world* w = c->w;
    if (c->st) c->st->tests[kind]++;
    switch (kind) {
        case RTW_GEOM_SPHERE: return sphere_hit(&w->spheres[idx], r, ts, te, h);
        case RTW_GEOM_RECT: return rect_hit(&w->rects[idx], r, ts, te, h);
        case RTW_GEOM_BOX: return box_hit(&w->boxes[idx], r, ts, te, h);
        default: return triangle_hit(&w->triangles[idx], r, ts, te, h);
    }
}

/* ------------------------------------------------------------------------------------------ */
/* transformations.rs                                                                          */
/* ------------------------------------------------------------------------------------------ */
typedef struct Xf {
    V3 offset;
    float ys, yc;
} Xf;
/* transformations.rs:107-111 */
static inline V3 rotate_around_up(float c, float s, V3 v) {
    const float x = v.e[0], y = v.e[2];
    V3 r = v;
    r.e[0] = c * x + s * y;
    r.e[2] = -s * x + c * y;
    return r;
}
/* :49-56 */
static inline V3 xf_reverse_point(const Xf* x, V3 p) { return rotate_around_up(x->yc, -x->ys, vsub(p, x->offset)); }
static inline V3 xf_reverse_normal(const Xf* x, V3 d) { return rotate_around_up(x->yc, -x->ys, d); }
/* :37-43 */
static inline V3 xf_apply_point(const Xf* x, V3 p) { return vadd(rotate_around_up(x->yc, x->ys, p), x->offset); }
static inline V3 xf_apply_normal(const Xf* x, V3 d) { return rotate_around_up(x->yc, x->ys, d); }
/* hittable.rs:271-283 */
static inline Ray xf_reverse_ray(const Xf* x, const Ray* r) {
    Ray o;
    o.origin = xf_reverse_point(x, r->origin);
    o.dir = xf_reverse_normal(x, r->dir);
    o.time = r->time;
    return o;
}
static inline void xf_apply_hit(const Xf* x, Hit* h) {
    h->position = xf_apply_point(x, h->position);
    h->normal = xf_apply_normal(x, h->normal);
}

/* ------------------------------------------------------------------------------------------ */
/* SceneElement::hit for one flattened leaf (hittable.rs:212-247, 309-341)                     */
/* ------------------------------------------------------------------------------------------ */
/* VolumeGeometry::hit (hittable.rs:309-341) */
static int volume_hit(const Ctx* c, const rtw_leaf* L, const Ray* r, float ts, float te, Hit* h) {
    Hit tmp;
    if (!geometry_hit(c, L->geom_kind, L->geom_index, r, -F32_INF, F32_INF, &tmp)) return 0;
    const float start_boundary = tmp.t;
    const float next = start_boundary + 0.001f;
    if (!geometry_hit(c, L->geom_kind, L->geom_index, r, next, F32_INF, &tmp)) return 0;
    const float end_boundary = tmp.t;
    const float start_medium = rtw_maxr(start_boundary, ts);
    const float end_medium = rtw_minr(end_boundary, te);
    if (start_medium >= end_medium) return 0;
    const float t = rtw_maxr(start_medium, 0.0f) + L->neg_inv_density * rtw_logf(rtw_gen_f32(c->rng));
    if (t > end_medium) return 0;
    h->position = ray_at(r, t);
    h->normal = v3(0.0f, 1.0f, 0.0f);
    h->u = 0.0f;
    h->v = 0.0f;
    h->t = t;
    h->front_face = 0;
    return 1;
}

static int surface_or_volume_hit(const Ctx* c, const rtw_leaf* L, const Ray* r, float ts, float te,
                                 Hit* h) {
    int ok;
    if (L->flags & RTW_LEAF_VOLUME) ok = volume_hit(c, L, r, ts, te, h);
    else ok = geometry_hit(c, L->geom_kind, L->geom_index, r, ts, te, h);
    if (ok) h->material = L->material;
    return ok;
}

static int transform_level_hit(const Ctx* c, const rtw_leaf* L, const Ray* r, float ts, float te,
                               Hit* h) {
    if (!(L->flags & RTW_LEAF_TRANSFORM)) return surface_or_volume_hit(c, L, r, ts, te, h);
    /* SceneElement::Transformation (hittable.rs:234-238) */
    Xf x;
    x.offset = vload(L->offset);
    x.ys = L->y_sin;
    x.yc = L->y_cos;
    const Ray rt = xf_reverse_ray(&x, r);
    if (!surface_or_volume_hit(c, L, &rt, ts, te, h)) return 0;
    xf_apply_hit(&x, h);
    return 1;
}

static int leaf_hit(const Ctx* c, int leaf, const Ray* r, float ts, float te, Hit* h) {
    const rtw_leaf* L = &c->w->leaves[leaf];
    if (!(L->flags & RTW_LEAF_ANIMATION)) return transform_level_hit(c, L, r, ts, te, h);
    /* SceneElement::Animation (hittable.rs:239-244): ZERO.translate(velocity * ray.time) */
    Xf x;
    const V3 vt = vmul(vload(L->velocity), r->time);
    x.offset = v3(0.0f + vt.e[0], 0.0f + vt.e[1], 0.0f + vt.e[2]);
    x.ys = 0.0f;
    x.yc = 1.0f;
    const Ray rt = xf_reverse_ray(&x, r);
    if (!transform_level_hit(c, L, &rt, ts, te, h)) return 0;
    xf_apply_hit(&x, h);
    return 1;
}

/* ------------------------------------------------------------------------------------------ */
/* BoundingVolumeHierarchy (hittable.rs:429-473) and Aabb::hit_cond (aabb.rs:65-78)            */
/* ------------------------------------------------------------------------------------------ */
static int aabb_hit_cond(const rtw_bvh_node* nd, const Ray* r, float ts, float te) {
    for (int i = 0; i < 3; ++i) {
        const float a = (nd->min[i] - r->origin.e[i]) / r->dir.e[i];
        const float b = (nd->max[i] - r->origin.e[i]) / r->dir.e[i];
        /* math.rs:35-41 minmax */
        const float t0 = (a < b) ? a : b;
        const float t1 = (a < b) ? b : a;
        const float t_min = rtw_maxr(t0, ts);
        const float t_max = rtw_minr(t1, te);
        if (t_max <= t_min) return 0;
    }
    return 1;
}

/* The product's extra proximity test (rtw_scalar.h rtw_cull_*; NOT part of the reference):
 * RTW_ORACLE_CULL mode applies it after hit_cond to check, on the CPU, that it changes no
 * result and to count the culled traversal's work. */
static int cull_pass(const float* km, int32_t n, const rtw_bvh_node* nd, const Ray* r, float ts, float te) {
    float ab[6], t0[3], t1[3];
    for (int i = 0; i < 3; ++i) {
        const float a = nd->min[i] - r->origin.e[i];
        const float b = nd->max[i] - r->origin.e[i];
        ab[2 * i] = a;
        ab[2 * i + 1] = b;
        const float qa = a / r->dir.e[i], qb = b / r->dir.e[i];
        t0[i] = (qa < qb) ? qa : qb;
        t1[i] = (qa < qb) ? qb : qa;
    }
    const float delta = rtw_cull_delta(km[2 * (size_t)n], km[2 * (size_t)n + 1], ab[0], ab[1], ab[2], ab[3], ab[4], ab[5]);
    float lo = ts, hi = te;
    for (int i = 0; i < 3; ++i) rtw_cull_axis(t0[i], t1[i], delta * fabsf(1.0f / r->dir.e[i]), &lo, &hi);
    return lo <= hi;
}

/* ------------------------------------------------------------------------------------------ */
/* texture.rs + perlin.rs                                                                      */
/* ------------------------------------------------------------------------------------------ */
/* perlin.rs:48-91 */
static float perlin_noise(const rtw_perlin* P, V3 p) {
    const int32_t mask = (int32_t)((1u << P->bits) - 1u);
    const float u = p.e[0] - floorf(p.e[0]);
    const float v = p.e[1] - floorf(p.e[1]);
    const float w = p.e[2] - floorf(p.e[2]);
    const int32_t i = rtw_f2i32_sat(floorf(p.e[0]));
    const int32_t j = rtw_f2i32_sat(floorf(p.e[1]));
    const int32_t k = rtw_f2i32_sat(floorf(p.e[2]));
    const float uu = u * u * (3.0f - 2.0f * u);
    const float vv = v * v * (3.0f - 2.0f * v);
    const float ww = w * w * (3.0f - 2.0f * w);
    V3 cc[2][2][2];
    for (int di = 0; di < 2; ++di)
        for (int dj = 0; dj < 2; ++dj)
            for (int dk = 0; dk < 2; ++dk) {
                const uint32_t ix = (uint32_t)(((uint32_t)i + (uint32_t)di) & (uint32_t)mask);
                const uint32_t jx = (uint32_t)(((uint32_t)j + (uint32_t)dj) & (uint32_t)mask);
                const uint32_t kx = (uint32_t)(((uint32_t)k + (uint32_t)dk) & (uint32_t)mask);
                const uint32_t rr = P->perm_x[ix] ^ P->perm_y[jx] ^ P->perm_z[kx];
                cc[di][dj][dk] = vload(P->ranvec[rr]);
            }
    float accum = 0.0f;
    for (int a = 0; a < 2; ++a) {
        const float fi = (float)a;
        for (int b = 0; b < 2; ++b) {
            const float fj = (float)b;
            for (int d = 0; d < 2; ++d) {
                const float fk = (float)d;
                const V3 weight = v3(u - (float)a, v - (float)b, w - (float)d);
                accum += (fi * uu + (1.0f - fi) * (1.0f - uu)) * (fj * vv + (1.0f - fj) * (1.0f - vv)) *
                         (fk * ww + (1.0f - fk) * (1.0f - ww)) * vdot(cc[a][b][d], weight);
            }
        }
    }
    return accum;
}
/* perlin.rs:37-47 */
static float perlin_turbulence(const rtw_perlin* P, V3 p, int depth, float fall_off) {
    float accum = 0.0f, weight = 1.0f;
    for (int i = 0; i < depth; ++i) {
        accum += weight * perlin_noise(P, p);
        weight *= fall_off;
        p = vmul(p, 2.0f);
    }
    return fabsf(accum);
}

/* Texture::sample (texture.rs:23-53) */
static V3 texture_sample(const Ctx* c, int tex, const Hit* h) {
    const rtw_world* w = c->w;
    for (;;) {
        const rtw_texture* T = &w->textures[tex];
        switch (T->kind) {
            case RTW_TEX_SOLID: return vload(T->color);
            case RTW_TEX_CHECKER: {
                const V3 s = vmul(h->position, T->inv_frequency);
                const float sines = rtw_sinf(s.e[0]) * rtw_sinf(s.e[1]) * rtw_sinf(s.e[2]);
                tex = (sines < 0.0f) ? T->even : T->odd;
                continue;
            }
            case RTW_TEX_IMAGE: {
                const rtw_image* I = &w->images[T->image];
                uint32_t pu = rtw_f2u32_sat(h->u * (float)I->width);
                uint32_t pv = rtw_f2u32_sat(h->v * (float)I->height);
                if (pu > (uint32_t)(I->width - 1)) pu = (uint32_t)(I->width - 1);
                if (pv > (uint32_t)(I->height - 1)) pv = (uint32_t)(I->height - 1);
                if (c->st) c->st->texel_reads++;
                const uint8_t* px = I->rgb + ((size_t)pv * (size_t)I->width + pu) * 3u;
                /* color.rs:29-35 new_rgb8 */
                return v3((float)px[0] / 255.0f, (float)px[1] / 255.0f, (float)px[2] / 255.0f);
            }
            default: { /* Marble */
                const float turb = perlin_turbulence(&w->perlins[T->perlin], h->position, 7, 0.5f);
                const float k = 1.0f + rtw_sinf(h->position.e[2] * T->scale + 10.0f * turb);
                const V3 half = vmul(v3(1.0f, 1.0f, 1.0f), 0.5f);
                return vmul(half, k);
            }
        }
    }
}

/* ------------------------------------------------------------------------------------------ */
/* material.rs                                                                                 */
/* ------------------------------------------------------------------------------------------ */
#define DIST_COSINE 0
#define DIST_MIRROR 1
typedef struct Dist {
    int kind;
    V3 v; /* normal (cosine) or direction (mirror) */
} Dist;

/* MaterialScatteringDistribution::generate / value (material.rs:17-40) */
static V3 dist_generate(const Dist* d, rtw_xoro* rng) {
    if (d->kind == DIST_MIRROR) return d->v;
    float s[3];
    rtw_unit_sphere(rng, s);
    return vunit_or_else(vadd(d->v, v3(s[0], s[1], s[2])), d->v);
}
static float dist_value(const Dist* d, V3 dir) {
    if (d->kind == DIST_MIRROR) return F32_INF;
    return rtw_maxr(vdot(d->v, dir), 0.0f) / F32_PI;
}

/* Material::scatter (material.rs:52-114); returns 0 for no scatter */
static int material_scatter(const Ctx* c, const rtw_material* M, const Ray* r, const Hit* h, V3* att,
                            Dist* dist) {
    switch (M->kind) {
        case RTW_MAT_LAMBERT:
            *att = texture_sample(c, M->texture, h);
            dist->kind = DIST_COSINE;
            dist->v = h->normal;
            return 1;
        case RTW_MAT_METAL: {
            V3 fuzz_dir = v3(0.0f, 0.0f, 0.0f);
            if (M->fuzz > 0.0f) {
                float b[3];
                rtw_unit_ball(c->rng, b);
                fuzz_dir = vmul(v3(b[0], b[1], b[2]), M->fuzz);
            }
            const V3 direction = vadd(vreflect(r->dir, h->normal), fuzz_dir);
            if (vdot(direction, h->normal) > 0.0f) {
                dist->kind = DIST_MIRROR;
                dist->v = vunit(direction);
                *att = texture_sample(c, M->texture, h);
                return 1;
            }
            return 0;
        }
        case RTW_MAT_DIELECTRIC: {
            const float ior = M->index_of_refraction;
            const float ratio = h->front_face ? (1.0f / ior) : ior;
            const float cos_theta = rtw_minr(vdot(vneg(r->dir), h->normal), 1.0f);
            const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
            const int cannot_refract = ratio * sin_theta > 1.0f;
            int reflect = cannot_refract;
            if (!reflect) {
                /* reflectance (material.rs:83-87); powi(5) = x * ((x*x) * (x*x)) */
                const float r0 = (1.0f - ratio) / (1.0f + ratio);
                const float rs = r0 * r0;
                const float x = 1.0f - cos_theta;
                const float x2 = x * x;
                const float p5 = x * (x2 * x2);
                const float refl = rs + (1.0f - rs) * p5;
                reflect = refl > rtw_gen_f32(c->rng);
            }
            const V3 direction = reflect ? vreflect(r->dir, h->normal) : vrefract(r->dir, h->normal, ratio);
            dist->kind = DIST_MIRROR;
            dist->v = vunit(direction);
            *att = v3(1.0f, 1.0f, 1.0f);
            return 1;
        }
        case RTW_MAT_ISOTROPIC: {
            float s[3];
            rtw_unit_sphere(c->rng, s);
            dist->kind = DIST_MIRROR;
            dist->v = v3(s[0], s[1], s[2]);
            *att = texture_sample(c, M->texture, h);
            return 1;
        }
        default: return 0; /* DiffuseLight */
    }
}
/* material.rs:116-130 */
static float material_scattering_pdf(const rtw_material* M, const Ray* scattered, const Hit* h) {
    if (M->kind == RTW_MAT_LAMBERT) {
        const float cosine = vdot(h->normal, scattered->dir);
        return rtw_maxr(cosine, 0.0f) / F32_PI;
    }
    return 0.0f;
}
/* material.rs:132-137 */
static V3 material_emit(const Ctx* c, const rtw_material* M, const Hit* h) {
    if (M->kind == RTW_MAT_DIFFUSE_LIGHT) return texture_sample(c, M->texture, h);
    return v3(0.0f, 0.0f, 0.0f);
}

/* ------------------------------------------------------------------------------------------ */
/* world_scattering_distribution.rs + rect_geometry.rs:60-85                                   */
/* ------------------------------------------------------------------------------------------ */
static V3 light_generate(const rtw_rect* g, V3 origin, rtw_xoro* rng) {
    int p0, p1, n;
    rect_axes(g->plane, &p0, &p1, &n);
    V3 e = v3(0.0f, 0.0f, 0.0f);
    e.e[p0] = rtw_gen_range_f32(g->r0[0], g->r0[1], rng);
    e.e[p1] = rtw_gen_range_f32(g->r1[0], g->r1[1], rng);
    e.e[n] = g->dist;
    return vunit(vsub(e, origin));
}
static float light_value(const rtw_rect* g, V3 origin, V3 dir) {
    Ray r;
    r.origin = origin;
    r.dir = dir;
    r.time = 0.0f;
    Hit h;
    if (rect_hit(g, &r, 0.001f, F32_INF, &h)) {
        const float area = (g->r0[1] - g->r0[0]) * (g->r1[1] - g->r1[0]);
        const float dsq = h.t * h.t;
        const float cosine = fabsf(vdot(h.normal, dir));
        return dsq / (cosine * area);
    }
    return 0.0f;
}

/* ------------------------------------------------------------------------------------------ */
/* background_color.rs:9-19                                                                    */
/* ------------------------------------------------------------------------------------------ */
static V3 background_sample(const rtw_background* bg, const Ray* r) {
    if (bg->kind == RTW_BG_SKY) {
        const float t = 0.5f * (vdot(v3(0.0f, 1.0f, 0.0f), r->dir) + 1.0f);
        const V3 ground = v3(0.5f, 0.7f, 1.0f);
        const V3 sky = v3(1.0f, 1.0f, 1.0f);
        return vadd(vmul(sky, 1.0f - t), vmul(ground, t)); /* math.rs:1-7 lerp */
    }
    return vload(bg->color);
}

/* ------------------------------------------------------------------------------------------ */
/* rendering.rs:19-92 ray_color                                                                */
/* ------------------------------------------------------------------------------------------ */
static void count_hit(const Ctx* c, int leaf) {
    if (c->st) {
        c->st->hits[c->w->leaves[leaf].geom_kind]++;
        c->st->material_reads++;
    }
}

/* Like scene_hit but also reports which leaf produced the closest hit (stats only). */
static int bvh_closest_leaf_recursive(const Ctx* c, int32_t node, const Ray* r, float ts, float* te,
                                      Hit* h, int* leaf);
static int bvh_list_leaf(const Ctx* c, int32_t a, int32_t b, const Ray* r, float ts, float* te, Hit* h,
                         int* leaf) {
    int found = 0;
    Hit hi;
    int lf;
    if (bvh_closest_leaf_recursive(c, a, r, ts, te, &hi, &lf)) { *te = hi.t; *h = hi; *leaf = lf; found = 1; }
    if (bvh_closest_leaf_recursive(c, b, r, ts, te, &hi, &lf)) { *te = hi.t; *h = hi; *leaf = lf; found = 1; }
    return found;
}
static int bvh_closest_leaf_recursive(const Ctx* c, int32_t node, const Ray* r, float ts, float* te,
                                      Hit* h, int* leaf) {
    if (node < 0) {
        *leaf = -1 - node;
        return leaf_hit(c, -1 - node, r, ts, *te, h);
    }
    const rtw_bvh_node* nd = &c->w->nodes[node];
    if (c->st) c->st->node_visits++;
    if (!aabb_hit_cond(nd, r, ts, *te)) return 0;
    if (c->km && !cull_pass(c->km, node, nd, r, ts, *te)) return 0;
    if (r->dir.e[nd->axis] > 0.0f) return bvh_list_leaf(c, nd->left, nd->right, r, ts, te, h, leaf);
    return bvh_list_leaf(c, nd->right, nd->left, r, ts, te, h, leaf);
}
static int world_hit_leaf(const Ctx* c, const Ray* r, Hit* h, int* leaf) {
    if (c->st) c->st->rays++;
    float end = F32_INF;
    *leaf = -1;
    const int ok = bvh_closest_leaf_recursive(c, c->w->root, r, 0.001f, &end, h, leaf);
    if (ok) count_hit(c, *leaf);
    return ok;
}
static int world_hit(const Ctx* c, const Ray* r, Hit* h) {
    int leaf;
    return world_hit_leaf(c, r, h, &leaf);
}

/* One loop for ray_color and rtw_oracle_path: `rec` (NULL for the renderer) receives one record per segment,
 * at most `cap` of them; *count is the number of segments walked.  The arithmetic does not know about it. */
static void put3(float* o, V3 v) { o[0] = v.e[0]; o[1] = v.e[1]; o[2] = v.e[2]; }
static rtw_oracle_vertex* vertex_begin(rtw_oracle_vertex* rec, int cap, int* count, const Ctx* c, const Ray* cur) {
    if (!rec) return NULL;
    const int k = (*count)++;
    if (k >= cap) return NULL;
    rtw_oracle_vertex* v = &rec[k];
    memset(v, 0, sizeof(*v));
    v->leaf = -1;
    v->material = -1;
    v->state_before[0] = c->rng->s0;
    v->state_before[1] = c->rng->s1;
    put3(v->origin, cur->origin);
    put3(v->dir, cur->dir);
    v->time = cur->time;
    return v;
}
static void vertex_end(rtw_oracle_vertex* v, const Ctx* c, int end, V3 att, V3 acc) {
    if (!v) return;
    v->end = end;
    put3(v->att, att);
    put3(v->acc, acc);
    v->state_after[0] = c->rng->s0;
    v->state_after[1] = c->rng->s1;
}

static V3 ray_color_rec(const Ctx* c, const Ray* ray, int32_t max_depth, rtw_oracle_vertex* rec, int cap, int* count) {
    const rtw_world* w = c->w;
    int32_t depth = max_depth;
    V3 att = v3(1.0f, 1.0f, 1.0f);
    V3 emitted_acc = v3(0.0f, 0.0f, 0.0f);
    Ray cur = *ray;
    for (;;) {
        Hit h;
        int leaf = -1;
        rtw_oracle_vertex* v = vertex_begin(rec, cap, count, c, &cur);
        if (world_hit_leaf(c, &cur, &h, &leaf)) {
            if (v) {
                v->hit = 1;
                v->leaf = leaf;
                v->t = h.t;
                put3(v->position, h.position);
                put3(v->normal, h.normal);
                v->front_face = h.front_face;
                v->material = h.material;
            }
            if (depth <= 1) {
                vertex_end(v, c, RTW_PATH_END_DEPTH, att, emitted_acc);
                return v3(0.0f, 0.0f, 0.0f);
            }
            const rtw_material* M = &w->materials[h.material];
            V3 a;
            Dist d;
            if (material_scatter(c, M, &cur, &h, &a, &d)) {
                Ray scattered;
                float prob;
                if (d.kind == DIST_MIRROR) {
                    scattered.origin = h.position;
                    scattered.dir = dist_generate(&d, c->rng);
                    scattered.time = cur.time;
                    prob = 1.0f;
                } else {
                    /* sample_final_scattering_distribution (rendering.rs:73-92) */
                    V3 dir;
                    float p;
                    if (w->has_light) {
                        const float mix = 0.5f;
                        if (rtw_gen_bool_half(c->rng)) dir = light_generate(&w->light, h.position, c->rng);
                        else dir = dist_generate(&d, c->rng);
                        p = mix * light_value(&w->light, h.position, dir) + (1.0f - mix) * dist_value(&d, dir);
                    } else {
                        dir = dist_generate(&d, c->rng);
                        p = dist_value(&d, dir);
                    }
                    scattered.origin = h.position;
                    scattered.dir = dir;
                    scattered.time = cur.time;
                    const float spdf = material_scattering_pdf(M, &scattered, &h);
                    prob = spdf / p;
                }
                const V3 e = material_emit(c, M, &h);
                emitted_acc = vadd(emitted_acc, vconv(att, e));
                att = vmul(vconv(att, a), prob);
                if (v) {
                    v->scatters = 1;
                    put3(v->scattered, scattered.dir);
                    put3(v->a, a);
                    put3(v->e, e);
                    v->prob = prob;
                }
                vertex_end(v, c, RTW_PATH_CONTINUES, att, emitted_acc);
                cur = scattered;
                depth -= 1;
                continue;
            }
            const V3 e = material_emit(c, M, &h);
            if (v) put3(v->e, e);
            vertex_end(v, c, RTW_PATH_END_ABSORBED, att, emitted_acc);
            return vadd(emitted_acc, vconv(att, e));
        }
        /* rendering.rs:67: background of the PRIMARY ray */
        const V3 e = background_sample(&w->background, ray);
        if (v) put3(v->e, e);
        vertex_end(v, c, RTW_PATH_END_MISS, att, emitted_acc);
        return vadd(emitted_acc, vconv(att, e));
    }
}
static V3 ray_color(const Ctx* c, const Ray* ray, int32_t max_depth) {
    return ray_color_rec(c, ray, max_depth, NULL, 0, NULL);
}

/* RenderMode::ray_color (rendering.rs:100-119) */
static V3 mode_ray_color(const Ctx* c, const Ray* ray, int32_t max_depth, int32_t mode) {
    if (mode == RTW_MODE_NORMALS) {
        Hit h;
        if (world_hit(c, ray, &h)) return vmul(vadd(h.normal, v3(1.0f, 1.0f, 1.0f)), 0.5f);
        return background_sample(&c->w->background, ray);
    }
    return ray_color(c, ray, max_depth);
}

/* ------------------------------------------------------------------------------------------ */
/* camera.rs:175-200                                                                           */
/* ------------------------------------------------------------------------------------------ */
static Ray camera_ray(const rtw_camera* cam, rtw_xoro* rng, float px, float py) {
    V3 offset = v3(0.0f, 0.0f, 0.0f);
    if (cam->lens_radius > 0.0f) {
        float d[2];
        rtw_unit_disc(rng, d);
        offset = vmul(vadd(vmul(vload(cam->unit_right), d[0]), vmul(vload(cam->unit_up), d[1])), cam->lens_radius);
    }
    float start_time;
    if (cam->time0 == cam->time1) start_time = cam->time0;
    else start_time = rtw_gen_range_f32(cam->time0, cam->time1, rng);
    const float time = start_time + (cam->shutter_pace[0] * px + cam->shutter_pace[1] * py);
    Ray r;
    r.origin = vadd(vload(cam->position), offset);
    r.dir = vunit(vsub(vsub(vadd(vload(cam->upper_left_corner), vmul(vload(cam->scaled_right), px)),
                            vmul(vload(cam->scaled_up), py)),
                       offset));
    r.time = time;
    return r;
}

/* ------------------------------------------------------------------------------------------ */
/* render (rendering.rs:121-252)                                                               */
/* ------------------------------------------------------------------------------------------ */
typedef struct Job {
    const rtw_world* w;
    const rtw_render_params* p;
    int mode; /* rng mode */
    const float* km; /* proximity cull constants or NULL */
    float* out;
    /* ctr */
    int row_begin, row_step;
    /* ref */
    uint32_t thread_id, spp_t;
    Stats st;
    int want_stats;
} Job;

static int tile_owned(const rtw_render_params* p, int x, int y) {
    const int tw = p->tile_width > 0 ? p->tile_width : 8;
    const int th = p->tile_height > 0 ? p->tile_height : 8;
    const int pc = p->part_count > 0 ? p->part_count : 1;
    const int tiles_x = (p->width + tw - 1) / tw;
    const int t = (y / th) * tiles_x + (x / tw);
    return (t % pc) == p->part_index;
}

static void* ctr_worker(void* arg) {
    Job* j = (Job*)arg;
    const rtw_render_params* p = j->p;
    const int W = p->width, H = p->height;
    const float sx = 1.0f / (float)(W - 1); /* size2i.rs:21-22 */
    const float sy = 1.0f / (float)(H - 1);
    /* rendering.rs:132-138 -> vec2.rs:46-60 Uniform::new(min, max) per axis */
    const rtw_uniform ux = rtw_uniform_new(0.0f, 1.0f / (float)(W - 1));
    const rtw_uniform uy = rtw_uniform_new(0.0f, 1.0f / (float)(H - 1));
    const uint64_t key = rtw_seed_key(p->seed);
    rtw_xoro rng;
    Ctx c;
    c.w = j->w;
    c.rng = &rng;
    c.st = j->want_stats ? &j->st : NULL;
    c.km = j->km;
    const uint32_t T = p->thread_count > 1 ? (uint32_t)p->thread_count : 1u;
    const uint32_t whole = p->samples_per_pixel / T, rem = p->samples_per_pixel % T;
    const uint32_t n_planes = whole > 0 ? T : rem;
    V3* plane = (V3*)malloc(sizeof(V3) * n_planes);
    for (int y = j->row_begin; y < H; y += j->row_step) {
        for (int x = 0; x < W; ++x) {
            if (!tile_owned(p, x, y)) continue;
            const uint32_t pix = (uint32_t)(y * W + x);
            const float fx = (float)x * sx, fy = (float)y * sy;
            /* thread_count planes (split_work_tasks, rendering.rs:222-237), each the in-order sum
             * of its sample range / its count (rendering.rs:172-179); with ctr streams plane t
             * renders the global samples start_t .. start_t + n_t - 1 */
            uint32_t s = 0;
            for (uint32_t t = 0; t < n_planes; ++t) {
                const uint32_t n_t = whole + (t < rem ? 1u : 0u);
                V3 sum = v3(0.0f, 0.0f, 0.0f);
                for (uint32_t k = 0; k < n_t; ++k, ++s) {
                    rng = rtw_sample_stream(key, pix, s);
                    const float jx = rtw_uniform_sample(&ux, &rng);
                    const float jy = rtw_uniform_sample(&uy, &rng);
                    const Ray r = camera_ray(&j->w->camera, &rng, fx + jx, fy + jy);
                    sum = vadd(sum, mode_ray_color(&c, &r, p->max_depth, p->render_mode));
                    if (c.st) c.st->samples++;
                }
                plane[t] = vdiv(sum, (float)n_t);
            }
            /* merge_planes (rendering.rs:239-252): last plane, += planes 0..n-2, * (1/n) */
            V3 px = plane[n_planes - 1];
            for (uint32_t t = 0; t + 1 < n_planes; ++t) px = vadd(px, plane[t]);
            if (n_planes > 1) px = vmul(px, 1.0f / (float)n_planes);
            float* o = j->out + (size_t)pix * 3u;
            o[0] = px.e[0];
            o[1] = px.e[1];
            o[2] = px.e[2];
        }
    }
    free(plane);
    return NULL;
}

static void* ref_worker(void* arg) {
    Job* j = (Job*)arg;
    const rtw_render_params* p = j->p;
    const int W = p->width, H = p->height;
    const float sx = 1.0f / (float)(W - 1);
    const float sy = 1.0f / (float)(H - 1);
    const rtw_uniform ux = rtw_uniform_new(0.0f, 1.0f / (float)(W - 1));
    const rtw_uniform uy = rtw_uniform_new(0.0f, 1.0f / (float)(H - 1));
    rtw_xoro rng = rtw_thread_stream(p->seed, j->thread_id); /* rendering.rs:170 */
    Ctx c;
    c.w = j->w;
    c.rng = &rng;
    c.st = j->want_stats ? &j->st : NULL;
    c.km = j->km;
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
            const float fx = (float)x * sx, fy = (float)y * sy;
            V3 sum = v3(0.0f, 0.0f, 0.0f);
            for (uint32_t s = 0; s < j->spp_t; ++s) {
                const float jx = rtw_uniform_sample(&ux, &rng);
                const float jy = rtw_uniform_sample(&uy, &rng);
                const Ray r = camera_ray(&j->w->camera, &rng, fx + jx, fy + jy);
                sum = vadd(sum, mode_ray_color(&c, &r, p->max_depth, p->render_mode));
                if (c.st) c.st->samples++;
            }
            const V3 px = vdiv(sum, (float)j->spp_t);
            float* o = j->out + ((size_t)y * (size_t)W + (size_t)x) * 3u;
            o[0] = px.e[0];
            o[1] = px.e[1];
            o[2] = px.e[2];
        }
    }
    return NULL;
}

static int validate(const rtw_world* w, const rtw_render_params* p) {
    if (!w || !p) return RTW_ERR_INVALID_ARGUMENT;
    if (p->width < 2 || p->height < 2 || p->samples_per_pixel < 1) return RTW_ERR_INVALID_ARGUMENT;
    if (w->leaf_count < 1) return RTW_ERR_INVALID_ARGUMENT;
    const int pc = p->part_count > 0 ? p->part_count : 1;
    if (p->part_index < 0 || p->part_index >= pc) return RTW_ERR_INVALID_ARGUMENT;
    if (p->thread_count < 0 || p->reserved0 != 0) return RTW_ERR_INVALID_ARGUMENT; /* as the device */
    return RTW_OK;
}

static void add_stats(rtw_render_stats* o, const Stats* s) {
    o->samples += s->samples;
    o->rays += s->rays;
    o->node_visits += s->node_visits;
    o->sphere_tests += s->tests[RTW_GEOM_SPHERE];
    o->rect_tests += s->tests[RTW_GEOM_RECT];
    o->box_tests += s->tests[RTW_GEOM_BOX];
    o->triangle_tests += s->tests[RTW_GEOM_TRIANGLE];
    o->sphere_hits += s->hits[RTW_GEOM_SPHERE];
    o->rect_hits += s->hits[RTW_GEOM_RECT];
    o->box_hits += s->hits[RTW_GEOM_BOX];
    o->triangle_hits += s->hits[RTW_GEOM_TRIANGLE];
    o->material_reads += s->material_reads;
    o->texel_reads += s->texel_reads;
}

RTW_API int rtw_oracle_render(const rtw_world* w, const rtw_render_params* p, int rng_mode, int threads,
                              float* out_rgb, rtw_render_stats* stats) {
    const int v = validate(w, p);
    if (v != RTW_OK) return v;
    if (!out_rgb) return RTW_ERR_INVALID_ARGUMENT;
    if (threads < 1) threads = 1;
    if (stats) memset(stats, 0, sizeof(*stats));
    float* km = NULL;
    if (rng_mode & RTW_ORACLE_CULL) {
        km = (float*)malloc(sizeof(float) * 2u * (size_t)(w->node_count > 0 ? w->node_count : 1));
        rtw_cull_prepare(w, km, 0);
    }
    rng_mode &= ~RTW_ORACLE_CULL;
    const size_t n = (size_t)p->width * (size_t)p->height * 3u;
    if (rng_mode == RTW_ORACLE_RNG_CTR) {
        Job* jobs = (Job*)calloc((size_t)threads, sizeof(Job));
        pthread_t* th = (pthread_t*)calloc((size_t)threads, sizeof(pthread_t));
        for (int t = 0; t < threads; ++t) {
            jobs[t].w = w;
            jobs[t].p = p;
            jobs[t].out = out_rgb;
            jobs[t].row_begin = t;
            jobs[t].row_step = threads;
            jobs[t].want_stats = stats != NULL;
            jobs[t].km = km;
            pthread_create(&th[t], NULL, ctr_worker, &jobs[t]);
        }
        for (int t = 0; t < threads; ++t) pthread_join(th[t], NULL);
        if (stats)
            for (int t = 0; t < threads; ++t) add_stats(stats, &jobs[t].st);
        free(th);
        free(jobs);
        free(km);
        return RTW_OK;
    }
    /* ref mode: split_work_tasks (rendering.rs:222-237) */
    const uint32_t spp = p->samples_per_pixel;
    const uint32_t whole = spp / (uint32_t)threads, rem = spp % (uint32_t)threads;
    int nt = 0;
    while (nt < threads) {
        const uint32_t s = whole + ((uint32_t)nt < rem ? 1u : 0u);
        if (s == 0) break;
        ++nt;
    }
    Job* jobs = (Job*)calloc((size_t)nt, sizeof(Job));
    pthread_t* th = (pthread_t*)calloc((size_t)nt, sizeof(pthread_t));
    float** planes = (float**)calloc((size_t)nt, sizeof(float*));
    for (int t = 0; t < nt; ++t) {
        planes[t] = (float*)malloc(n * sizeof(float));
        jobs[t].w = w;
        jobs[t].p = p;
        jobs[t].out = planes[t];
        jobs[t].thread_id = (uint32_t)t;
        jobs[t].spp_t = whole + ((uint32_t)t < rem ? 1u : 0u);
        jobs[t].want_stats = stats != NULL;
        jobs[t].km = km;
        pthread_create(&th[t], NULL, ref_worker, &jobs[t]);
    }
    for (int t = 0; t < nt; ++t) pthread_join(th[t], NULL);
    /* merge_planes (rendering.rs:239-252): last plane += planes[0..n-1] in order, * 1/n */
    const float mult = 1.0f / (float)nt;
    float* px = planes[nt - 1];
    for (int t = 0; t < nt - 1; ++t)
        for (size_t i = 0; i < n; ++i) px[i] += planes[t][i];
    for (size_t i = 0; i < n; ++i) out_rgb[i] = px[i] * mult;
    if (stats)
        for (int t = 0; t < nt; ++t) add_stats(stats, &jobs[t].st);
    for (int t = 0; t < nt; ++t) free(planes[t]);
    free(planes);
    free(th);
    free(jobs);
    free(km);
    return RTW_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* single-ray entry points for known-answer tests                                              */
/* ------------------------------------------------------------------------------------------ */
RTW_API int rtw_oracle_scene_hit(const rtw_world* w, const float origin[3], const float dir[3], float time,
                                 float t_start, float t_end, uint64_t rng_state[2], rtw_oracle_hit* out) {
    if (!w || !out || w->leaf_count < 1) return RTW_ERR_INVALID_ARGUMENT;
    rtw_xoro rng = {rng_state[0], rng_state[1]};
    Ctx c = {w, &rng, NULL, NULL};
    Ray r;
    r.origin = vload(origin);
    r.dir = vload(dir);
    r.time = time;
    Hit h;
    float end = t_end;
    memset(out, 0, sizeof(*out));
    int leaf = -1;
    out->hit = bvh_closest_leaf_recursive(&c, w->root, &r, t_start, &end, &h, &leaf);
    if (out->hit) {
        out->t = h.t;
        for (int i = 0; i < 3; ++i) {
            out->position[i] = h.position.e[i];
            out->normal[i] = h.normal.e[i];
        }
        out->uv[0] = h.u;
        out->uv[1] = h.v;
        out->front_face = h.front_face;
        out->material = h.material;
    }
    rng_state[0] = rng.s0;
    rng_state[1] = rng.s1;
    return RTW_OK;
}

RTW_API int rtw_oracle_camera_ray(const rtw_camera* cam, float px, float py, uint64_t rng_state[2],
                                  float origin[3], float dir[3], float* time) {
    rtw_xoro rng = {rng_state[0], rng_state[1]};
    const Ray r = camera_ray(cam, &rng, px, py);
    for (int i = 0; i < 3; ++i) {
        origin[i] = r.origin.e[i];
        dir[i] = r.dir.e[i];
    }
    *time = r.time;
    rng_state[0] = rng.s0;
    rng_state[1] = rng.s1;
    return RTW_OK;
}

RTW_API int rtw_oracle_ray_color(const rtw_world* w, const float origin[3], const float dir[3], float time,
                                 int32_t max_depth, int32_t mode, uint64_t rng_state[2], float color[3]) {
    if (!w || w->leaf_count < 1) return RTW_ERR_INVALID_ARGUMENT;
    rtw_xoro rng = {rng_state[0], rng_state[1]};
    Ctx c = {w, &rng, NULL, NULL};
    Ray r;
    r.origin = vload(origin);
    r.dir = vload(dir);
    r.time = time;
    const V3 col = mode_ray_color(&c, &r, max_depth, mode);
    for (int i = 0; i < 3; ++i) color[i] = col.e[i];
    rng_state[0] = rng.s0;
    rng_state[1] = rng.s1;
    return RTW_OK;
}

RTW_API int rtw_oracle_path(const rtw_world* w, const float origin[3], const float dir[3], float time,
                            int32_t max_depth, uint64_t rng_state[2], rtw_oracle_vertex* vertices, int32_t capacity,
                            int32_t* count, float color[3]) {
    if (!w || w->leaf_count < 1 || !vertices || capacity < 0 || !count) return RTW_ERR_INVALID_ARGUMENT;
    rtw_xoro rng = {rng_state[0], rng_state[1]};
    Ctx c = {w, &rng, NULL, NULL};
    Ray r;
    r.origin = vload(origin);
    r.dir = vload(dir);
    r.time = time;
    int n = 0;
    const V3 col = ray_color_rec(&c, &r, max_depth, vertices, capacity, &n);
    *count = n;
    for (int i = 0; i < 3; ++i) color[i] = col.e[i];
    rng_state[0] = rng.s0;
    rng_state[1] = rng.s1;
    return RTW_OK;
}

/* rtw_oracle_path over n rays (packed origins, directions, times and states), `capacity` records a ray. */
RTW_API int rtw_oracle_paths(const rtw_world* w, const float* origins, const float* dirs, const float* times,
                             int64_t n, int32_t max_depth, uint64_t* rng_states, rtw_oracle_vertex* vertices,
                             int32_t capacity, int32_t* counts, float* colors) {
    for (int64_t i = 0; i < n; ++i) {
        const int rc = rtw_oracle_path(w, origins + 3 * i, dirs + 3 * i, times[i], max_depth, rng_states + 2 * i,
                                       vertices + (size_t)capacity * (size_t)i, capacity, counts + i, colors + 3 * i);
        if (rc != RTW_OK) return rc;
    }
    return RTW_OK;
}

RTW_API int rtw_oracle_ray_colors(const rtw_world* w, const float* origins, const float* dirs, const float* times,
                                  int64_t n, int32_t max_depth, uint64_t* rng_states, float* colors) {
    for (int64_t i = 0; i < n; ++i) {
        const int rc = rtw_oracle_ray_color(w, origins + 3 * i, dirs + 3 * i, times[i], max_depth, RTW_MODE_DEFAULT,
                                            rng_states + 2 * i, colors + 3 * i);
        if (rc != RTW_OK) return rc;
    }
    return RTW_OK;
}

/* One camera sample's radiance in ctr mode: pixel (x, y), global sample index s (the per-sample
 * term of rendering.rs:172-178 before any summation). */
RTW_API int rtw_oracle_sample_color(const rtw_world* w, const rtw_render_params* p, int32_t x, int32_t y, uint32_t s,
                                    float color[3]) {
    const int v = validate(w, p);
    if (v != RTW_OK) return v;
    const int W = p->width, H = p->height;
    if (x < 0 || y < 0 || x >= W || y >= H) return RTW_ERR_INVALID_ARGUMENT;
    const rtw_uniform ux = rtw_uniform_new(0.0f, 1.0f / (float)(W - 1));
    const rtw_uniform uy = rtw_uniform_new(0.0f, 1.0f / (float)(H - 1));
    rtw_xoro rng = rtw_sample_stream(rtw_seed_key(p->seed), (uint32_t)(y * W + x), s);
    Ctx c = {w, &rng, NULL, NULL};
    const float jx = rtw_uniform_sample(&ux, &rng);
    const float jy = rtw_uniform_sample(&uy, &rng);
    const Ray r = camera_ray(&w->camera, &rng, (float)x * (1.0f / (float)(W - 1)) + jx,
                             (float)y * (1.0f / (float)(H - 1)) + jy);
    const V3 col = mode_ray_color(&c, &r, p->max_depth, p->render_mode);
    for (int i = 0; i < 3; ++i) color[i] = col.e[i];
    return RTW_OK;
}

RTW_API int rtw_oracle_eval_scalar(int fn, const float* a, const float* b, int64_t n, float* out) {
    for (int64_t i = 0; i < n; ++i) {
        switch (fn) {
            case 0: out[i] = rtw_acosf(a[i]); break;
            case 1: out[i] = rtw_atan2f(a[i], b[i]); break;
            case 2: out[i] = rtw_logf(a[i]); break;
            case 3: out[i] = rtw_sinf(a[i]); break;
            case 4: out[i] = a[i] / b[i]; break;
            case 5: out[i] = sqrtf(a[i]); break;
            case 6: out[i] = a[i] / b[i]; break;
            default: return RTW_ERR_INVALID_ARGUMENT;
        }
    }
    return RTW_OK;
}

RTW_API int rtw_oracle_node_pass(const float* box, const float* ray, const float* range, const float* km, int64_t n,
                                 int32_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        rtw_bvh_node nd;
        memset(&nd, 0, sizeof(nd));
        for (int k = 0; k < 3; ++k) {
            nd.min[k] = box[6 * i + k];
            nd.max[k] = box[6 * i + 3 + k];
        }
        Ray r;
        memset(&r, 0, sizeof(r));
        for (int k = 0; k < 3; ++k) {
            r.origin.e[k] = ray[6 * i + k];
            r.dir.e[k] = ray[6 * i + 3 + k];
        }
        const float ts = range[2 * i], te = range[2 * i + 1];
        out[i] = aabb_hit_cond(&nd, &r, ts, te) && cull_pass(km + 2 * i, 0, &nd, &r, ts, te);
    }
    return RTW_OK;
}
