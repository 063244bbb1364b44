/*
 * rtw_beam.h -- which leaves a tile's camera rays can reach (the per-tile
 * leaf lists that replace the SAH walk for primary rays).  Plain C99 (gcc) and HIP C++ (hipcc) from
 * one text, like rtw_scalar.h: IEEE f32 add / sub / mul / div / sqrt only, no contraction, no fused
 * steps, no fast intrinsics, so the host builder and the device builder produce the same lists bit
 * for bit.
 *
 * The beam of a tile.  camera_ray (camera.rs:175-200) gives pixel coordinates (px, py) the ray from
 *   O' = position + e,   e = (unit_right d0 + unit_up d1) lens_radius, d0^2 + d1^2 <= 1
 * through
 *   F' = position + upper_left_corner + scaled_right px - scaled_up py.
 * For a tile, (px, py) lies in the closed rectangle [x0 sx, x1 sx + sx] x [y0 sy, y1 sy + sy]
 * (sx = 1 / (W - 1): pixel x0..x1, plus the jitter range [0, sx)).  With (pxc, pyc) its centre and
 * (hx, hy) its half sides,
 *   F' = F + f,  F = position + A,  A = ulc + sr pxc - su pyc,  |f| <= h = |sr| hx + |su| hy
 *   |e| <= l = lens_radius sqrt(|unit_right|^2 + |unit_up|^2)       (Cauchy-Schwarz; no orthogonality assumed)
 * and a point of a beam ray at parameter lambda >= 0 (1 at the focus plane) is
 *   O' + lambda (F' - O') = [position + lambda A] + (1 - lambda) e + lambda f,
 * i.e. within R(lambda) = l |1 - lambda| + h lambda of the axis point at the same lambda.
 *
 * The rule for a plain sphere leaf (centre c, radius r).  rtw_cull.h proves that the leaf's test
 * accepts a root only at a point within delta = k Dq + 64u D + m of its box [c - r, c + r], where Dq
 * and D bound the squared and the L1 distance from the ray origin to the box's far corner.  Here
 * they are taken over every lens point: M_i = |c_i - position_i| + r + l per axis.  The box grown by
 * delta lies in the ball B(c, rho), rho = sqrt(3) (r + delta).  If a beam ray meets that ball at a
 * point p with parameter lambda:
 *   |p - O'| = lambda |F' - O'|,  |F' - O'| in [L - l - h, L + l + h]  (L = |A|),
 *   |p - O'| in [dc - l - rho, dc + l + rho]                         (dc = |c - position|),
 * so lambda lies in [lmin, lmax] = [max(0, (dc - l - rho) / (L + l + h)), (dc + l + rho) / (L - l - h)];
 * R is convex, so R(lambda) <= Rmax = max(R(lmin), R(lmax)); and the distance from c to the axis LINE,
 * dperp = |(c - position) x A| / L, is at most |c - p| + |p - axis point| <= rho + Rmax.
 * The leaf may be left out only if  dperp > rho + Rmax + margin.
 *
 * The margin covers the f32 rounding of camera_ray and of this file's own arithmetic, generously (a
 * longer list costs a few sphere tests, a missing leaf an image): delta is doubled, Rmax grows by
 * 2^-10 of itself, and `margin` adds 2^-14 of every length involved -- the coordinates' magnitudes
 * (the rounding of position + e and of the direction's sums is a few u of them, u = 2^-24), the
 * distance to the far side of the ball times the direction's relative error, and dc, L for the
 * cross product and the norms here.  Any NaN keeps the leaf.  A camera whose tile has
 * L - l - h <= L / 2 (a lens or a tile as large as the focus distance), a non-finite value, or
 * L = 0 is degenerate: the tile takes the walk.
 */
#ifndef RTW_BEAM_H
#define RTW_BEAM_H

#include "rtw.h"
#include "rtw_scalar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a tile's result when it has no list: its camera rays take the SAH walk */
#define RTW_BEAM_WALK (-1)
#define RTW_BEAM_CAP_DEFAULT 16

typedef struct rtw_beam_tile {
    float pos[3];  /* camera position */
    float a[3];    /* the axis: position -> the focus point of the tile's centre */
    float L;       /* |a| */
    float l;       /* bound on a lens offset's length */
    float h;       /* bound on the focus point's offset from the axis end */
    float mag;     /* sum of the coordinate magnitudes camera_ray adds up */
    int32_t ok;    /* 0: degenerate, the tile takes the walk */
} rtw_beam_tile;

/* correctly rounded on both sides (the device build's -fhip-fp32-correctly-rounded-divide-sqrt) */
RTW_HD float rtw_beam_sqrt(float x) { return __builtin_sqrtf(x); }
RTW_HD float rtw_beam_len(const float v[3]) { return rtw_beam_sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
RTW_HD float rtw_beam_abs3(const float v[3]) {
    return (__builtin_fabsf(v[0]) + __builtin_fabsf(v[1])) + __builtin_fabsf(v[2]);
}

/* The beam of tile (tile_x, tile_y) of a W x H frame with tiles of tw x th pixels. */
RTW_HD void rtw_beam_tile_setup(const rtw_camera* c, int32_t W, int32_t H, int32_t tw, int32_t th, int32_t tile_x,
                                int32_t tile_y, rtw_beam_tile* t) {
    const float inf = rtw_u2f(0x7F800000u);
    const float sx = 1.0f / (float)(W - 1), sy = 1.0f / (float)(H - 1); /* size2i.rs:52-55, as the kernel */
    const int32_t x0 = tile_x * tw, y0 = tile_y * th;
    int32_t x1 = x0 + tw - 1, y1 = y0 + th - 1;
    if (x1 > W - 1) x1 = W - 1;
    if (y1 > H - 1) y1 = H - 1;
    const float pxa = (float)x0 * sx, pxb = (float)x1 * sx + sx;
    const float pya = (float)y0 * sy, pyb = (float)y1 * sy + sy;
    const float pxc = (pxa + pxb) * 0.5f, pyc = (pya + pyb) * 0.5f;
    /* half sides, measured from the rounded centre to both ends */
    const float hx = rtw_maxr(pxc - pxa, pxb - pxc), hy = rtw_maxr(pyc - pya, pyb - pyc);
    for (int i = 0; i < 3; ++i) {
        t->pos[i] = c->position[i];
        t->a[i] = (c->upper_left_corner[i] + c->scaled_right[i] * pxc) - c->scaled_up[i] * pyc;
    }
    t->L = rtw_beam_len(t->a);
    const float ur = rtw_beam_len(c->unit_right), uu = rtw_beam_len(c->unit_up);
    t->l = c->lens_radius > 0.0f ? c->lens_radius * rtw_beam_sqrt(ur * ur + uu * uu) : 0.0f;
    t->h = rtw_beam_len(c->scaled_right) * hx + rtw_beam_len(c->scaled_up) * hy;
    t->mag = (rtw_beam_abs3(c->position) + rtw_beam_abs3(c->upper_left_corner)) +
             ((rtw_beam_abs3(c->scaled_right) * pxb + rtw_beam_abs3(c->scaled_up) * pyb) + t->l);
    const float lmin = (t->L - t->l) - t->h;
    t->ok = (t->L > 0.0f && t->L < inf && t->l < inf && t->h < inf && t->mag < inf && lmin > t->L * 0.5f) ? 1 : 0;
}

/* 1: the sphere leaf {c, r} stays in the tile's list; 0: no beam ray can make its test accept.
 * Only for t->ok tiles and cullable spheres (rtw_cull_sphere: finite, r > 0). */
RTW_HD int rtw_beam_sphere_in(const rtw_beam_tile* t, float cx, float cy, float cz, float r) {
    const float v[3] = {cx - t->pos[0], cy - t->pos[1], cz - t->pos[2]};
    const float dc = rtw_beam_len(v);
    /* delta over every lens point (rtw_cull_delta's terms without its fused steps), doubled */
    const float m0 = (__builtin_fabsf(v[0]) + r) + t->l, m1 = (__builtin_fabsf(v[1]) + r) + t->l,
                m2 = (__builtin_fabsf(v[2]) + r) + t->l;
    const float cm = rtw_maxr(rtw_maxr(__builtin_fabsf(cx), __builtin_fabsf(cy)), __builtin_fabsf(cz));
    const float k = (64.0f * RTW_CULL_U) / r, m = (8.0f * RTW_CULL_U) * (cm + r); /* rtw_cull_sphere */
    const float delta = 2.0f * ((k * ((m0 * m0 + m1 * m1) + m2 * m2) + (64.0f * RTW_CULL_U) * ((m0 + m1) + m2)) + m);
    const float rho = 1.7320509f * (r + delta); /* RN(sqrt 3) rounded up */
    const float lmax = ((dc + t->l) + rho) / ((t->L - t->l) - t->h);
    float lmin = ((dc - t->l) - rho) / ((t->L + t->l) + t->h);
    if (!(lmin > 0.0f)) lmin = 0.0f;
    const float ra = t->l * __builtin_fabsf(1.0f - lmin) + t->h * lmin;
    const float rb = t->l * __builtin_fabsf(1.0f - lmax) + t->h * lmax;
    const float rmax = rtw_maxr(ra, rb);
    const float x[3] = {v[1] * t->a[2] - v[2] * t->a[1], v[2] * t->a[0] - v[0] * t->a[2], v[0] * t->a[1] - v[1] * t->a[0]};
    const float dperp = rtw_beam_len(x) / t->L;
    const float far_ = (dc + rho) + t->l;
    const float margin = 0x1p-14f * (((t->mag + cm) + (dc + t->L)) + far_ * (t->mag / t->L));
    const float bound = (rho + (rmax + rmax * 0x1p-10f)) + margin;
    if (dperp > bound) return 0;
    /* the slabs of the grown box (a sphere far larger than its distance, the ground under a sky tile, passes
     * the ball test from every tile): with R(lambda) <= l + g lambda, g = l + h, a beam point's coordinate i
     * lies within l + g lambda of pos_i + lambda a_i, so it reaches [lo_i - delta, hi_i + delta] only if
     *   lambda (a_i - g) <= (hi_i - pos_i) + e   and   lambda (a_i + g) >= (lo_i - pos_i) - e,
     * e = delta + l + margin.  The six half-lines must share a lambda in [0, lmax]; each quotient is widened
     * by 2^-12 of itself (the divisions and a_i -+ g round by a few u, and lambda <= lmax keeps the product's
     * error far inside the margin). */
    const float g = t->l + t->h;
    const float e = (delta + t->l) + margin;
    const float cc[3] = {cx, cy, cz};
    float lb = 0.0f, ub = lmax + lmax * 0x1p-10f;
    for (int i = 0; i < 3; ++i) {
        const float au = t->a[i] - g, bu = ((cc[i] + r) - t->pos[i]) + e;
        if (au != 0.0f) {
            const float q = bu / au;
            if (au > 0.0f) ub = rtw_minr(ub, q + __builtin_fabsf(q) * 0x1p-12f);
            else lb = rtw_maxr(lb, q - __builtin_fabsf(q) * 0x1p-12f);
        } else if (bu < 0.0f) {
            return 0;
        }
        const float al = t->a[i] + g, bl = ((cc[i] - r) - t->pos[i]) - e;
        if (al != 0.0f) {
            const float q = bl / al;
            if (al > 0.0f) lb = rtw_maxr(lb, q - __builtin_fabsf(q) * 0x1p-12f);
            else ub = rtw_minr(ub, q + __builtin_fabsf(q) * 0x1p-12f);
        } else if (bl > 0.0f) {
            return 0;
        }
    }
    return !(lb > ub);
}

/* One tile's list over the world's leaf records (`fast`: 4 floats per leaf, a plain sphere's
 * {c, r}; leaf_count of them), in leaf order.  Returns the number of entries written to list[0 ..
 * cap), or RTW_BEAM_WALK when the tile is degenerate or more than cap leaves stay.  The host form of
 * the device builder (one leaf per lane there, the same tests, the same order). */
RTW_HD int32_t rtw_beam_tile_list(const rtw_camera* c, int32_t W, int32_t H, int32_t tw, int32_t th, int32_t tile_x,
                                  int32_t tile_y, const float* fast, int32_t leaf_count, int32_t cap, int32_t* list) {
    rtw_beam_tile t;
    rtw_beam_tile_setup(c, W, H, tw, th, tile_x, tile_y, &t);
    if (!t.ok) return RTW_BEAM_WALK;
    int32_t n = 0;
    for (int32_t i = 0; i < leaf_count; ++i) {
        if (!rtw_beam_sphere_in(&t, fast[4 * i], fast[4 * i + 1], fast[4 * i + 2], fast[4 * i + 3])) continue;
        if (n >= cap) return RTW_BEAM_WALK;
        list[n++] = i;
    }
    return n;
}

#ifdef __cplusplus
}
#endif

#endif /* RTW_BEAM_H */
