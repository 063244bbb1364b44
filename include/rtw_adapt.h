/*
 * rtw_adapt.h -- the per-tile convergence test of an adaptive accumulator (RTW_ACCUM_ADAPTIVE, rtw.h;
 * DESIGN.md 5.5d).  Plain C99 (gcc) and HIP C++ (hipcc) from one text, like rtw_beam.h: IEEE f32
 * add / sub / mul / div / sqrt only, no contraction, no fused steps, so the device kernel, the host
 * twin (rtw_adapt_tiles_host) and a numpy restatement take the same decisions bit for bit.
 *
 * Per channel, from the running sum and sum of squares of n samples (the order is the contract):
 *   nf = (float)n; mean = sum / nf; d = sq - sum * mean; var = (d < 0 ? 0 : d) / (float)(n - 1);
 *   se = sqrt(var / nf)
 * per pixel
 *   e = ((se_r + se_g) + se_b) / (((mean_r + mean_g) + mean_b) + 0.01f)
 * and per tile E = the maximum of e over the tile's owned pixels whose e is finite (0 when there is
 * none).  A maximum does not depend on the order it is taken in.  The tile stops at n samples when
 *   n >= min_samples  and  E <= target.
 */
#ifndef RTW_ADAPT_H
#define RTW_ADAPT_H

#include "rtw.h"
#include "rtw_scalar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one partition's tiles, as the render kernel lays them out (defaults resolved: tile 0 -> 8, part_count 0 -> 1) */
typedef struct rtw_adapt_geom {
    int32_t width, height, tile_w, tile_h, tiles_x, part_index, part_count;
    int32_t local_tiles; /* tiles t = part_index, part_index + part_count, ... of the frame */
} rtw_adapt_geom;

/* 0, or -1 for params no frame takes */
RTW_HD int rtw_adapt_geom_of(const rtw_render_params* p, rtw_adapt_geom* g) {
    if (p->width < 2 || p->height < 2) return -1;
    g->width = p->width;
    g->height = p->height;
    g->tile_w = p->tile_width > 0 ? p->tile_width : 8;
    g->tile_h = p->tile_height > 0 ? p->tile_height : 8;
    g->part_count = p->part_count > 0 ? p->part_count : 1;
    g->part_index = p->part_index;
    if (g->part_index < 0 || g->part_index >= g->part_count) return -1;
    g->tiles_x = (g->width + g->tile_w - 1) / g->tile_w;
    const int64_t n_tiles = (int64_t)g->tiles_x * ((g->height + g->tile_h - 1) / g->tile_h);
    const int64_t owned = n_tiles > g->part_index ? (n_tiles - g->part_index + g->part_count - 1) / g->part_count : 0;
    if (owned * g->tile_w * g->tile_h >= (int64_t)0xFFFFFFFF) return -1;
    g->local_tiles = (int32_t)owned;
    return 0;
}

/* the standard error of a channel's mean (rtw_accum_resolve_stderr); samples >= 2 */
RTW_HD float rtw_adapt_se(float sum, float sq, uint32_t samples, float* mean) {
    const float nf = (float)samples;
    *mean = sum / nf;
    const float d = sq - sum * *mean;
    const float var = (d < 0.0f ? 0.0f : d) / (float)(samples - 1); /* a NaN d stays NaN */
    return __builtin_sqrtf(var / nf);
}

/* a pixel's relative error (rtw_accum_noise) from its 3 sums and 3 squares */
RTW_HD float rtw_adapt_pixel(const float* S, const float* Q, uint32_t samples) {
    float mr, mg, mb;
    const float sr = rtw_adapt_se(S[0], Q[0], samples, &mr);
    const float sg = rtw_adapt_se(S[1], Q[1], samples, &mg);
    const float sb = rtw_adapt_se(S[2], Q[2], samples, &mb);
    return ((sr + sg) + sb) / (((mr + mg) + mb) + 0.01f);
}

RTW_HD int rtw_adapt_finite(float e) { return __builtin_fabsf(e) < rtw_u2f(0x7F800000u); } /* 0 for NaN */

/* The running maximum starts at -inf (no finite pixel yet); rtw_adapt_tile_e turns that into 0. */
RTW_HD float rtw_adapt_none(void) { return rtw_u2f(0xFF800000u); }
RTW_HD float rtw_adapt_max(float E, float e) { return rtw_adapt_finite(e) && e > E ? e : E; }
RTW_HD float rtw_adapt_tile_e(float E) { return E == rtw_adapt_none() ? 0.0f : E; }

/* the stop rule: the value tile_stop takes (0: the tile stays active) */
RTW_HD uint32_t rtw_adapt_stop(float E, uint32_t samples, float target, uint32_t min_samples) {
    return samples >= min_samples && E <= target ? samples : 0u;
}

/* slot `it` of local tile `lt`: 1 and its pixel when the partition owns one there, 0 for padding */
RTW_HD int rtw_adapt_slot_pixel(const rtw_adapt_geom* g, int32_t lt, int32_t it, int32_t* px, int32_t* py) {
    const int32_t tile = g->part_index + lt * g->part_count;
    *px = (tile % g->tiles_x) * g->tile_w + it % g->tile_w;
    *py = (tile / g->tiles_x) * g->tile_h + it / g->tile_w;
    return *px < g->width && *py < g->height;
}

/* One tile's E over its slots, one after the other: the host form of the device's wave (lanes stride
 * over the slots, then a 64-lane maximum). */
RTW_HD float rtw_adapt_tile(const float* sums, const float* squares, const rtw_adapt_geom* g, int32_t lt,
                            uint32_t samples) {
    const int32_t per_tile = g->tile_w * g->tile_h;
    float E = rtw_adapt_none();
    for (int32_t it = 0; it < per_tile; ++it) {
        int32_t px, py;
        if (!rtw_adapt_slot_pixel(g, lt, it, &px, &py)) continue;
        const size_t at = 3 * ((size_t)lt * (size_t)per_tile + (size_t)it);
        E = rtw_adapt_max(E, rtw_adapt_pixel(sums + at, squares + at, samples));
    }
    return rtw_adapt_tile_e(E);
}

/* rtw_accum_adapt on host arrays (sums, squares: 3 floats per slot, tile-major; tile_stop: one entry
 * per local tile, updated in place: a stopped tile stays as it is).  0, or -1 for arguments the device
 * call refuses too (samples < 2, min_samples < 2, bad geometry). */
RTW_HD int rtw_adapt_tiles(const float* sums, const float* squares, const rtw_render_params* params, uint32_t samples,
                           float target, uint32_t min_samples, uint32_t* tile_stop) {
    rtw_adapt_geom g;
    if (samples < 2 || min_samples < 2 || rtw_adapt_geom_of(params, &g) != 0) return -1;
    for (int32_t lt = 0; lt < g.local_tiles; ++lt) {
        if (tile_stop[lt] != 0) continue;
        tile_stop[lt] = rtw_adapt_stop(rtw_adapt_tile(sums, squares, &g, lt, samples), samples, target, min_samples);
    }
    return 0;
}

#ifdef __cplusplus
}
#endif

#endif /* RTW_ADAPT_H */
