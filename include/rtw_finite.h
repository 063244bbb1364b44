/*
 * rtw_finite.h -- finite-sample accumulation (RTW_ACCUM_FINITE, rtw.h).  Plain C99 (gcc) and
 * HIP C++ (hipcc) from one text, like rtw_adapt.h: IEEE f32 add / mul / div / sqrt only, no contraction, so the
 * device kernels, the host twins (rtw_finite_accumulate_host, rtw_adapt_tiles_finite_host) and a numpy
 * restatement hold the same bits.
 *
 * The definition (the order is the contract).  A sample's colour c is finite iff each of its three channels x
 * satisfies fabsf(x) < inf: NaN and +-inf fail, and one bad channel rejects the whole sample.  Per slot, in
 * sample order,
 *   a finite c:      sum = add(sum, c);  sq = add(sq, mul(c, c)) (accumulators with moments only);  kept += 1
 *   a non-finite c:  touches nothing.
 * kept is one uint32_t per slot, zero at create and in padding slots;
 *   rejected = (the slot's sample count, rtw_accum_resolve_samples) - kept.
 * Resolve: sum / (float)kept; kept == 0 gives +0.0 in each channel.  Standard error, noise and adapt:
 * rtw_adapt_se / rtw_adapt_pixel (rtw_adapt.h) with n = the pixel's kept in place of the tile's count.  For
 * kept < 2 that expression is not finite (kept 0: the mean is 0 / 0; kept 1: var is d / 0 with d >= 0 or NaN, so
 * se is +inf or NaN), and rtw_adapt_finite leaves such a pixel out of the noise mean and of a tile's E: nothing
 * new is defined for it.  A finite c whose square overflows is kept; its sq becomes +inf and the pixel drops out
 * of the noise estimate as it does without the flag.
 *
 * On a pixel with no rejected sample kept equals the sample count and every value is the plain accumulator's,
 * bit for bit.
 */
#ifndef RTW_FINITE_H
#define RTW_FINITE_H

#include "rtw_adapt.h"

#ifdef __cplusplus
extern "C" {
#endif

RTW_HD int rtw_finite_channel(float x) { return __builtin_fabsf(x) < rtw_u2f(0x7F800000u); } /* 0 for NaN */
RTW_HD int rtw_finite_sample(float r, float g, float b) {
    return rtw_finite_channel(r) & rtw_finite_channel(g) & rtw_finite_channel(b);
}

/* sum / (float)kept of one channel; +0.0 for kept == 0 */
RTW_HD float rtw_finite_mean(float sum, uint32_t kept) { return kept ? sum / (float)kept : 0.0f; }

/* One launch's samples onto host arrays: colors[(s * total + slot) * 3 + ch] for s < n_samples (the render
 * kernel's colour buffer), sums / squares (may be null: no moments) 3 floats per slot, kept one entry per slot.
 * Every slot is taken as it comes (no geometry here): a padding slot whose colours are NaN stays zero, as the
 * device leaves it. */
RTW_HD void rtw_finite_accumulate(const float* colors, uint32_t n_samples, uint32_t total, float* sums, float* squares,
                                  uint32_t* kept) {
    for (uint32_t slot = 0; slot < total; ++slot) {
        float* S = sums + 3 * (size_t)slot;
        float* Q = squares ? squares + 3 * (size_t)slot : (float*)0;
        uint32_t k = kept[slot];
        for (uint32_t s = 0; s < n_samples; ++s) {
            const float* c = colors + 3 * ((size_t)s * (size_t)total + (size_t)slot);
            if (!rtw_finite_sample(c[0], c[1], c[2])) continue;
            for (int ch = 0; ch < 3; ++ch) {
                S[ch] = S[ch] + c[ch];
                if (Q) {
                    const float cc = c[ch] * c[ch];
                    Q[ch] = Q[ch] + cc;
                }
            }
            ++k;
        }
        kept[slot] = k;
    }
}

/* rtw_adapt_tile with each pixel's own kept as its n */
RTW_HD float rtw_adapt_tile_finite(const float* sums, const float* squares, const uint32_t* kept, const rtw_adapt_geom* g,
                                   int32_t lt) {
    const int32_t per_tile = g->tile_w * g->tile_h;
    float E = rtw_adapt_none();
    for (int32_t it = 0; it < per_tile; ++it) {
        int32_t px, py;
        if (!rtw_adapt_slot_pixel(g, lt, it, &px, &py)) continue;
        const size_t slot = (size_t)lt * (size_t)per_tile + (size_t)it;
        E = rtw_adapt_max(E, rtw_adapt_pixel(sums + 3 * slot, squares + 3 * slot, kept[slot]));
    }
    return rtw_adapt_tile_e(E);
}

/* rtw_adapt_tiles of a finite accumulator: the same call-level preconditions (samples, the frontier, >= 2) and
 * the same stop rule on `samples`; only the per-pixel n is kept[slot]. */
RTW_HD int rtw_adapt_tiles_finite(const float* sums, const float* squares, const uint32_t* kept,
                                  const rtw_render_params* params, uint32_t samples, float target, uint32_t min_samples,
                                  uint32_t* tile_stop) {
    rtw_adapt_geom g;
    if (samples < 2 || min_samples < 2 || rtw_adapt_geom_of(params, &g) != 0) return -1;
    for (int32_t lt = 0; lt < g.local_tiles; ++lt) {
        if (tile_stop[lt] != 0) continue;
        tile_stop[lt] = rtw_adapt_stop(rtw_adapt_tile_finite(sums, squares, kept, &g, lt), samples, target, min_samples);
    }
    return 0;
}

/* The two host twins librtw.so exports (no GPU needed).  rtw_finite_accumulate_host: rtw_finite_accumulate;
 * squares may be NULL.  rtw_adapt_tiles_finite_host: rtw_adapt_tiles_host plus kept. */
RTW_API int rtw_finite_accumulate_host(const float* colors, uint32_t n_samples, uint32_t total, float* sums, float* squares,
                                       uint32_t* kept);
RTW_API int rtw_adapt_tiles_finite_host(const float* sums, const float* squares, const uint32_t* kept,
                                        const rtw_render_params* params, uint32_t samples, float target,
                                        uint32_t min_samples, uint32_t* tile_stop);

#ifdef __cplusplus
}
#endif

#endif /* RTW_FINITE_H */
