/*
 * rtw_clamp.h -- sample clamping at the accumulate step (RTW_ACCUM_CLAMP, rtw.h).  Plain C99 (gcc)
 * and HIP C++ (hipcc) from one text, like rtw_finite.h: IEEE f32 add / sub / mul / div / max / min only, no
 * contraction, so the device kernel, the host twin (rtw_clamp_accumulate_host) and a numpy restatement hold the
 * same bits.
 *
 * The definition (the order is the contract).  A clamp accumulator has a level L, an f32 with 0 < L < inf.  Per
 * slot, in sample order,
 *   a non-finite c (rtw_finite_sample, rtw_finite.h):  touches nothing.
 *   a finite c = (r, g, b):  m = max(max(r, g), b).
 *     m > L:   s = div(L, m);  c' = (min(mul(r, s), L), min(mul(g, s), L), min(mul(b, s), L));
 *              lost = add(lost, sub(c, c')) per channel;  clamped += 1
 *     else:    c' = c;  lost and clamped are untouched
 *     then     sum = add(sum, c');  sq = add(sq, mul(c', c')) (accumulators with moments only);  kept += 1
 * Scaling by the largest channel keeps the hue; the final min makes "no channel of an accumulated sample exceeds
 * L" hold exactly where mul(x, s) rounds above L.  A negative channel beside a large one is scaled with the rest.
 * clamped is one uint32_t per slot and lost three f32, zero at create and in padding slots; clamped <= kept.
 *
 * The resolves, standard error, noise and adapt are the finite accumulator's expressions (rtw_finite.h) on these
 * sums, squares and kept.  rtw_clamp_loss_mean: lost / (float)kept per channel, the mean radiance the clamp took
 * out of the pixel (mean + loss is the mean of the pixel's finite samples, up to rounding).
 *
 * On a pixel with no clamped sample every value is the finite accumulator's, bit for bit.
 */
#ifndef RTW_CLAMP_H
#define RTW_CLAMP_H

#include "rtw_finite.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a level an accumulator takes: 0 < L < inf (false for NaN) */
RTW_HD int rtw_clamp_level_ok(float level) { return level > 0.0f && level < rtw_u2f(0x7F800000u); }

/* max / min of finite operands (no NaN reaches them: the sample passed rtw_finite_sample) */
RTW_HD float rtw_clamp_max(float a, float b) { return a > b ? a : b; }
RTW_HD float rtw_clamp_min(float a, float b) { return a < b ? a : b; }

/* One finite sample c against the level: c' into out[3].  Returns 1 when the sample was clamped (then c - c' is
 * what the caller adds to lost), else 0 with out = c. */
RTW_HD int rtw_clamp_sample(float r, float g, float b, float level, float* out) {
    const float m = rtw_clamp_max(rtw_clamp_max(r, g), b);
    if (m > level) {
        const float s = level / m;
        const float rs = r * s, gs = g * s, bs = b * s;
        out[0] = rtw_clamp_min(rs, level);
        out[1] = rtw_clamp_min(gs, level);
        out[2] = rtw_clamp_min(bs, level);
        return 1;
    }
    out[0] = r;
    out[1] = g;
    out[2] = b;
    return 0;
}

/* lost / (float)kept of one channel; +0.0 for kept == 0 */
RTW_HD float rtw_clamp_loss_mean(float lost, uint32_t kept) { return kept ? lost / (float)kept : 0.0f; }

/* One launch's samples onto host arrays, the twin of rtw_finite_accumulate: colors[(s * total + slot) * 3 + ch] for
 * s < n_samples, sums / squares (may be null: no moments) / lost 3 floats per slot, kept / clamped one entry per
 * slot.  Every slot is taken as it comes: a padding slot whose colours are NaN stays zero. */
RTW_HD void rtw_clamp_accumulate(const float* colors, uint32_t n_samples, uint32_t total, float level, float* sums,
                                 float* squares, uint32_t* kept, uint32_t* clamped, float* lost) {
    for (uint32_t slot = 0; slot < total; ++slot) {
        float* S = sums + 3 * (size_t)slot;
        float* Q = squares ? squares + 3 * (size_t)slot : (float*)0;
        float* D = lost + 3 * (size_t)slot;
        uint32_t k = kept[slot], n = clamped[slot];
        for (uint32_t s = 0; s < n_samples; ++s) {
            const float* c = colors + 3 * ((size_t)s * (size_t)total + (size_t)slot);
            float v[3];
            if (!rtw_finite_sample(c[0], c[1], c[2])) continue;
            if (rtw_clamp_sample(c[0], c[1], c[2], level, v)) {
                for (int ch = 0; ch < 3; ++ch) {
                    const float d = c[ch] - v[ch];
                    D[ch] = D[ch] + d;
                }
                ++n;
            }
            for (int ch = 0; ch < 3; ++ch) {
                S[ch] = S[ch] + v[ch];
                if (Q) {
                    const float vv = v[ch] * v[ch];
                    Q[ch] = Q[ch] + vv;
                }
            }
            ++k;
        }
        kept[slot] = k;
        clamped[slot] = n;
    }
}

/* The host twin librtw.so exports (no GPU needed): rtw_clamp_accumulate; squares may be NULL; a level that is
 * NaN, <= 0 or infinite is refused (RTW_ERR_INVALID_ARGUMENT). */
RTW_API int rtw_clamp_accumulate_host(const float* colors, uint32_t n_samples, uint32_t total, float level, float* sums,
                                      float* squares, uint32_t* kept, uint32_t* clamped, float* lost);

#ifdef __cplusplus
}
#endif

#endif /* RTW_CLAMP_H */
