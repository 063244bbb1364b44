/*
 * rtw_denoise.h -- the variance-guided a-trous preview filter of rtw_denoiser_run / rtw_denoise_host
 * (rtw.h).  Plain C99 (gcc) and HIP C++ (hipcc) from one text, like rtw_adapt.h: IEEE f32
 * add / sub / mul / div / sqrt only, no contraction, no transcendental function, so the device kernels, the
 * host twin and a numpy restatement give the same bits.  The order below is the contract.
 *
 * Inputs (RTW_LAYOUT_IMAGE, row-major from the top-left pixel): colour C (W*H*3), standard error E (W*H*3,
 * what rtw_accum_resolve_stderr writes), optional guide G (W*H*gc, gc in 0..4).
 * Constants: h = {1/16, 1/4, 3/8, 1/4, 1/16}, k = {1/4, 1/2, 1/4} (all products exact),
 * inv_sg2 = 1.0f / (sigma_g * sigma_g), finite(a) = fabsf(a) < inf.
 *
 * Prep, per pixel p:
 *   l = (C.r + C.g) + C.b;  v_c = E_c * E_c;  vl = (v_r + v_g) + v_b
 *   ok_p = finite(l) && finite(vl) && every guide channel of p is finite;  m_p = ok_p ? vl : NaN
 *   sk = 0; sv = 0; for dy = -1..1 (outer), dx = -1..1 (inner), q inside the image with ok_q:
 *       sk = sk + k[dy]k[dx];  sv = sv + (k[dy]k[dx]) * m_q
 *   g_p = ok_p ? sv / sk : NaN
 *   R0_p = {C.r, C.g, C.b, g_p}   (w: the variance of the luminance estimate); the guide is padded to 4 floats
 *   with zeros.
 * Level i = 0 .. iterations-1, step s = 1 << i, centre p: a record whose w is not finite passes through bit
 * for bit; otherwise
 *   lp = (r + g) + b; sw = 0; sc_c = 0; s2 = 0
 *   for dy = -2..2 (outer), dx = -2..2 (inner), q = (x + s dx, y + s dy); q outside the image or R_q.w not
 *   finite: skipped (never clamped); else
 *       lq = (r_q + g_q) + b_q
 *       x  = fabsf(lq - lp) / (sigma_l * sqrtf(R_p.w + R_q.w) + 1e-6f);  wl = 1.0f / (1.0f + x * x)
 *       d2 = 0; for c < gc: d = G_q[c] - G_p[c]; d2 = d2 + d * d
 *       t  = 1.0f - d2 * inv_sg2; if (t < 0) t = 0;  wg = t * t   (gc == 0: wg = 1)
 *       w  = (h[dy] * h[dx]) * (wl * wg)
 *       sw = sw + w;  sc_c = sc_c + w * q_c;  s2 = s2 + (w * w) * R_q.w
 *   R'_p = {sc_r / sw, sc_g / sw, sc_b / sw, s2 / (sw * sw)}     (the centre tap weighs 9/64: sw > 0)
 * Output: the last records' rgb, and optionally their w (NaN for pixels that were left out).
 *
 * The padded guide channels are zeros, so their d is +0 and d2 + d * d == d2 whatever d2 holds: summing 4
 * channels (the kernel) and gc channels give the same bits.
 *
 * Albedo demodulation (rtw_denoiser_run_albedo / rtw_denoise_host_albedo): with an albedo image
 * A (W*H*3) the filter above runs unchanged between a pre-step and a post-step.  Per pixel p and channel c:
 *   D_c = A_c >= 1/64 ? A_c : 1/64;  C'_c = C_c / D_c;  E'_c = E_c / D_c      (IEEE divisions)
 *   Prep reads (C', E', G) for (C, E, G) -- its 3 x 3 window included -- and ok_p also needs every albedo
 *   channel of p to be finite.
 * Output: F_c * D_c for a pixel with ok_p (F the last records' rgb), else the input C_c bit for bit.  The
 * variance output is the last records' w as before: the variance of the demodulated luminance estimate
 * (C'_r + C'_g) + C'_b, NaN for pixels that were left out.  Without A nothing changes, bit for bit.
 */
#ifndef RTW_DENOISE_H
#define RTW_DENOISE_H

#include "rtw.h"
#include "rtw_scalar.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__clang__)
#define RTW_DENOISE_UNROLL _Pragma("unroll") /* the 25 taps' loads issue together on the device */
#else
#define RTW_DENOISE_UNROLL
#endif

/* one pixel's record, and one pixel's padded guide: 16 bytes, read and written as one */
typedef struct __attribute__((aligned(16))) rtw_denoise_rec {
    float r, g, b, w;
} rtw_denoise_rec;

/* records of scratch rtw_denoise_image needs (two record buffers and the guide buffer) */
#define RTW_DENOISE_SCRATCH_RECS 3

RTW_HD int rtw_denoise_finite(float a) { return __builtin_fabsf(a) < rtw_u2f(0x7F800000u); } /* 0 for NaN */
RTW_HD float rtw_denoise_nan(void) { return rtw_u2f(0x7FC00000u); }
RTW_HD float rtw_denoise_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }
RTW_HD float rtw_denoise_k(int d) { return d == 0 ? 0.5f : 0.25f; }
RTW_HD float rtw_denoise_inv_sg2(float sigma_g) { return 1.0f / (sigma_g * sigma_g); }

/* 0, or the name of the first field no run takes */
RTW_HD const char* rtw_denoise_check(const rtw_denoise_params* p) {
    if (p->width < 2) return "width";
    if (p->height < 2) return "height";
    if (p->iterations < 1 || p->iterations > 6) return "iterations";
    if (p->guide_channels < 0 || p->guide_channels > 4) return "guide_channels";
    if (!(p->sigma_l > 0.0f) || !rtw_denoise_finite(p->sigma_l)) return "sigma_l";
    if (!(p->sigma_g > 0.0f) || !rtw_denoise_finite(p->sigma_g)) return "sigma_g";
    if (p->reserved0 != 0) return "reserved0";
    if (p->reserved1 != 0) return "reserved1";
    return 0;
}

/* m_p of pixel `at`: the luminance variance, NaN when the pixel is left out (ok_p == finite(m_p)) */
RTW_HD float rtw_denoise_m(const float* C, const float* E, const float* G, int32_t gc, size_t at) {
    const float* c = C + 3 * at;
    const float* e = E + 3 * at;
    const float l = (c[0] + c[1]) + c[2];
    const float vr = e[0] * e[0], vg = e[1] * e[1], vb = e[2] * e[2];
    const float vl = (vr + vg) + vb;
    int ok = rtw_denoise_finite(l) && rtw_denoise_finite(vl);
    for (int32_t ch = 0; ch < gc; ++ch) ok = ok && rtw_denoise_finite(G[(size_t)gc * at + (size_t)ch]);
    return ok ? vl : rtw_denoise_nan();
}

/* the prep record of pixel (x, y) */
RTW_HD rtw_denoise_rec rtw_denoise_prep_pixel(const float* C, const float* E, const float* G, int32_t gc, int32_t W,
                                              int32_t H, int32_t x, int32_t y) {
    const size_t at = (size_t)y * (size_t)W + (size_t)x;
    const int ok = rtw_denoise_finite(rtw_denoise_m(C, E, G, gc, at));
    float sk = 0.0f, sv = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        for (int dx = -1; dx <= 1; ++dx) {
            const int32_t qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float m = rtw_denoise_m(C, E, G, gc, (size_t)qy * (size_t)W + (size_t)qx);
            if (!rtw_denoise_finite(m)) continue;
            const float kk = rtw_denoise_k(dy) * rtw_denoise_k(dx);
            sk = sk + kk;
            sv = sv + kk * m;
        }
    }
    rtw_denoise_rec r;
    r.r = C[3 * at];
    r.g = C[3 * at + 1];
    r.b = C[3 * at + 2];
    r.w = ok ? sv / sk : rtw_denoise_nan();
    return r;
}

/* D of one albedo channel (a NaN gives 1/64; such a pixel is left out anyway) */
RTW_HD float rtw_denoise_d(float a) { return a >= 0.015625f ? a : 0.015625f; }

/* m_p with an albedo image: the demodulated colour of pixel `at` into c[3], and the luminance variance of the
 * demodulated pixel, NaN when the pixel is left out */
RTW_HD float rtw_denoise_m_albedo(const float* C, const float* E, const float* G, const float* A, int32_t gc, size_t at,
                                  float c[3]) {
    const float* a = A + 3 * at;
    const float d0 = rtw_denoise_d(a[0]), d1 = rtw_denoise_d(a[1]), d2 = rtw_denoise_d(a[2]);
    c[0] = C[3 * at] / d0;
    c[1] = C[3 * at + 1] / d1;
    c[2] = C[3 * at + 2] / d2;
    const float e0 = E[3 * at] / d0, e1 = E[3 * at + 1] / d1, e2 = E[3 * at + 2] / d2;
    const float l = (c[0] + c[1]) + c[2];
    const float vr = e0 * e0, vg = e1 * e1, vb = e2 * e2;
    const float vl = (vr + vg) + vb;
    int ok = rtw_denoise_finite(a[0]) && rtw_denoise_finite(a[1]) && rtw_denoise_finite(a[2]);
    ok = ok && rtw_denoise_finite(l) && rtw_denoise_finite(vl);
    for (int32_t ch = 0; ch < gc; ++ch) ok = ok && rtw_denoise_finite(G[(size_t)gc * at + (size_t)ch]);
    return ok ? vl : rtw_denoise_nan();
}

/* the prep record of pixel (x, y) with an albedo image: rtw_denoise_prep_pixel on the demodulated inputs */
RTW_HD rtw_denoise_rec rtw_denoise_prep_pixel_albedo(const float* C, const float* E, const float* G, const float* A,
                                                     int32_t gc, int32_t W, int32_t H, int32_t x, int32_t y) {
    const size_t at = (size_t)y * (size_t)W + (size_t)x;
    float c[3], cq[3];
    const int ok = rtw_denoise_finite(rtw_denoise_m_albedo(C, E, G, A, gc, at, c));
    float sk = 0.0f, sv = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        for (int dx = -1; dx <= 1; ++dx) {
            const int32_t qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float m = rtw_denoise_m_albedo(C, E, G, A, gc, (size_t)qy * (size_t)W + (size_t)qx, cq);
            if (!rtw_denoise_finite(m)) continue;
            const float kk = rtw_denoise_k(dy) * rtw_denoise_k(dx);
            sk = sk + kk;
            sv = sv + kk * m;
        }
    }
    rtw_denoise_rec r;
    r.r = c[0];
    r.g = c[1];
    r.b = c[2];
    r.w = ok ? sv / sk : rtw_denoise_nan();
    return r;
}

/* The post-step of pixel `at`: the last record f times D where the pixel was in at prep, else the input colour.
 * Prep marks a pixel it leaves out with w = NaN and a level hands such a record on as it is; a pixel that was in
 * never gets a NaN w (sv / sk and s2 / (sw * sw) divide sums of non-negative terms by sk > 0 and sw >= 9/64: they
 * may reach +inf, never NaN).  So f.w is NaN exactly for the pixels that were left out. */
RTW_HD __attribute__((always_inline)) void rtw_denoise_remodulate(const float* C, const float* A, size_t at,
                                                                  rtw_denoise_rec f, float o[3]) {
    const int ok = f.w == f.w;
    o[0] = ok ? f.r * rtw_denoise_d(A[3 * at]) : C[3 * at];
    o[1] = ok ? f.g * rtw_denoise_d(A[3 * at + 1]) : C[3 * at + 1];
    o[2] = ok ? f.b * rtw_denoise_d(A[3 * at + 2]) : C[3 * at + 2];
}

/* the guide of pixel `at`, padded with zeros */
RTW_HD rtw_denoise_rec rtw_denoise_guide_pixel(const float* G, int32_t gc, size_t at) {
    rtw_denoise_rec g;
    g.r = gc > 0 ? G[(size_t)gc * at] : 0.0f;
    g.g = gc > 1 ? G[(size_t)gc * at + 1] : 0.0f;
    g.b = gc > 2 ? G[(size_t)gc * at + 2] : 0.0f;
    g.w = gc > 3 ? G[(size_t)gc * at + 3] : 0.0f;
    return g;
}

/* one tap's guide weight; gc channels of the padded guides, in order */
RTW_HD __attribute__((always_inline)) float rtw_denoise_wg(rtw_denoise_rec gq, rtw_denoise_rec gp, int32_t gc, float inv_sg2) {
    float d2 = 0.0f, d;
    if (gc > 0) { d = gq.r - gp.r; d2 = d2 + d * d; }
    if (gc > 1) { d = gq.g - gp.g; d2 = d2 + d * d; }
    if (gc > 2) { d = gq.b - gp.b; d2 = d2 + d * d; }
    if (gc > 3) { d = gq.w - gp.w; d2 = d2 + d * d; }
    float t = 1.0f - d2 * inv_sg2;
    if (t < 0.0f) t = 0.0f;
    return t * t;
}

/* pixel (x, y) of level `step` (1 << i): R the level's input records, G4 the padded guides (read only when
 * gc > 0).  Always inlined: a kernel's constant gc folds, and its loads stay global ones. */
RTW_HD __attribute__((always_inline)) rtw_denoise_rec rtw_denoise_level_pixel(const rtw_denoise_rec* R, const rtw_denoise_rec* G4, int32_t gc, int32_t W,
                                               int32_t H, int32_t x, int32_t y, int32_t step, float sigma_l,
                                               float inv_sg2) {
    const size_t at = (size_t)y * (size_t)W + (size_t)x;
    const rtw_denoise_rec p = R[at];
    if (!rtw_denoise_finite(p.w)) return p;
    rtw_denoise_rec gp = p; /* (unused when gc == 0) */
    if (gc > 0) gp = G4[at];
    const float lp = (p.r + p.g) + p.b;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s2 = 0.0f;
    /* Straight-line: a skipped tap reads the centre's address instead and its sums are dropped by a select, so
     * that the 25 taps' loads issue together and stay 16 bytes wide. */
    RTW_DENOISE_UNROLL
    for (int dy = -2; dy <= 2; ++dy) {
        RTW_DENOISE_UNROLL
        for (int dx = -2; dx <= 2; ++dx) {
            const int64_t qx = (int64_t)x + (int64_t)step * dx;
            const int64_t qy = (int64_t)y + (int64_t)step * dy;
            const int inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
            const size_t qat = inside ? (size_t)qy * (size_t)W + (size_t)qx : at;
            const rtw_denoise_rec q = R[qat];
            const int take = inside && rtw_denoise_finite(q.w);
            const float lq = (q.r + q.g) + q.b;
            const float xx = __builtin_fabsf(lq - lp) / (sigma_l * __builtin_sqrtf(p.w + q.w) + 1e-6f);
            const float wl = 1.0f / (1.0f + xx * xx);
            const float wg = gc > 0 ? rtw_denoise_wg(G4[qat], gp, gc, inv_sg2) : 1.0f;
            const float w = (rtw_denoise_h(dy) * rtw_denoise_h(dx)) * (wl * wg);
            sw = take ? sw + w : sw;
            sr = take ? sr + w * q.r : sr;
            sg = take ? sg + w * q.g : sg;
            sb = take ? sb + w * q.b : sb;
            s2 = take ? s2 + (w * w) * q.w : s2;
        }
    }
    rtw_denoise_rec o;
    o.r = sr / sw;
    o.g = sg / sw;
    o.b = sb / sw;
    o.w = s2 / (sw * sw);
    return o;
}

/* The whole filter on host arrays, pixel after pixel: the host form of the device's three kernels.  `scratch`
 * holds RTW_DENOISE_SCRATCH_RECS * width * height records.  out may be color (the prep pass reads the inputs
 * first); out_variance may be NULL; guide may be NULL when guide_channels is 0; albedo may be NULL (no
 * demodulation).  0, or -1 for params rtw_denoise_check refuses. */
RTW_HD int rtw_denoise_image_albedo(const rtw_denoise_params* p, const float* color, const float* std_err,
                                    const float* guide, const float* albedo, float* out, float* out_variance,
                                    rtw_denoise_rec* scratch) {
    if (rtw_denoise_check(p) != 0) return -1;
    const int32_t W = p->width, H = p->height, gc = p->guide_channels;
    const size_t n = (size_t)W * (size_t)H;
    rtw_denoise_rec* src = scratch;
    rtw_denoise_rec* dst = scratch + n;
    rtw_denoise_rec* G4 = scratch + 2 * n;
    const float inv_sg2 = rtw_denoise_inv_sg2(p->sigma_g);
    for (int32_t y = 0; y < H; ++y) {
        for (int32_t x = 0; x < W; ++x) {
            const size_t at = (size_t)y * (size_t)W + (size_t)x;
            src[at] = albedo ? rtw_denoise_prep_pixel_albedo(color, std_err, guide, albedo, gc, W, H, x, y)
                             : rtw_denoise_prep_pixel(color, std_err, guide, gc, W, H, x, y);
            G4[at] = rtw_denoise_guide_pixel(guide, gc, at);
        }
    }
    for (int32_t i = 0; i < p->iterations; ++i) {
        for (int32_t y = 0; y < H; ++y)
            for (int32_t x = 0; x < W; ++x)
                dst[(size_t)y * (size_t)W + (size_t)x] =
                    rtw_denoise_level_pixel(src, G4, gc, W, H, x, y, (int32_t)1 << i, p->sigma_l, inv_sg2);
        rtw_denoise_rec* t = src;
        src = dst;
        dst = t;
    }
    for (size_t at = 0; at < n; ++at) {
        if (albedo) {  /* (reads the pixel's own inputs before writing it: out may be color) */
            float o[3];
            rtw_denoise_remodulate(color, albedo, at, src[at], o);
            out[3 * at] = o[0];
            out[3 * at + 1] = o[1];
            out[3 * at + 2] = o[2];
        } else {
            out[3 * at] = src[at].r;
            out[3 * at + 1] = src[at].g;
            out[3 * at + 2] = src[at].b;
        }
        if (out_variance) out_variance[at] = src[at].w;
    }
    return 0;
}

RTW_HD int rtw_denoise_image(const rtw_denoise_params* p, const float* color, const float* std_err, const float* guide,
                             float* out, float* out_variance, rtw_denoise_rec* scratch) {
    return rtw_denoise_image_albedo(p, color, std_err, guide, 0, out, out_variance, scratch);
}

#ifdef __cplusplus
}
#endif

#endif /* RTW_DENOISE_H */
