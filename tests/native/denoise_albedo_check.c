/* The preview denoiser with albedo demodulation on the host (include/rtw_denoise.h): rtw_denoise_image_albedo,
 * the header loop behind librtw.so's rtw_denoise_host_albedo, run stand-alone so that a sanitizer build can watch
 * every index it forms.
 *   denoise_albedo_check FILE
 * FILE: int32 width, height, iterations, guide_channels, has_albedo, alias; float sigma_l, sigma_g; then
 * width * height * 3 floats of colour, as many of standard error, width * height * guide_channels of guide and,
 * with has_albedo, width * height * 3 of albedo.  alias != 0: the output is written over the colour array (the
 * call's `out may be color`).  Every array is copied into an exact-size heap block, the scratch included.
 * Prints "rc R pixels N" and "sum X Y": the 64-bit FNV-1a checksums of the output image's and of the output
 * variance's f32 bit patterns, pixel after pixel, every NaN counted as 0x7FC00000.  Exit status 2 on a short or
 * inconsistent file.  Built with -ffp-contract=off like the kernel. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rtw_denoise.h"

static uint64_t fnv(const float* a, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; ++i) {
        uint32_t u = a[i] != a[i] ? 0x7FC00000u : rtw_f2u(a[i]);
        for (int b = 0; b < 4; ++b) {
            h ^= (u >> (8 * b)) & 0xFFu;
            h *= 0x100000001B3ull;
        }
    }
    return h;
}

static float* read_floats(FILE* f, size_t n) {
    float* a = (float*)malloc((n ? n : 1) * sizeof(float));
    if (!a || fread(a, 4, n, f) != n) exit(2);
    return a;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t g[6];
    float s[2];
    if (fread(g, 4, 6, f) != 6 || fread(s, 4, 2, f) != 2) return 2;
    rtw_denoise_params p;
    memset(&p, 0, sizeof(p));
    p.width = g[0];
    p.height = g[1];
    p.iterations = g[2];
    p.guide_channels = g[3];
    p.sigma_l = s[0];
    p.sigma_g = s[1];
    if (rtw_denoise_check(&p) != 0) return 2;
    const size_t n = (size_t)p.width * (size_t)p.height;
    float* color = read_floats(f, 3 * n);
    float* se = read_floats(f, 3 * n);
    float* guide = p.guide_channels > 0 ? read_floats(f, (size_t)p.guide_channels * n) : 0;
    float* albedo = g[4] ? read_floats(f, 3 * n) : 0;
    fclose(f);
    float* out = g[5] ? color : (float*)malloc(3 * n * sizeof(float));
    float* var = (float*)malloc(n * sizeof(float));
    rtw_denoise_rec* scratch = (rtw_denoise_rec*)aligned_alloc(16, RTW_DENOISE_SCRATCH_RECS * n * sizeof(rtw_denoise_rec));
    if (!out || !var || !scratch) return 2;
    const int rc = rtw_denoise_image_albedo(&p, color, se, guide, albedo, out, var, scratch);
    printf("rc %d pixels %llu\n", rc, (unsigned long long)n);
    printf("sum %016llx %016llx\n", (unsigned long long)fnv(out, 3 * n), (unsigned long long)fnv(var, n));
    if (out != color) free(out);
    free(color);
    free(se);
    free(guide);
    free(albedo);
    free(var);
    free(scratch);
    return 0;
}
