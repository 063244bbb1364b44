/* Finite-sample accumulation on the host (include/rtw_finite.h): rtw_finite_accumulate and rtw_adapt_tiles_finite,
 * the header functions behind librtw.so's rtw_finite_accumulate_host and rtw_adapt_tiles_finite_host, run
 * stand-alone so that a sanitizer build can watch every index they form.
 *   finite_check FILE
 * FILE: int32 width, height, tile_w, tile_h, part_index, part_count; uint32 n_samples, batch, moments, min_samples;
 * float target; then n_samples * slots * 3 floats of colours, sample-major (slots = local tiles * tile_w * tile_h;
 * a padding slot's colours are NaN, so the filter leaves it alone).  The samples are added `batch` at a time; with
 * moments an adapt follows every batch (an adaptive accumulator's run: a stopped tile's sums, squares and kept
 * stay as they were at its stop).  Every array lives in an exact-size heap block.
 * Prints "rc R slots N", then "sum A B C D E F": the 64-bit FNV-1a checksums of the f32 / u32 bit patterns of
 * sums, squares, kept, the resolved image, the standard error and the per-slot e (every NaN counted as 0x7FC00000;
 * without moments B, E and F are 0), then "low K finite Z": the owned slots with kept < 2 and those of them whose
 * e is finite, then per adapt "stop" and the stop map.  Exit status 2 on a short or inconsistent file.  Built with
 * -ffp-contract=off like the kernel. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rtw_finite.h"

static uint64_t fnv_u32(uint64_t h, uint32_t u) {
    for (int b = 0; b < 4; ++b) {
        h ^= (u >> (8 * b)) & 0xFFu;
        h *= 0x100000001B3ull;
    }
    return h;
}

static uint64_t fnv(const float* a, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; ++i) h = fnv_u32(h, a[i] != a[i] ? 0x7FC00000u : rtw_f2u(a[i]));
    return h;
}

static uint64_t fnv_counts(const uint32_t* a, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; ++i) h = fnv_u32(h, a[i]);
    return h;
}

static void* block(size_t bytes) {
    void* p = calloc(bytes ? bytes : 1, 1);
    if (!p) exit(2);
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t g[6];
    uint32_t u[4];
    float target;
    if (fread(g, 4, 6, f) != 6 || fread(u, 4, 4, f) != 4 || fread(&target, 4, 1, f) != 1) return 2;
    const uint32_t n_samples = u[0], batch = u[1], moments = u[2], min_samples = u[3];
    rtw_render_params p;
    memset(&p, 0, sizeof(p));
    p.width = g[0];
    p.height = g[1];
    p.tile_width = g[2];
    p.tile_height = g[3];
    p.part_index = g[4];
    p.part_count = g[5];
    rtw_adapt_geom G;
    if (rtw_adapt_geom_of(&p, &G) != 0 || G.local_tiles < 1 || batch < 1 || n_samples % batch != 0) return 2;
    const int32_t per_tile = G.tile_w * G.tile_h;
    const size_t tiles = (size_t)G.local_tiles, slots = tiles * (size_t)per_tile;
    const size_t batch_floats = (size_t)batch * slots * 3;
    float* sums = (float*)block(3 * slots * sizeof(float));
    float* squares = moments ? (float*)block(3 * slots * sizeof(float)) : 0;
    uint32_t* kept = (uint32_t*)block(slots * sizeof(uint32_t));
    float* sums0 = (float*)block(3 * slots * sizeof(float));
    float* squares0 = (float*)block(3 * slots * sizeof(float));
    uint32_t* kept0 = (uint32_t*)block(slots * sizeof(uint32_t));
    uint32_t* stop = (uint32_t*)block(tiles * sizeof(uint32_t));
    uint32_t* stops = (uint32_t*)block((size_t)(n_samples / batch) * tiles * sizeof(uint32_t));
    int rc = 0, adapts = 0;
    for (uint32_t s0 = 0; s0 < n_samples; s0 += batch) {
        float* colors = (float*)block(batch_floats * sizeof(float)); /* one launch's colour buffer */
        if (fread(colors, 4, batch_floats, f) != batch_floats) return 2;
        memcpy(sums0, sums, 3 * slots * sizeof(float));
        if (moments) memcpy(squares0, squares, 3 * slots * sizeof(float));
        memcpy(kept0, kept, slots * sizeof(uint32_t));
        rtw_finite_accumulate(colors, batch, (uint32_t)slots, sums, squares, kept);
        free(colors);
        for (size_t t = 0; t < tiles; ++t) { /* a stopped tile is frozen */
            if (stop[t] == 0) continue;
            const size_t at = t * (size_t)per_tile, n = (size_t)per_tile;
            memcpy(sums + 3 * at, sums0 + 3 * at, 3 * n * sizeof(float));
            if (moments) memcpy(squares + 3 * at, squares0 + 3 * at, 3 * n * sizeof(float));
            memcpy(kept + at, kept0 + at, n * sizeof(uint32_t));
        }
        if (moments && s0 + batch >= 2) {
            rc |= rtw_adapt_tiles_finite(sums, squares, kept, &p, s0 + batch, target, min_samples, stop);
            memcpy(stops + (size_t)adapts * tiles, stop, tiles * sizeof(uint32_t));
            ++adapts;
        }
    }
    fclose(f);
    float* image = (float*)block(3 * slots * sizeof(float));
    float* se = (float*)block(3 * slots * sizeof(float));
    float* e = (float*)block(slots * sizeof(float));
    unsigned low = 0, low_finite = 0;
    for (size_t t = 0; t < tiles; ++t)
        for (int32_t it = 0; it < per_tile; ++it) {
            const size_t slot = t * (size_t)per_tile + (size_t)it;
            int32_t px, py;
            for (int ch = 0; ch < 3; ++ch) image[3 * slot + ch] = rtw_finite_mean(sums[3 * slot + ch], kept[slot]);
            if (!moments) continue;
            float m;
            for (int ch = 0; ch < 3; ++ch) se[3 * slot + ch] = rtw_adapt_se(sums[3 * slot + ch], squares[3 * slot + ch], kept[slot], &m);
            e[slot] = rtw_adapt_pixel(sums + 3 * slot, squares + 3 * slot, kept[slot]);
            if (rtw_adapt_slot_pixel(&G, (int32_t)t, it, &px, &py) && kept[slot] < 2) {
                ++low;
                low_finite += rtw_adapt_finite(e[slot]) ? 1u : 0u;
            }
        }
    printf("rc %d slots %llu\n", rc, (unsigned long long)slots);
    printf("sum %016llx %016llx %016llx %016llx %016llx %016llx\n", (unsigned long long)fnv(sums, 3 * slots),
           (unsigned long long)(moments ? fnv(squares, 3 * slots) : 0), (unsigned long long)fnv_counts(kept, slots),
           (unsigned long long)fnv(image, 3 * slots), (unsigned long long)(moments ? fnv(se, 3 * slots) : 0),
           (unsigned long long)(moments ? fnv(e, slots) : 0));
    printf("low %u finite %u\n", low, low_finite);
    for (int a = 0; a < adapts; ++a) {
        printf("stop");
        for (size_t t = 0; t < tiles; ++t) printf(" %u", (unsigned)stops[(size_t)a * tiles + t]);
        printf("\n");
    }
    free(sums);
    free(squares);
    free(kept);
    free(sums0);
    free(squares0);
    free(kept0);
    free(stop);
    free(stops);
    free(image);
    free(se);
    free(e);
    return 0;
}
