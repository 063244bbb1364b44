/* parts_check.c -- rtw_parts.h's merge on host arrays, stand-alone, for colour and AOV records
 * (tests/test_parts_host.py and tests/test_aov_parts_host.py build it plain and with -fsanitize=address,undefined
 * and run it alone).  argv: the kind ("colour" or "aov") and one case file,
 *   colour: int32 width, height, tile_w, tile_h, part_count; uint32 flags; uint64 stride_words;
 *   aov:    int32 width, height, part_count; uint32 channels; uint64 stride_words;
 *   then part_count * stride_words uint32: the gathered records
 * merges them into arrays of exactly the whole image's size (so that a word placed out of range is an error the
 * sanitizer sees) and prints
 *   rc 0 samples <n>      or, refused,      rc -1 field <name> at <record> <tile>     (aov: at <record>)
 *   fnv <sums> <squares> <kept> <tile_stop>     or     fnv <albedo> <normal> <depth> <hits>
 *       (64-bit FNV-1a over the arrays' bytes; 0 for an absent array)
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rtw_aov_parts.h"

static uint64_t fnv(const uint32_t* a, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    if (!a) return 0;
    for (size_t i = 0; i < n; ++i)
        for (int b = 0; b < 4; ++b) h = (h ^ ((a[i] >> (8 * b)) & 0xFFu)) * 0x100000001B3ull;
    return h;
}

static uint32_t* words(size_t n) {
    uint32_t* p = (uint32_t*)malloc(n ? n * sizeof(uint32_t) : 1);
    if (!p) exit(3);
    memset(p, 0xAB, n * sizeof(uint32_t));
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[1], "colour") != 0 && strcmp(argv[1], "aov") != 0)) return 2;
    const int aov = strcmp(argv[1], "aov") == 0;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    int32_t g[5] = {0, 0, 8, 8, 0}; /* width, height, tile, part_count */
    uint32_t kind;
    uint64_t stride;
    if (fread(g, sizeof(int32_t), 2, f) != 2 || (!aov && fread(g + 2, sizeof(int32_t), 2, f) != 2) || fread(g + 4, sizeof(int32_t), 1, f) != 1 ||
        fread(&kind, sizeof(kind), 1, f) != 1 || fread(&stride, sizeof(stride), 1, f) != 1)
        return 2;
    const size_t n_words = (size_t)g[4] * (size_t)stride;
    uint32_t* gathered = words(n_words);
    if (fread(gathered, sizeof(uint32_t), n_words, f) != n_words) return 2;
    fclose(f);
    rtw_render_params p;
    memset(&p, 0, sizeof(p));
    p.width = g[0];
    p.height = g[1];
    p.tile_width = aov ? 0 : g[2];
    p.tile_height = aov ? 0 : g[3];
    const size_t tiles = (size_t)((g[0] + g[2] - 1) / g[2]) * (size_t)((g[1] + g[3] - 1) / g[3]);
    const size_t slots = tiles * (size_t)g[2] * (size_t)g[3];
    /* The four arrays of the kind in the order of the fnv line, each of exactly its own size, and the sections of
     * the record they hold: colour sums, squares, kept, tile_stop (the record's order); aov albedo, normal (3
     * planes each), depth, hits. */
    const uint32_t bit[2][4] = {{0u, RTW_ACCUM_MOMENTS, RTW_ACCUM_FINITE, RTW_ACCUM_ADAPTIVE}, {RTW_AOV_ALBEDO, RTW_AOV_NORMAL, RTW_AOV_DEPTH, 0u}}; /* (0: always) */
    const size_t size[2][4] = {{3 * slots, 3 * slots, slots, tiles}, {3 * slots, 3 * slots, slots, slots}};
    uint32_t* out[4];
    uint32_t* dst[RTW_PARTS_MAX_SECTIONS];
    int sections = 0;
    for (int i = 0; i < 4; ++i) {
        out[i] = (!bit[aov][i] || (kind & bit[aov][i])) ? words(size[aov][i]) : 0;
        for (int k = 0; out[i] && k < (aov && i < 2 ? 3 : 1); ++k) dst[sections++] = out[i] + (size_t)k * slots;
    }
    uint32_t samples = 0;
    const char* field = "params";
    int32_t at[2] = {0, 0};
    rtw_parts_layout L;
    int rc = aov ? rtw_aov_parts_layout_of(&p, kind, g[4], &L) : rtw_parts_layout_of(&p, kind, g[4], &L);
    if (rc == 0 && L.sections != sections) return 2;
    if (rc == 0) rc = rtw_parts_merge(&L, gathered, stride, dst, &samples, &field, at);
    if (rc != 0 && aov)
        printf("rc %d field %s at %d\n", rc, field ? field : "-", (int)at[0]);
    else if (rc != 0)
        printf("rc %d field %s at %d %d\n", rc, field ? field : "-", (int)at[0], (int)at[1]);
    else
        printf("rc 0 samples %" PRIu32 "\n", samples);
    if (rc == 0)
        printf("fnv %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", fnv(out[0], size[aov][0]), fnv(out[1], size[aov][1]),
               fnv(out[2], size[aov][2]), fnv(out[3], size[aov][3]));
    free(gathered);
    for (int i = 0; i < 4; ++i) free(out[i]);
    return 0;
}
