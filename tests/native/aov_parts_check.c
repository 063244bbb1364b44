/* aov_parts_check.c -- rtw_aov_parts.h's merge on host arrays, stand-alone (tests/test_aov_parts_host.py builds it
 * plain and with -fsanitize=address,undefined and runs it alone).  Reads one case file:
 *   int32 width, height, part_count; uint32 channels; uint64 stride_words;
 *   part_count * stride_words uint32: the gathered records
 * merges them into arrays of exactly the whole image's size (so that a word placed out of range is an error the
 * sanitizer sees) and prints
 *   rc 0 samples <n>      or, refused,      rc -1 field <name> at <record>
 *   fnv <albedo> <normal> <depth> <hits>     (64-bit FNV-1a over the arrays' bytes; 0 for an absent array)
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
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t g[3];
    uint32_t channels;
    uint64_t stride;
    if (fread(g, sizeof(g), 1, f) != 1 || fread(&channels, sizeof(channels), 1, f) != 1 || fread(&stride, sizeof(stride), 1, f) != 1)
        return 2;
    const size_t n_words = (size_t)g[2] * (size_t)stride;
    uint32_t* gathered = words(n_words);
    if (fread(gathered, sizeof(uint32_t), n_words, f) != n_words) return 2;
    fclose(f);
    rtw_render_params p;
    memset(&p, 0, sizeof(p));
    p.width = g[0];
    p.height = g[1];
    const size_t slots = (size_t)((g[0] + 7) / 8) * (size_t)((g[1] + 7) / 8) * 64;
    uint32_t* albedo = (channels & RTW_AOV_ALBEDO) ? words(3 * slots) : 0;
    uint32_t* normal = (channels & RTW_AOV_NORMAL) ? words(3 * slots) : 0;
    uint32_t* depth = (channels & RTW_AOV_DEPTH) ? words(slots) : 0;
    uint32_t* hits = words(slots);
    uint32_t samples = 0;
    const char* field = 0;
    int32_t at = 0;
    const int rc = rtw_aov_parts_merge(&p, channels, gathered, stride, g[2], albedo, normal, depth, hits, &samples, &field, &at);
    if (rc != 0)
        printf("rc %d field %s at %d\n", rc, field ? field : "-", (int)at);
    else
        printf("rc 0 samples %" PRIu32 "\n", samples);
    if (rc == 0)
        printf("fnv %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", fnv(albedo, 3 * slots), fnv(normal, 3 * slots),
               fnv(depth, slots), fnv(hits, slots));
    free(gathered);
    free(albedo);
    free(normal);
    free(depth);
    free(hits);
    return 0;
}
