/*
 * rtw_aov_parts.h -- the packed record of one partition's first-hit AOV state and the placement that merges N of
 * them into the whole image's AOV accumulator (rtw_aov_pack, rtw_aov_merge_parts, rtw.h).
 * Plain C99 (gcc) and HIP C++ (hipcc) from one text, like rtw_parts.h, whose placement it reuses: integer
 * arithmetic only, so the device kernels, the host twin (rtw_aov_merge_parts_host) and a numpy restatement place
 * the same words.
 *
 * An AOV accumulator's planes are SoA over its own slots, 64 per 8 x 8 tile (a wave is a tile): local tile lt of
 * part (r, N) is tile r + lt * N of the frame, and the whole image's accumulator (part (0, 1)) holds tile t at
 * local index t.  Every plane is tile-major with 64 words per tile, so a merge places whole 256-byte tile blocks
 * (rtw_parts_source with per = 64); nothing is added or rounded.
 *
 * The record, in 4-byte words (S0, T0: the slots and tiles of part (0, N), which owns the most tiles, so the
 * records of all N parts have one size and one set of plane offsets):
 *   header   8 words: record version (1), channels (RTW_AOV_*), part_index, part_count, samples, slots, tiles,
 *                     RTW_AOV_PARTS_MAGIC (a colour record of rtw_parts.h holds 0 there)
 *   albedo   3 planes of S0 f32   with RTW_AOV_ALBEDO
 *   normal   3 planes of S0 f32   with RTW_AOV_NORMAL
 *   depth    1 plane of S0 f32    with RTW_AOV_DEPTH
 *   hits     1 plane of S0 u32    always
 * A plane's words past the partition's own slots are zero.
 */
#ifndef RTW_AOV_PARTS_H
#define RTW_AOV_PARTS_H

#include "rtw_parts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_AOV_PARTS_VERSION 1u
#define RTW_AOV_PARTS_MAGIC 0x564F4152u /* "RAOV" */
#define RTW_AOV_PARTS_PER_TILE 64
/* the header's words: rtw_parts.h's, with the channels in the flags' word and the magic in the reserved one */
#define RTW_AOV_PARTS_H_CHANNELS RTW_PARTS_H_FLAGS
#define RTW_AOV_PARTS_H_MAGIC RTW_PARTS_H_ZERO
#define RTW_AOV_CHANNELS_ALL (RTW_AOV_ALBEDO | RTW_AOV_NORMAL | RTW_AOV_DEPTH)

typedef struct rtw_aov_parts_layout {
    uint32_t channels;
    int32_t part_count;
    int32_t n_tiles; /* tiles of the frame */
    int32_t tiles0;  /* T0 */
    uint32_t slots0; /* S0 = T0 * 64 */
    int32_t planes;  /* planes of a record, hits included: 1 .. 8 */
    /* word offsets of the sections inside a record (an absent section: 0) and the record's words */
    uint64_t albedo, normal, depth, hits, words;
} rtw_aov_parts_layout;

/* The layout of the records of `part_count` parts of params' frame (params' own part is not read).  0, or -1 for
 * params no frame takes, a tile other than 8 x 8 (0 counts as 8), channels 0 or unknown, or part_count < 1. */
RTW_HD int rtw_aov_parts_layout_of(const rtw_render_params* params, uint32_t channels, int32_t part_count,
                                   rtw_aov_parts_layout* L) {
    rtw_parts_layout C;
    if (channels == 0 || (channels & ~RTW_AOV_CHANNELS_ALL)) return -1;
    if (rtw_parts_layout_of(params, 0u, part_count, &C) != 0 || C.per_tile != RTW_AOV_PARTS_PER_TILE) return -1;
    if ((params->tile_width > 0 ? params->tile_width : 8) != 8) return -1;
    /* (slots are 32-bit with the sign bit free in the AOV kernels) */
    if ((int64_t)C.n_tiles * RTW_AOV_PARTS_PER_TILE >= (int64_t)0x7FFFFFFF) return -1;
    L->channels = channels;
    L->part_count = part_count;
    L->n_tiles = C.n_tiles;
    L->tiles0 = C.tiles0;
    L->slots0 = C.slots0;
    uint64_t at = RTW_PARTS_HEADER_WORDS;
    L->albedo = (channels & RTW_AOV_ALBEDO) ? at : 0;
    at += (channels & RTW_AOV_ALBEDO) ? 3 * (uint64_t)L->slots0 : 0;
    L->normal = (channels & RTW_AOV_NORMAL) ? at : 0;
    at += (channels & RTW_AOV_NORMAL) ? 3 * (uint64_t)L->slots0 : 0;
    L->depth = (channels & RTW_AOV_DEPTH) ? at : 0;
    at += (channels & RTW_AOV_DEPTH) ? (uint64_t)L->slots0 : 0;
    L->hits = at;
    at += (uint64_t)L->slots0;
    L->words = at;
    L->planes = ((channels & RTW_AOV_ALBEDO) ? 3 : 0) + ((channels & RTW_AOV_NORMAL) ? 3 : 0) + ((channels & RTW_AOV_DEPTH) ? 1 : 0) + 1;
    return 0;
}

/* the tiles part r owns: t = r, r + N, ... below n_tiles */
RTW_HD int32_t rtw_aov_parts_tiles(const rtw_aov_parts_layout* L, int32_t r) {
    return L->n_tiles > r ? (L->n_tiles - r + L->part_count - 1) / L->part_count : 0;
}

/* Word `w` of plane `plane` (0 .. planes - 1, in record order) of the whole comes from this word of the gathered
 * buffer.  The planes of a record follow one another S0 words apart, and every tile block starts on 16 bytes
 * inside a record: the same expression serves the 16-byte path with every quantity counted in units of 4 words. */
RTW_HD uint64_t rtw_aov_parts_source(uint64_t w, uint32_t plane, uint32_t per, uint32_t part_count, uint64_t stride,
                                     uint64_t header, uint64_t plane_words) {
    return rtw_parts_source(w, per, part_count, stride, header + (uint64_t)plane * plane_words);
}

/* A record's header against the layout: 0, or the name of the first field that differs ("version", "magic",
 * "channels", "part_index", "part_count", "slots", "tiles").  samples is the caller's to compare. */
RTW_HD const char* rtw_aov_parts_check_header(const rtw_aov_parts_layout* L, int32_t r, const uint32_t* h) {
    const uint32_t tiles = (uint32_t)rtw_aov_parts_tiles(L, r);
    if (h[RTW_PARTS_H_VERSION] != RTW_AOV_PARTS_VERSION) return "version";
    if (h[RTW_AOV_PARTS_H_MAGIC] != RTW_AOV_PARTS_MAGIC) return "magic";
    if (h[RTW_AOV_PARTS_H_CHANNELS] != L->channels) return "channels";
    if (h[RTW_PARTS_H_PART_INDEX] != (uint32_t)r) return "part_index";
    if (h[RTW_PARTS_H_PART_COUNT] != (uint32_t)L->part_count) return "part_count";
    if (h[RTW_PARTS_H_SLOTS] != tiles * (uint32_t)RTW_AOV_PARTS_PER_TILE) return "slots";
    if (h[RTW_PARTS_H_TILES] != tiles) return "tiles";
    return (const char*)0;
}

/* The headers of part_count gathered records, `header_stride` words apart (the records themselves, or their
 * headers read back one after the other): 0 with *samples, or -1 with *field naming what was refused and *at
 * the record. */
RTW_HD int rtw_aov_parts_check(const rtw_aov_parts_layout* L, const uint32_t* headers, uint64_t header_stride,
                               uint32_t* samples, const char** field, int32_t* at) {
    uint32_t n = 0;
    for (int32_t r = 0; r < L->part_count; ++r) {
        const uint32_t* h = headers + (uint64_t)r * header_stride;
        const char* bad = rtw_aov_parts_check_header(L, r, h);
        *at = r;
        if (bad) {
            *field = bad;
            return -1;
        }
        if (r > 0 && h[RTW_PARTS_H_SAMPLES] != n) {
            *field = "samples";
            return -1;
        }
        n = h[RTW_PARTS_H_SAMPLES];
    }
    *field = (const char*)0;
    *samples = n;
    return 0;
}

/* rtw_aov_merge_parts on host arrays (rtw.h): `gathered` holds part_count records at r * stride_words; albedo and
 * normal take the whole's 3 planes of `slots` words each, depth and hits one plane (albedo, normal, depth non-null
 * exactly when `channels` holds them), *samples the whole's sample count.  Returns 0 or, with *field naming what
 * was refused and *at the record, -1; nothing is written on a refusal. */
RTW_HD int rtw_aov_parts_merge(const rtw_render_params* params, uint32_t channels, const uint32_t* gathered,
                               uint64_t stride_words, int32_t part_count, uint32_t* albedo, uint32_t* normal,
                               uint32_t* depth, uint32_t* hits, uint32_t* samples, const char** field, int32_t* at) {
    rtw_aov_parts_layout L;
    *at = 0;
    *field = "params";
    if (rtw_aov_parts_layout_of(params, channels, part_count, &L) != 0) return -1;
    *field = "stride_bytes";
    if (stride_words < L.words) return -1;
    uint32_t n = 0;
    if (rtw_aov_parts_check(&L, gathered, stride_words, &n, field, at) != 0) return -1;
    const uint64_t slots = (uint64_t)L.n_tiles * RTW_AOV_PARTS_PER_TILE;
    uint32_t plane = 0;
    for (int c = 0; c < 4; ++c) {
        uint32_t* dst = c == 0 ? albedo : c == 1 ? normal : c == 2 ? depth : hits;
        const int count = c < 2 ? 3 : 1;
        if (c < 3 && !(channels & (1u << c))) continue;
        for (int k = 0; k < count; ++k, ++plane)
            for (uint64_t w = 0; w < slots; ++w)
                dst[(uint64_t)k * slots + w] = gathered[rtw_aov_parts_source(w, plane, RTW_AOV_PARTS_PER_TILE, (uint32_t)part_count,
                                                                             stride_words, RTW_PARTS_HEADER_WORDS, L.slots0)];
    }
    *samples = n;
    return 0;
}

#ifdef __cplusplus
}
#endif

#endif /* RTW_AOV_PARTS_H */
