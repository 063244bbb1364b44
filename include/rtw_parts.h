/*
 * rtw_parts.h -- the packed record of one partition's accumulator state and the placement that merges N of
 * them into the whole image's accumulator (rtw_accum_pack, rtw_accum_merge_parts, rtw.h).
 * Plain C99 (gcc) and HIP C++ (hipcc) from one text, like rtw_adapt.h: integer arithmetic only, so the device
 * kernels, the host twin (rtw_accum_merge_parts_host) and a numpy restatement place the same words.
 *
 * An accumulator's sums, squares and kept counts are tile-major over its own tiles: local tile lt of part
 * (r, N) is tile r + lt * N of the frame, and the whole image's accumulator (part (0, 1)) holds tile t at local
 * index t.  A merge is therefore a placement of whole tile blocks; nothing is added or rounded.
 *
 * The record, in 4-byte words (S0, T0: the slots and tiles of part (0, N), which owns the most tiles, so the
 * records of all N parts have one size and one set of section offsets):
 *   header     8 words: record version (1), flags (RTW_ACCUM_*), part_index, part_count, samples, slots, tiles, 0
 *   sums       3 * S0 f32
 *   squares    3 * S0 f32   with RTW_ACCUM_MOMENTS
 *   kept       S0 u32       with RTW_ACCUM_FINITE
 *   tile_stop  T0 u32       with RTW_ACCUM_ADAPTIVE
 * A section's words past the partition's own slots or tiles are zero.
 */
#ifndef RTW_PARTS_H
#define RTW_PARTS_H

#include "rtw_adapt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_PARTS_VERSION 1u
#define RTW_PARTS_HEADER_WORDS 8
/* the header's words */
#define RTW_PARTS_H_VERSION 0
#define RTW_PARTS_H_FLAGS 1
#define RTW_PARTS_H_PART_INDEX 2
#define RTW_PARTS_H_PART_COUNT 3
#define RTW_PARTS_H_SAMPLES 4
#define RTW_PARTS_H_SLOTS 5
#define RTW_PARTS_H_TILES 6
#define RTW_PARTS_H_ZERO 7

typedef struct rtw_parts_layout {
    uint32_t flags;
    int32_t part_count;
    int32_t per_tile; /* slots of one tile: tile_w * tile_h */
    int32_t n_tiles;  /* tiles of the frame */
    int32_t tiles0;   /* T0 */
    uint32_t slots0;  /* S0 = T0 * per_tile */
    /* word offsets of the sections inside a record (an absent section: 0) and the record's words */
    uint64_t sums, squares, kept, stop, words;
} rtw_parts_layout;

/* The layout of the records of `part_count` parts of params' frame (params' own part is not read).  0, or -1
 * for params no frame takes, unknown flags or part_count < 1. */
RTW_HD int rtw_parts_layout_of(const rtw_render_params* params, uint32_t flags, int32_t part_count, rtw_parts_layout* L) {
    rtw_render_params q = *params;
    rtw_adapt_geom g;
    if (part_count < 1 || (flags & ~(RTW_ACCUM_MOMENTS | RTW_ACCUM_ADAPTIVE | RTW_ACCUM_FINITE))) return -1;
    q.part_index = 0;
    q.part_count = part_count;
    if (rtw_adapt_geom_of(&q, &g) != 0) return -1;
    const int64_t n_tiles = (int64_t)g.tiles_x * ((g.height + g.tile_h - 1) / g.tile_h);
    /* (the whole image's slots fit 32 bits too: what an accumulator of part (0, 1) takes) */
    if (n_tiles * g.tile_w * g.tile_h >= (int64_t)0xFFFFFFFF) return -1;
    L->flags = flags;
    L->part_count = part_count;
    L->per_tile = g.tile_w * g.tile_h;
    L->n_tiles = (int32_t)n_tiles;
    L->tiles0 = g.local_tiles;
    L->slots0 = (uint32_t)g.local_tiles * (uint32_t)L->per_tile;
    uint64_t at = RTW_PARTS_HEADER_WORDS;
    L->sums = at;
    at += 3 * (uint64_t)L->slots0;
    L->squares = (flags & RTW_ACCUM_MOMENTS) ? at : 0;
    at += (flags & RTW_ACCUM_MOMENTS) ? 3 * (uint64_t)L->slots0 : 0;
    L->kept = (flags & RTW_ACCUM_FINITE) ? at : 0;
    at += (flags & RTW_ACCUM_FINITE) ? (uint64_t)L->slots0 : 0;
    L->stop = (flags & RTW_ACCUM_ADAPTIVE) ? at : 0;
    at += (flags & RTW_ACCUM_ADAPTIVE) ? (uint64_t)L->tiles0 : 0;
    L->words = at;
    return 0;
}

/* the tiles part r owns: t = r, r + N, ... below n_tiles */
RTW_HD int32_t rtw_parts_tiles(const rtw_parts_layout* L, int32_t r) {
    return L->n_tiles > r ? (L->n_tiles - r + L->part_count - 1) / L->part_count : 0;
}

/* The placement.  Word `w` of one of the whole's arrays, whose tiles are `per` words each (3 * per_tile for sums
 * and squares, per_tile for kept, 1 for tile_stop), comes from this word of the gathered buffer: tile t = w / per
 * is local tile t / N of part t % N, whose record starts at (t % N) * stride.  The same expression serves the
 * 16-byte path with every quantity counted in units of 4 words. */
RTW_HD uint64_t rtw_parts_source(uint64_t w, uint32_t per, uint32_t part_count, uint64_t stride, uint64_t section) {
    const uint64_t t = w / per, in = w % per;
    return (t % part_count) * stride + section + (t / part_count) * (uint64_t)per + in;
}

/* The 16-byte path needs every tile block of every section to start and end on 16 bytes inside a record:
 * per_tile a multiple of 4 (then S0 and the section offsets are too).  The callers add the buffer's own
 * alignment and the stride. */
RTW_HD int rtw_parts_wide(const rtw_parts_layout* L) { return L->per_tile % 4 == 0; }

/* A record's header against the layout: 0, or the name of the first field that differs ("version", "flags",
 * "part_index", "part_count", "slots", "tiles", "reserved").  samples is the caller's to compare. */
RTW_HD const char* rtw_parts_check_header(const rtw_parts_layout* L, int32_t r, const uint32_t* h) {
    const uint32_t tiles = (uint32_t)rtw_parts_tiles(L, r);
    if (h[RTW_PARTS_H_VERSION] != RTW_PARTS_VERSION) return "version";
    if (h[RTW_PARTS_H_FLAGS] != L->flags) return "flags";
    if (h[RTW_PARTS_H_PART_INDEX] != (uint32_t)r) return "part_index";
    if (h[RTW_PARTS_H_PART_COUNT] != (uint32_t)L->part_count) return "part_count";
    if (h[RTW_PARTS_H_SLOTS] != tiles * (uint32_t)L->per_tile) return "slots";
    if (h[RTW_PARTS_H_TILES] != tiles) return "tiles";
    if (h[RTW_PARTS_H_ZERO] != 0u) return "reserved";
    return (const char*)0;
}

/* rtw_accum_merge_parts on host arrays (rtw.h): `gathered` holds part_count records at r * stride_bytes; sums,
 * squares and kept take the whole's 3 * slots, 3 * slots and slots entries, tile_stop its tiles (each non-null
 * exactly when `flags` calls for it), *samples the whole's sample count.  Returns 0 or, with *field naming what
 * was refused, -1; nothing is written on a refusal.  stop_at: the record and local tile of a refused stop. */
RTW_HD int rtw_parts_merge(const rtw_render_params* params, uint32_t flags, const uint32_t* gathered, uint64_t stride_words,
                           int32_t part_count, uint32_t* sums, uint32_t* squares, uint32_t* kept, uint32_t* tile_stop,
                           uint32_t* samples, const char** field, int32_t* stop_at) {
    rtw_parts_layout L;
    *field = "params";
    if (rtw_parts_layout_of(params, flags, part_count, &L) != 0) return -1;
    *field = "stride_bytes";
    if (stride_words < L.words) return -1;
    uint32_t n = 0;
    for (int32_t r = 0; r < part_count; ++r) {
        const uint32_t* h = gathered + (uint64_t)r * stride_words;
        const char* bad = rtw_parts_check_header(&L, r, h);
        if (bad) {
            *field = bad;
            stop_at[0] = r;
            return -1;
        }
        const uint32_t s = h[RTW_PARTS_H_SAMPLES];
        *field = "samples";
        stop_at[0] = r;
        if (!(flags & RTW_ACCUM_ADAPTIVE) && r > 0 && s != n) return -1;
        n = s > n ? s : n;
        if (flags & RTW_ACCUM_ADAPTIVE) {
            *field = "tile_stop";
            for (int32_t lt = 0; lt < rtw_parts_tiles(&L, r); ++lt) {
                const uint32_t v = h[L.stop + (uint64_t)lt];
                stop_at[1] = lt;
                if (v == 1u || v > s) return -1;
            }
        }
    }
    *field = (const char*)0;
    const uint64_t slots = (uint64_t)L.n_tiles * (uint64_t)L.per_tile;
    const uint32_t per3 = 3u * (uint32_t)L.per_tile;
    for (uint64_t w = 0; w < 3 * slots; ++w) {
        sums[w] = gathered[rtw_parts_source(w, per3, (uint32_t)part_count, stride_words, L.sums)];
        if (flags & RTW_ACCUM_MOMENTS) squares[w] = gathered[rtw_parts_source(w, per3, (uint32_t)part_count, stride_words, L.squares)];
    }
    if (flags & RTW_ACCUM_FINITE)
        for (uint64_t w = 0; w < slots; ++w)
            kept[w] = gathered[rtw_parts_source(w, (uint32_t)L.per_tile, (uint32_t)part_count, stride_words, L.kept)];
    if (flags & RTW_ACCUM_ADAPTIVE)
        for (uint64_t w = 0; w < (uint64_t)L.n_tiles; ++w)
            tile_stop[w] = gathered[rtw_parts_source(w, 1u, (uint32_t)part_count, stride_words, L.stop)];
    *samples = n;
    return 0;
}

#ifdef __cplusplus
}
#endif

#endif /* RTW_PARTS_H */
