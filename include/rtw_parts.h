/*
 * rtw_parts.h -- the packed record of one partition's accumulator state and the placement that merges N of them
 * into the whole image's accumulator: one mechanism for the colour accumulator (rtw_accum_pack,
 * rtw_accum_merge_parts) and the first-hit AOV accumulator (rtw_aov_pack, rtw_aov_merge_parts;
 * include/rtw_aov_parts.h).  Plain C99 (gcc) and HIP C++ (hipcc) from one text, like rtw_adapt.h:
 * integer arithmetic only, so the device kernels, the host twins and a numpy restatement place the same words.
 *
 * An accumulator's arrays are tile-major over its own tiles: local tile lt of part (r, N) is tile r + lt * N of
 * the frame, and the whole image's accumulator (part (0, 1)) holds tile t at local index t.  A merge is therefore
 * a placement of whole tile blocks; nothing is added or rounded.
 *
 * A record is a header and an ordered table of up to 8 sections, in 4-byte words.  Section s holds per[s] words
 * for every tile and starts at word at[s]; T0 tiles, those of part (0, N), which owns the most, so the records of
 * all N parts have one size and one set of offsets.  A section's words past the partition's own tiles are zero.
 *   header     8 words: record version (1), kind (what the sections are), part_index, part_count, samples, slots,
 *                       tiles, tag (which accumulator the record belongs to)
 * The colour record (rtw_parts_layout_of): kind = flags (RTW_ACCUM_*), tag = 0, per_tile = tile_w * tile_h, and
 *   sums       3 * per_tile f32 a tile
 *   squares    3 * per_tile f32    with RTW_ACCUM_MOMENTS
 *   kept       per_tile u32        with RTW_ACCUM_FINITE
 *   clamped    per_tile u32        with RTW_ACCUM_CLAMP
 *   lost       3 * per_tile f32    with RTW_ACCUM_CLAMP
 *   tile_stop  1 u32               with RTW_ACCUM_ADAPTIVE (the layout's `stop` section)
 * With RTW_ACCUM_CLAMP the header's last word of a colour record carries the bits of the accumulator's f32 level
 * (the layout's `level`, set by rtw_parts_set_level; 0 without the flag), checked like every other header word.
 */
#ifndef RTW_PARTS_H
#define RTW_PARTS_H

#include "rtw_adapt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_PARTS_VERSION 1u
#define RTW_PARTS_HEADER_WORDS 8
#define RTW_PARTS_MAX_SECTIONS 8
/* the header's words */
#define RTW_PARTS_H_VERSION 0
#define RTW_PARTS_H_KIND 1
#define RTW_PARTS_H_PART_INDEX 2
#define RTW_PARTS_H_PART_COUNT 3
#define RTW_PARTS_H_SAMPLES 4
#define RTW_PARTS_H_SLOTS 5
#define RTW_PARTS_H_TILES 6
#define RTW_PARTS_H_TAG 7

typedef struct rtw_parts_layout {
    uint32_t kind;     /* the header's kind word: the colour accumulator's flags, the AOV accumulator's channels */
    uint32_t tag;      /* the header's tag word: 0 (colour) or RTW_AOV_PARTS_MAGIC */
    int32_t part_count;
    int32_t per_tile;  /* slots of one tile */
    int32_t n_tiles;   /* tiles of the frame */
    int32_t tiles0;    /* T0 */
    uint32_t slots0;   /* S0 = T0 * per_tile */
    int32_t sections;
    /* The section that is a stop map, one word a tile, or -1.  With one, the parts may differ in samples (the
     * whole's is the largest) and every stop must be 0 or within 2 .. its record's samples. */
    int32_t stop;
    uint32_t level;    /* a colour record's last header word: 0, or the bits of the clamp level (RTW_ACCUM_CLAMP) */
    uint32_t per[RTW_PARTS_MAX_SECTIONS]; /* words of one tile */
    uint64_t at[RTW_PARTS_MAX_SECTIONS];  /* the section's first word in a record */
    uint64_t words;                       /* of a record */
} rtw_parts_layout;

/* The frame of a layout: part_count, per_tile, n_tiles, tiles0, slots0 from params (params' own part is not read),
 * no sections yet.  0, or -1 for params no frame takes or part_count < 1. */
RTW_HD int rtw_parts_frame(const rtw_render_params* params, int32_t part_count, rtw_parts_layout* L) {
    rtw_render_params q = *params;
    rtw_adapt_geom g;
    if (part_count < 1) return -1;
    q.part_index = 0;
    q.part_count = part_count;
    if (rtw_adapt_geom_of(&q, &g) != 0) return -1;
    const int64_t n_tiles = (int64_t)g.tiles_x * ((g.height + g.tile_h - 1) / g.tile_h);
    /* (the whole image's slots fit 32 bits too: what an accumulator of part (0, 1) takes) */
    if (n_tiles * g.tile_w * g.tile_h >= (int64_t)0xFFFFFFFF) return -1;
    L->part_count = part_count;
    L->per_tile = g.tile_w * g.tile_h;
    L->n_tiles = (int32_t)n_tiles;
    L->tiles0 = g.local_tiles;
    L->slots0 = (uint32_t)g.local_tiles * (uint32_t)L->per_tile;
    L->sections = 0;
    L->stop = -1;
    L->level = 0u;
    L->words = RTW_PARTS_HEADER_WORDS;
    return 0;
}

/* appends a section of `per` words a tile (the builders stay within RTW_PARTS_MAX_SECTIONS) */
RTW_HD void rtw_parts_add_section(rtw_parts_layout* L, uint32_t per) {
    L->per[L->sections] = per;
    L->at[L->sections] = L->words;
    L->words += (uint64_t)L->tiles0 * per;
    L->sections += 1;
}

/* The layout of the colour records of `part_count` parts of params' frame.  0, or -1 for what rtw_parts_frame
 * refuses or unknown flags. */
RTW_HD int rtw_parts_layout_of(const rtw_render_params* params, uint32_t flags, int32_t part_count, rtw_parts_layout* L) {
    if ((flags & ~(RTW_ACCUM_MOMENTS | RTW_ACCUM_ADAPTIVE | RTW_ACCUM_FINITE | RTW_ACCUM_CLAMP)) ||
        ((flags & RTW_ACCUM_CLAMP) && !(flags & RTW_ACCUM_FINITE)) || rtw_parts_frame(params, part_count, L) != 0)
        return -1;
    L->kind = flags;
    L->tag = 0u;
    rtw_parts_add_section(L, 3u * (uint32_t)L->per_tile);
    if (flags & RTW_ACCUM_MOMENTS) rtw_parts_add_section(L, 3u * (uint32_t)L->per_tile);
    if (flags & RTW_ACCUM_FINITE) rtw_parts_add_section(L, (uint32_t)L->per_tile);
    if (flags & RTW_ACCUM_CLAMP) {
        rtw_parts_add_section(L, (uint32_t)L->per_tile);
        rtw_parts_add_section(L, 3u * (uint32_t)L->per_tile);
    }
    if (flags & RTW_ACCUM_ADAPTIVE) {
        L->stop = L->sections;
        rtw_parts_add_section(L, 1u);
    }
    return 0;
}

/* the clamp level of a colour layout whose flags hold RTW_ACCUM_CLAMP (the records' last header word) */
RTW_HD void rtw_parts_set_level(rtw_parts_layout* L, float level) { L->level = rtw_f2u(level); }

/* a record's last header word: the AOV magic, or a colour record's level word */
RTW_HD uint32_t rtw_parts_last_word(const rtw_parts_layout* L) { return L->tag != 0u ? L->tag : L->level; }

/* the tiles part r owns: t = r, r + N, ... below n_tiles */
RTW_HD int32_t rtw_parts_tiles(const rtw_parts_layout* L, int32_t r) {
    return L->n_tiles > r ? (L->n_tiles - r + L->part_count - 1) / L->part_count : 0;
}

/* The placement.  Word `w` of one of the whole's arrays, whose tiles are `per` words each, comes from this word of
 * the gathered buffer: tile t = w / per is local tile t / N of part t % N, whose record starts at (t % N) * stride.
 * The same expression serves the 16-byte path with every quantity counted in units of 4 words. */
RTW_HD uint64_t rtw_parts_source(uint64_t w, uint32_t per, uint32_t part_count, uint64_t stride, uint64_t section) {
    const uint64_t t = w / per, in = w % per;
    return (t % part_count) * stride + section + (t / part_count) * (uint64_t)per + in;
}

/* The 16-byte path needs every tile block of a section to start and end on 16 bytes inside a record: per_tile a
 * multiple of 4 (then S0 and the section offsets are too), and the section's own words a tile as well (a stop map
 * always goes as dwords).  The callers add the buffers' own alignment and the stride. */
RTW_HD int rtw_parts_wide(const rtw_parts_layout* L, int32_t s) { return L->per_tile % 4 == 0 && L->per[s] % 4 == 0; }

/* A record's header against the layout: 0, or the name of the first field that differs.  A colour record:
 * "version", "flags", "part_index", "part_count", "slots", "tiles", "reserved" (flags with RTW_ACCUM_CLAMP: "clamp",
 * a level other than the layout's); an AOV record: "version", "magic",
 * "channels", "part_index", "part_count", "slots", "tiles".  samples is rtw_parts_check's to compare. */
RTW_HD const char* rtw_parts_check_header(const rtw_parts_layout* L, int32_t r, const uint32_t* h) {
    const uint32_t tiles = (uint32_t)rtw_parts_tiles(L, r);
    if (h[RTW_PARTS_H_VERSION] != RTW_PARTS_VERSION) return "version";
    if (L->tag != 0u && h[RTW_PARTS_H_TAG] != L->tag) return "magic";
    if (h[RTW_PARTS_H_KIND] != L->kind) return L->tag != 0u ? "channels" : "flags";
    if (h[RTW_PARTS_H_PART_INDEX] != (uint32_t)r) return "part_index";
    if (h[RTW_PARTS_H_PART_COUNT] != (uint32_t)L->part_count) return "part_count";
    if (h[RTW_PARTS_H_SLOTS] != tiles * (uint32_t)L->per_tile) return "slots";
    if (h[RTW_PARTS_H_TILES] != tiles) return "tiles";
    if (L->tag == 0u && h[RTW_PARTS_H_TAG] != L->level) return (L->kind & RTW_ACCUM_CLAMP) ? "clamp" : "reserved";
    return (const char*)0;
}

/* The part_count gathered records one after the other: record r's header at headers + r * header_stride and, for a
 * layout with a stop section, its stop map `stop_at` words after its header (the records themselves, or what was
 * read back of them).  0 with *samples, the whole's sample count, or -1 with *field naming what was refused, at[0]
 * the record and, for "tile_stop", at[1] the local tile. */
RTW_HD int rtw_parts_check(const rtw_parts_layout* L, const uint32_t* headers, uint64_t header_stride, uint64_t stop_at,
                           uint32_t* samples, const char** field, int32_t* at) {
    uint32_t n = 0;
    for (int32_t r = 0; r < L->part_count; ++r) {
        const uint32_t* h = headers + (uint64_t)r * header_stride;
        const uint32_t s = h[RTW_PARTS_H_SAMPLES];
        at[0] = r;
        *field = rtw_parts_check_header(L, r, h);
        if (*field) return -1;
        *field = "samples";
        if (L->stop < 0 && r > 0 && s != n) return -1;
        n = s > n ? s : n;
        if (L->stop < 0) continue;
        *field = "tile_stop";
        for (int32_t lt = 0; lt < rtw_parts_tiles(L, r); ++lt) {
            const uint32_t v = h[stop_at + (uint64_t)lt];
            at[1] = lt;
            if (v == 1u || v > s) return -1;
        }
    }
    *field = (const char*)0;
    *samples = n;
    return 0;
}

/* The merge on host arrays (rtw_accum_merge_parts_host, rtw_aov_merge_parts_host of rtw.h): `gathered` holds
 * part_count records at r * stride_words; dst[s] takes section s of the whole, n_tiles * per[s] words; *samples
 * the whole's sample count.  Returns 0 or, with *field and at[2] as rtw_parts_check's ("stride_bytes": a stride
 * below the record's words), -1; nothing is written on a refusal. */
RTW_HD int rtw_parts_merge(const rtw_parts_layout* L, const uint32_t* gathered, uint64_t stride_words, uint32_t* const* dst,
                           uint32_t* samples, const char** field, int32_t* at) {
    uint32_t n = 0;
    at[0] = at[1] = 0;
    *field = "stride_bytes";
    if (stride_words < L->words) return -1;
    if (rtw_parts_check(L, gathered, stride_words, L->stop < 0 ? 0 : L->at[L->stop], &n, field, at) != 0) return -1;
    for (int32_t s = 0; s < L->sections; ++s)
        for (uint64_t w = 0; w < (uint64_t)L->n_tiles * L->per[s]; ++w)
            dst[s][w] = gathered[rtw_parts_source(w, L->per[s], (uint32_t)L->part_count, stride_words, L->at[s])];
    *samples = n;
    return 0;
}

#ifdef __cplusplus
}
#endif

#endif /* RTW_PARTS_H */
