/*
 * rtw_aov_parts.h -- the packed record of one partition's first-hit AOV state (rtw_aov_pack, rtw_aov_merge_parts,
 * rtw.h): a section table for rtw_parts.h, which holds the check, the placement and the merge.
 * Plain C99 (gcc) and HIP C++ (hipcc) from one text.
 *
 * An AOV accumulator's planes are SoA over its own slots, 64 per 8 x 8 tile (a wave is a tile), so every plane is
 * one section of 64 words a tile and a merge places whole 256-byte tile blocks.  The record: kind = channels
 * (RTW_AOV_*), tag = RTW_AOV_PARTS_MAGIC (a colour record holds 0 there), and
 *   albedo   3 planes of f32   with RTW_AOV_ALBEDO
 *   normal   3 planes of f32   with RTW_AOV_NORMAL
 *   depth    1 plane of f32    with RTW_AOV_DEPTH
 *   hits     1 plane of u32    always
 */
#ifndef RTW_AOV_PARTS_H
#define RTW_AOV_PARTS_H

#include "rtw_parts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_AOV_PARTS_MAGIC 0x564F4152u /* "RAOV" */
#define RTW_AOV_PARTS_PER_TILE 64
#define RTW_AOV_CHANNELS_ALL (RTW_AOV_ALBEDO | RTW_AOV_NORMAL | RTW_AOV_DEPTH)

/* The layout of the AOV records of `part_count` parts of params' frame: 1 .. 8 sections, one a plane, hits last.
 * 0, or -1 for what rtw_parts_frame refuses, a tile other than 8 x 8 (0 counts as 8), or channels 0 or unknown. */
RTW_HD int rtw_aov_parts_layout_of(const rtw_render_params* params, uint32_t channels, int32_t part_count, rtw_parts_layout* L) {
    if (channels == 0 || (channels & ~RTW_AOV_CHANNELS_ALL)) return -1;
    if (rtw_parts_frame(params, part_count, L) != 0 || L->per_tile != RTW_AOV_PARTS_PER_TILE) return -1;
    if ((params->tile_width > 0 ? params->tile_width : 8) != 8) return -1;
    /* (slots are 32-bit with the sign bit free in the AOV kernels) */
    if ((int64_t)L->n_tiles * RTW_AOV_PARTS_PER_TILE >= (int64_t)0x7FFFFFFF) return -1;
    L->kind = channels;
    L->tag = RTW_AOV_PARTS_MAGIC;
    const int planes = ((channels & RTW_AOV_ALBEDO) ? 3 : 0) + ((channels & RTW_AOV_NORMAL) ? 3 : 0) + ((channels & RTW_AOV_DEPTH) ? 1 : 0) + 1;
    for (int k = 0; k < planes; ++k) rtw_parts_add_section(L, RTW_AOV_PARTS_PER_TILE);
    return 0;
}

#ifdef __cplusplus
}
#endif

#endif /* RTW_AOV_PARTS_H */
