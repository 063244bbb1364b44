// rtw_parts.hip -- packing one partition's accumulator state into a record and placing N gathered records into
// the whole image's accumulator: rtw_accum_pack, rtw_accum_merge_parts and rtw_aov_pack,
// rtw_aov_merge_parts of rtw.h, through one pack kernel and one merge kernel.
//
// The layout and the placement are include/rtw_parts.h's, one text for the kernels here, the host twins and a
// numpy restatement; a record is a header and a table of sections, and the kernels take that table as their
// argument.  Both are pure copies bound by HBM: one lane per destination unit, destination order, so every store is
// coalesced and a wave's loads run through one tile block (768 B of sums, 256 B of an AOV plane for the 8 x 8
// tile) before they jump to the next record.  Every section takes whole blocks of the grid, one after the other, so
// a block finds its section with a few scalar steps and its lanes share one path.  A section's unit is 16 bytes
// where every tile block of it starts on 16 bytes (rtw_parts_wide, aligned buffers and stride), else a dword; a
// stop map always goes as dwords, beside 16-byte sections of the same launch.  rtw_device.hip owns the
// accumulators and calls the two launchers; its own kernels compile as before.
#include <algorithm>
#include <cstdlib>
#include <string>

#include <hip/hip_runtime.h>

#include "rtw_common.h"
#include "../../include/rtw_aov_parts.h"
#include "../../include/rtw_clamp.h"

#define RTW_PARTS_BLOCK 256

namespace {
struct Section {
    uint32_t* data;   // the accumulator's array: a pack's source, a merge's destination
    uint64_t own;     // units of it
    uint64_t rec;     // units of the section in a record (part 0's)
    uint64_t at;      // the section's first unit in a record
    uint32_t per;     // units of one tile
    uint32_t wide;    // the unit: 16 bytes (1) or a dword (0)
    uint32_t blocks;  // blocks of the grid that cover the section
};

struct Args {
    Section sec[RTW_PARTS_MAX_SECTIONS];
    uint32_t sections;
    uint32_t part_count;
    uint64_t stride_words;  // between the gathered records (a merge's)
    uint32_t header[RTW_PARTS_HEADER_WORDS];  // (a pack's)
};

// the section of this block and the block's first unit in it; false past the last section
__device__ __forceinline__ bool parts_section(const Args& A, uint32_t* s, uint64_t* first) {
    uint32_t b = blockIdx.x, i = 0;
    while (i < A.sections && b >= A.sec[i].blocks) b -= A.sec[i++].blocks;
    *s = i;
    *first = (uint64_t)b * RTW_PARTS_BLOCK;
    return i < A.sections;
}

// The record's sections in record order; a unit past the partition's own tiles is zero.
__global__ __launch_bounds__(RTW_PARTS_BLOCK) void parts_pack_kernel(Args A, uint32_t* __restrict__ rec) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int h = 0; h < RTW_PARTS_HEADER_WORDS; ++h) rec[h] = A.header[h];
    }
    uint32_t s;
    uint64_t j;
    if (!parts_section(A, &s, &j)) return;
    const Section& S = A.sec[s];
    j += threadIdx.x;
    if (j >= S.rec) return;
    if (S.wide)
        ((uint4*)rec)[S.at + j] = j < S.own ? ((const uint4*)S.data)[j] : make_uint4(0u, 0u, 0u, 0u);
    else
        rec[S.at + j] = j < S.own ? S.data[j] : 0u;
}

// The whole's arrays one after the other; each unit comes from rtw_parts_source's place in the gathered buffer.
__global__ __launch_bounds__(RTW_PARTS_BLOCK) void parts_merge_kernel(Args A, const uint32_t* __restrict__ gathered) {
    uint32_t s;
    uint64_t j;
    if (!parts_section(A, &s, &j)) return;
    const Section& S = A.sec[s];
    j += threadIdx.x;
    if (j >= S.own) return;
    if (S.wide)
        ((uint4*)S.data)[j] = ((const uint4*)gathered)[rtw_parts_source(j, S.per, A.part_count, A.stride_words / 4, S.at)];
    else
        S.data[j] = gathered[rtw_parts_source(j, S.per, A.part_count, A.stride_words, S.at)];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The table of a launch: section s between the accumulator's arrays[s], `own_tiles` tiles long, and the records.
// The 16-byte path: every section that can take it does, or none (RTW_PARTS_DWORD=1 forces the dword path, for
// A/B measurements).  Returns the blocks of the grid.
uint32_t parts_args(const rtw_parts_layout& L, uint32_t own_tiles, const void* const* arrays, bool buffer_wide, bool pack, Args* A) {
    const char* e = std::getenv("RTW_PARTS_DWORD");
    bool wide = buffer_wide && !(e && std::atoi(e) != 0);
    for (int32_t s = 0; s < L.sections; ++s) wide = wide && (!rtw_parts_wide(&L, s) || aligned16(arrays[s]));
    uint64_t blocks = 0;
    A->sections = (uint32_t)L.sections;
    A->part_count = (uint32_t)L.part_count;
    for (int32_t s = 0; s < L.sections; ++s) {
        Section& S = A->sec[s];
        const uint64_t v = wide && rtw_parts_wide(&L, s) ? 4 : 1;
        S.data = (uint32_t*)arrays[s];
        S.own = (uint64_t)own_tiles * L.per[s] / v;
        S.rec = (uint64_t)L.tiles0 * L.per[s] / v;
        S.at = L.at[s] / v;
        S.per = (uint32_t)(L.per[s] / v);
        S.wide = v == 4;
        S.blocks = (uint32_t)(((pack ? S.rec : S.own) + RTW_PARTS_BLOCK - 1) / RTW_PARTS_BLOCK);
        blocks += S.blocks;
    }
    return (uint32_t)blocks;
}
}  // namespace

namespace rtw {

// what rtw_parts_merge (or the device path's reading of the headers) refused, by field name, of a colour record
// (tag 0) or an AOV record
int parts_refuse(uint32_t tag, const char* field, const int32_t at[2]) {
    const bool aov = tag != 0u;
    const std::string f = field ? field : "?";
    const std::string rec = "record " + std::to_string(at[0]);
    if (f == "params")
        return fail(RTW_ERR_INVALID_ARGUMENT, aov ? "params: an AOV merge needs a frame's geometry in 8 x 8 tiles, known channels and part_count >= 1"
                                                  : "params: a merge needs a frame's geometry, known flags and part_count >= 1");
    if (f == "stride_bytes")
        return fail(RTW_ERR_INVALID_ARGUMENT,
                    std::string("stride_bytes must be a multiple of 4 and at least ") + (aov ? "rtw_aov_packed_bytes" : "rtw_accum_packed_bytes"));
    if (f == "samples")
        return fail(RTW_ERR_INVALID_ARGUMENT, rec + " does not match the others: samples differs" + (aov ? "" : " (only adaptive parts may differ)"));
    if (f == "tile_stop")
        return fail(RTW_ERR_INVALID_ARGUMENT,
                    rec + ": tile_stop[" + std::to_string(at[1]) + "] is 1 or above the record's samples: a stop is 0 or within 2 .. samples");
    if (f == "magic")
        return fail(RTW_ERR_INVALID_ARGUMENT, rec + " is not an AOV record: magic differs (a colour accumulator's record holds 0 there)");
    return fail(RTW_ERR_INVALID_ARGUMENT, rec + " does not match the " + (aov ? "AOV " : "") + "accumulator: " + f + " differs");
}

hipError_t parts_pack_launch(const rtw_parts_layout& L, int32_t r, uint32_t samples, const void* const* arrays, void* d_packed,
                             hipStream_t stream) {
    const uint32_t own_tiles = (uint32_t)rtw_parts_tiles(&L, r);
    Args A{};
    // (at least one block: the header's)
    const uint32_t blocks = std::max(1u, parts_args(L, own_tiles, arrays, aligned16(d_packed), true, &A));
    const uint32_t header[RTW_PARTS_HEADER_WORDS] = {RTW_PARTS_VERSION, L.kind, (uint32_t)r, (uint32_t)L.part_count,
                                                     samples, own_tiles * (uint32_t)L.per_tile, own_tiles, rtw_parts_last_word(&L)};
    for (int h = 0; h < RTW_PARTS_HEADER_WORDS; ++h) A.header[h] = header[h];
    hipLaunchKernelGGL(parts_pack_kernel, dim3(blocks), dim3(RTW_PARTS_BLOCK), 0, stream, A, (uint32_t*)d_packed);
    return hipGetLastError();
}

hipError_t parts_merge_launch(const rtw_parts_layout& L, const void* d_gathered, uint64_t stride_bytes, void* const* arrays,
                              hipStream_t stream) {
    Args A{};
    const uint32_t blocks = parts_args(L, (uint32_t)L.n_tiles, arrays, aligned16(d_gathered) && (L.part_count == 1 || stride_bytes % 16 == 0),
                                       false, &A);
    A.stride_words = stride_bytes / 4;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(parts_merge_kernel, dim3(blocks), dim3(RTW_PARTS_BLOCK), 0, stream, A, (const uint32_t*)d_gathered);
    return hipGetLastError();
}

}  // namespace rtw

namespace {
// One of a host entry point's arrays, listed in the order the entry point checks them: given exactly when the kind
// word holds `bit` (0: always); the `rank`-th of the record, `planes` sections, the whole's slots apart.
struct HostArray {
    uint32_t bit;
    void* p;
    const char* name;
    int rank, planes;
};

int packed_bytes(int built, const rtw_parts_layout& L, const char* refusal, int64_t* bytes) {
    if (built != 0) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, refusal);
    *bytes = (int64_t)(L.words * 4);
    return RTW_OK;
}

// the two host twins: `built` is the layout builder's result, `want` the entry point's arrays, `when` the end of the
// message about an array that does not go with the kind word
template <size_t K>
int merge_host(int built, const rtw_parts_layout& L, uint32_t tag, uint32_t kind, const char* when, const HostArray (&want)[K],
               const void* gathered, int64_t stride_bytes, uint32_t* samples) {
    const int32_t none[2] = {0, 0};
    for (const auto& w : want)
        if (w.bit != 0 && ((kind & w.bit) != 0) != (w.p != nullptr))
            return rtw::fail(RTW_ERR_INVALID_ARGUMENT, std::string(w.name) + " is given exactly when the " + when);
    if (stride_bytes < 0 || stride_bytes % 4 != 0) return rtw::parts_refuse(tag, "stride_bytes", none);
    if (built != 0) return rtw::parts_refuse(tag, "params", none);
    uint32_t* dst[RTW_PARTS_MAX_SECTIONS];
    int n = 0;
    for (int rank = 0; rank < (int)K; ++rank)
        for (const auto& w : want)
            for (int k = 0; w.rank == rank && w.p && k < w.planes; ++k)
                dst[n++] = (uint32_t*)w.p + (size_t)k * (size_t)L.n_tiles * (size_t)L.per_tile;
    const char* field = nullptr;
    int32_t at[2];
    if (rtw_parts_merge(&L, (const uint32_t*)gathered, (uint64_t)stride_bytes / 4, dst, samples, &field, at) == 0) return RTW_OK;
    return rtw::parts_refuse(tag, field, at);
}
}  // namespace

extern "C" RTW_API int rtw_aov_packed_bytes(const rtw_render_params* params, uint32_t channels, int32_t part_count,
                                            int64_t* bytes) {
    if (!params || !bytes) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    rtw_parts_layout L;
    return packed_bytes(rtw_aov_parts_layout_of(params, channels, part_count, &L), L,
                        "a packed AOV record needs a frame's geometry in 8 x 8 tiles, known channels and part_count >= 1", bytes);
}

extern "C" RTW_API int rtw_aov_merge_parts_host(const rtw_render_params* params, uint32_t channels, const void* gathered,
                                                int64_t stride_bytes, int32_t part_count, float* albedo, float* normal,
                                                float* depth, uint32_t* hits, uint32_t* samples) {
    if (!params || !gathered || !hits || !samples) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    const HostArray want[4] = {{RTW_AOV_ALBEDO, albedo, "albedo", 0, 3}, {RTW_AOV_NORMAL, normal, "normal", 1, 3},
                               {RTW_AOV_DEPTH, depth, "depth", 2, 1}, {0u, hits, "hits", 3, 1}};
    rtw_parts_layout L;
    return merge_host(rtw_aov_parts_layout_of(params, channels, part_count, &L), L, RTW_AOV_PARTS_MAGIC, channels, "channels hold it", want,
                      gathered, stride_bytes, samples);
}

extern "C" RTW_API int rtw_accum_packed_bytes(const rtw_render_params* params, uint32_t flags, int32_t part_count,
                                              int64_t* bytes) {
    if (!params || !bytes) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    rtw_parts_layout L;
    return packed_bytes(rtw_parts_layout_of(params, flags, part_count, &L), L,
                        "a packed record needs a frame's geometry, known flags and part_count >= 1", bytes);
}

extern "C" RTW_API int rtw_accum_merge_parts_host(const rtw_render_params* params, uint32_t flags, const void* gathered,
                                                  int64_t stride_bytes, int32_t part_count, float* sums, float* squares,
                                                  uint32_t* kept, uint32_t* tile_stop, uint32_t* samples) {
    if (!params || !gathered || !sums || !samples) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & RTW_ACCUM_CLAMP)
        return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "rtw_accum_merge_parts_host: the flags hold RTW_ACCUM_CLAMP, whose records carry a level, "
                                                   "clamped and lost: use rtw_accum_merge_parts_host_clamp");
    const HostArray want[4] = {{0u, sums, "sums", 0, 1}, {RTW_ACCUM_MOMENTS, squares, "squares", 1, 1},
                               {RTW_ACCUM_ADAPTIVE, tile_stop, "tile_stop", 3, 1}, {RTW_ACCUM_FINITE, kept, "kept", 2, 1}};
    rtw_parts_layout L;
    return merge_host(rtw_parts_layout_of(params, flags, part_count, &L), L, 0u, flags, "flags call for it", want, gathered, stride_bytes,
                      samples);
}

extern "C" RTW_API int rtw_accum_merge_parts_host_clamp(const rtw_render_params* params, uint32_t flags, float level,
                                                        const void* gathered, int64_t stride_bytes, int32_t part_count,
                                                        float* sums, float* squares, uint32_t* kept, uint32_t* clamped,
                                                        float* lost, uint32_t* tile_stop, uint32_t* samples) {
    if (!params || !gathered || !sums || !samples) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    if (!(flags & RTW_ACCUM_CLAMP)) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "rtw_accum_merge_parts_host_clamp needs flags with RTW_ACCUM_CLAMP");
    if (!rtw_clamp_level_ok(level)) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "clamp: the level must be a finite f32 above 0");
    const HostArray want[6] = {{0u, sums, "sums", 0, 1},
                               {RTW_ACCUM_MOMENTS, squares, "squares", 1, 1},
                               {RTW_ACCUM_ADAPTIVE, tile_stop, "tile_stop", 5, 1},
                               {RTW_ACCUM_FINITE, kept, "kept", 2, 1},
                               {RTW_ACCUM_CLAMP, clamped, "clamped", 3, 1},
                               {RTW_ACCUM_CLAMP, lost, "lost", 4, 1}};
    rtw_parts_layout L;
    const int built = rtw_parts_layout_of(params, flags, part_count, &L);
    if (built == 0) rtw_parts_set_level(&L, level);
    return merge_host(built, L, 0u, flags, "flags call for it", want, gathered, stride_bytes, samples);
}
