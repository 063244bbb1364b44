// rtw_parts.hip -- packing one partition's accumulator state into a record and placing N gathered records
// into the whole image's accumulator (rtw_accum_pack, rtw_accum_merge_parts of rtw.h).
//
// The layout and the placement are include/rtw_parts.h's, one text for the kernels here, the host twin and a
// numpy restatement.  Both kernels are pure copies bound by HBM: one lane per destination unit, destination
// order, so every store is coalesced and a wave's loads run through one tile block (768 B of sums for the 8 x 8
// tile) before they jump to the next record.  T is uint4 where every tile block and section starts on 16 bytes
// (rtw_parts_wide, an aligned buffer and stride), else uint32_t.  The stop map and the header are a dword tail of
// the same launch.  rtw_device.hip owns struct rtw_accum and calls the two launchers; its own kernels compile
// as before.
//
// The AOV records (rtw_aov_pack, rtw_aov_merge_parts; include/rtw_aov_parts.h) are the same two
// copies over planes: every plane is tile-major with 64 words per tile, so blockIdx.y is the plane and one lane
// handles one destination unit of it.  An accumulator's albedo, normal and depth planes are one allocation and
// its hits another; in a record all of them follow the header S0 words apart.
#include <algorithm>
#include <cstdlib>
#include <string>

#include <hip/hip_runtime.h>

#include "rtw_common.h"
#include "../../include/rtw_aov_parts.h"
#include "../../include/rtw_parts.h"

#define RTW_PARTS_BLOCK 256

namespace {
struct PackArgs {
    const uint32_t* sums;     // the accumulator's arrays (null: the flags do not call for it)
    const uint32_t* squares;
    const uint32_t* kept;
    const uint32_t* stop;
    uint64_t own3, own1;      // units the partition itself holds in a 3-word and in a 1-word section
    uint64_t sec3, sec1;      // units of such a section in the record (part 0's)
    uint64_t stop_word;       // the record's word where the stop section starts
    uint32_t own_tiles, tiles0;  // (tiles0 = 0 without a stop section)
    uint32_t header[RTW_PARTS_HEADER_WORDS];
};

template <class T>
__device__ __forceinline__ T parts_zero();
template <>
__device__ __forceinline__ uint32_t parts_zero<uint32_t>() {
    return 0u;
}
template <>
__device__ __forceinline__ uint4 parts_zero<uint4>() {
    return make_uint4(0u, 0u, 0u, 0u);
}

// The record's sections in record order; a unit past the partition's own slots is zero.
template <class T>
__global__ __launch_bounds__(RTW_PARTS_BLOCK) void parts_pack_kernel(PackArgs P, uint32_t* __restrict__ rec) {
    uint64_t j = (uint64_t)blockIdx.x * RTW_PARTS_BLOCK + threadIdx.x;
    T* __restrict__ bulk = (T*)(rec + RTW_PARTS_HEADER_WORDS);
    const uint64_t i = j;
    if (j < P.sec3) {
        bulk[i] = j < P.own3 ? ((const T*)P.sums)[j] : parts_zero<T>();
        return;
    }
    j -= P.sec3;
    if (P.squares) {
        if (j < P.sec3) {
            bulk[i] = j < P.own3 ? ((const T*)P.squares)[j] : parts_zero<T>();
            return;
        }
        j -= P.sec3;
    }
    if (P.kept) {
        if (j < P.sec1) {
            bulk[i] = j < P.own1 ? ((const T*)P.kept)[j] : parts_zero<T>();
            return;
        }
        j -= P.sec1;
    }
    if (j < P.tiles0) {
        rec[P.stop_word + j] = j < P.own_tiles ? P.stop[j] : 0u;
        return;
    }
    if (j == P.tiles0) {
#pragma unroll
        for (int h = 0; h < RTW_PARTS_HEADER_WORDS; ++h) rec[h] = P.header[h];
    }
}

struct MergeArgs {
    uint32_t* sums;  // the whole's arrays (null: the flags do not call for it)
    uint32_t* squares;
    uint32_t* kept;
    uint32_t* stop;
    uint64_t n3, n1;                           // units of the whole's sums (squares) and kept
    uint64_t stride, at_sums, at_squares, at_kept;  // in units
    uint64_t stride_words, at_stop;            // in words
    uint32_t per3, per1;                       // units of one tile
    uint32_t part_count, n_tiles;
};

// The whole's arrays one after the other; each unit comes from rtw_parts_source's place in the gathered buffer.
template <class T>
__global__ __launch_bounds__(RTW_PARTS_BLOCK) void parts_merge_kernel(MergeArgs M, const uint32_t* __restrict__ gathered) {
    uint64_t j = (uint64_t)blockIdx.x * RTW_PARTS_BLOCK + threadIdx.x;
    const T* __restrict__ src = (const T*)gathered;
    if (j < M.n3) {
        ((T*)M.sums)[j] = src[rtw_parts_source(j, M.per3, M.part_count, M.stride, M.at_sums)];
        return;
    }
    j -= M.n3;
    if (M.squares) {
        if (j < M.n3) {
            ((T*)M.squares)[j] = src[rtw_parts_source(j, M.per3, M.part_count, M.stride, M.at_squares)];
            return;
        }
        j -= M.n3;
    }
    if (M.kept) {
        if (j < M.n1) {
            ((T*)M.kept)[j] = src[rtw_parts_source(j, M.per1, M.part_count, M.stride, M.at_kept)];
            return;
        }
        j -= M.n1;
    }
    if (M.stop && j < M.n_tiles) M.stop[j] = gathered[rtw_parts_source(j, 1u, M.part_count, M.stride_words, M.at_stop)];
}

struct AovPackArgs {
    const uint32_t* planes;  // the accumulator's value planes, `own` units apart (null: the part holds no tiles)
    const uint32_t* hits;
    uint32_t value_planes;   // planes before hits
    uint32_t own, sec;       // units of a plane the part itself holds, and of a plane in the record (part 0's)
    uint32_t header[RTW_PARTS_HEADER_WORDS];
};

// grid.y: the record's planes in record order; a unit past the part's own slots is zero.
template <class T>
__global__ __launch_bounds__(RTW_PARTS_BLOCK) void aov_parts_pack_kernel(AovPackArgs P, uint32_t* __restrict__ rec) {
    const uint32_t j = blockIdx.x * RTW_PARTS_BLOCK + threadIdx.x, plane = blockIdx.y;
    if (j == 0 && plane == 0) {
#pragma unroll
        for (int h = 0; h < RTW_PARTS_HEADER_WORDS; ++h) rec[h] = P.header[h];
    }
    if (j >= P.sec) return;
    const T* __restrict__ src = (const T*)(plane < P.value_planes ? P.planes : P.hits) + (plane < P.value_planes ? (size_t)plane * P.own : 0);
    T* __restrict__ bulk = (T*)(rec + RTW_PARTS_HEADER_WORDS);
    bulk[(size_t)plane * P.sec + j] = j < P.own ? src[j] : parts_zero<T>();
}

struct AovMergeArgs {
    uint32_t* planes;  // the whole's value planes, `n` units apart
    uint32_t* hits;
    uint32_t value_planes;
    uint32_t n;               // units of one of the whole's planes
    uint32_t sec;             // units of a plane in a record
    uint32_t part_count;
    uint64_t stride, header;  // in units
};

// grid.y: the plane; each unit of the whole's plane comes from rtw_aov_parts_source's place in the gathered buffer.
// PER: units of one tile (64 words, or 16 uint4).
template <class T, uint32_t PER>
__global__ __launch_bounds__(RTW_PARTS_BLOCK) void aov_parts_merge_kernel(AovMergeArgs M, const uint32_t* __restrict__ gathered) {
    const uint32_t j = blockIdx.x * RTW_PARTS_BLOCK + threadIdx.x, plane = blockIdx.y;
    if (j >= M.n) return;
    T* __restrict__ dst = (T*)(plane < M.value_planes ? M.planes : M.hits) + (plane < M.value_planes ? (size_t)plane * M.n : 0);
    dst[j] = ((const T*)gathered)[rtw_aov_parts_source(j, plane, PER, M.part_count, M.stride, M.header, M.sec)];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
// RTW_PARTS_DWORD=1 forces the dword path (A/B measurements)
bool force_dword() {
    const char* e = std::getenv("RTW_PARTS_DWORD");
    return e && std::atoi(e) != 0;
}
}  // namespace

namespace rtw {

// what rtw_parts_merge (or the device path's own reading of the headers) refused, by field name
int parts_refuse(const char* field, const int32_t at[2]) {
    const std::string f = field ? field : "?";
    const std::string rec = "record " + std::to_string(at[0]);
    if (f == "params") return fail(RTW_ERR_INVALID_ARGUMENT, "params: a merge needs a frame's geometry, known flags and part_count >= 1");
    if (f == "stride_bytes")
        return fail(RTW_ERR_INVALID_ARGUMENT, "stride_bytes must be a multiple of 4 and at least rtw_accum_packed_bytes");
    if (f == "samples")
        return fail(RTW_ERR_INVALID_ARGUMENT, rec + " does not match the others: samples differs (only adaptive parts may differ)");
    if (f == "tile_stop")
        return fail(RTW_ERR_INVALID_ARGUMENT,
                    rec + ": tile_stop[" + std::to_string(at[1]) + "] is 1 or above the record's samples: a stop is 0 or within 2 .. samples");
    return fail(RTW_ERR_INVALID_ARGUMENT, rec + " does not match the accumulator: " + f + " differs");
}

hipError_t parts_pack_launch(const rtw_parts_layout& L, int32_t r, uint32_t samples, const float* sums, const float* squares,
                             const uint32_t* kept, const uint32_t* stop, void* d_packed, hipStream_t stream) {
    const uint32_t own_tiles = (uint32_t)rtw_parts_tiles(&L, r);
    const uint64_t own_slots = (uint64_t)own_tiles * (uint64_t)L.per_tile;
    const bool wide = rtw_parts_wide(&L) && aligned16(d_packed) && aligned16(sums) && aligned16(squares) && aligned16(kept) &&
                      !force_dword();
    const uint64_t v = wide ? 4 : 1;
    PackArgs P{};
    P.sums = (const uint32_t*)sums;
    P.squares = (const uint32_t*)squares;
    P.kept = kept;
    P.stop = stop;
    P.own3 = 3 * own_slots / v;
    P.own1 = own_slots / v;
    P.sec3 = 3 * (uint64_t)L.slots0 / v;
    P.sec1 = (uint64_t)L.slots0 / v;
    P.stop_word = L.stop;
    P.own_tiles = own_tiles;
    P.tiles0 = stop ? (uint32_t)L.tiles0 : 0u;
    const uint32_t header[RTW_PARTS_HEADER_WORDS] = {RTW_PARTS_VERSION, L.flags, (uint32_t)r, (uint32_t)L.part_count,
                                                     samples, (uint32_t)own_slots, own_tiles, 0u};
    for (int h = 0; h < RTW_PARTS_HEADER_WORDS; ++h) P.header[h] = header[h];
    const uint64_t lanes = P.sec3 * (squares ? 2 : 1) + (kept ? P.sec1 : 0) + P.tiles0 + 1;
    const dim3 grid((unsigned)((lanes + RTW_PARTS_BLOCK - 1) / RTW_PARTS_BLOCK));
    if (wide)
        hipLaunchKernelGGL(parts_pack_kernel<uint4>, grid, dim3(RTW_PARTS_BLOCK), 0, stream, P, (uint32_t*)d_packed);
    else
        hipLaunchKernelGGL(parts_pack_kernel<uint32_t>, grid, dim3(RTW_PARTS_BLOCK), 0, stream, P, (uint32_t*)d_packed);
    return hipGetLastError();
}

hipError_t parts_merge_launch(const rtw_parts_layout& L, const void* d_gathered, uint64_t stride_bytes, float* sums,
                              float* squares, uint32_t* kept, uint32_t* stop, hipStream_t stream) {
    const uint64_t slots = (uint64_t)L.n_tiles * (uint64_t)L.per_tile;
    const bool wide = rtw_parts_wide(&L) && aligned16(d_gathered) && (L.part_count == 1 || stride_bytes % 16 == 0) &&
                      aligned16(sums) && aligned16(squares) && aligned16(kept) && !force_dword();
    const uint64_t v = wide ? 4 : 1;
    MergeArgs M{};
    M.sums = (uint32_t*)sums;
    M.squares = (uint32_t*)squares;
    M.kept = kept;
    M.stop = stop;
    M.n3 = 3 * slots / v;
    M.n1 = slots / v;
    M.stride = stride_bytes / 4 / v;
    M.at_sums = L.sums / v;
    M.at_squares = L.squares / v;
    M.at_kept = L.kept / v;
    M.stride_words = stride_bytes / 4;
    M.at_stop = L.stop;
    M.per3 = (uint32_t)(3 * (uint64_t)L.per_tile / v);
    M.per1 = (uint32_t)((uint64_t)L.per_tile / v);
    M.part_count = (uint32_t)L.part_count;
    M.n_tiles = (uint32_t)L.n_tiles;
    const uint64_t lanes = M.n3 * (squares ? 2 : 1) + (kept ? M.n1 : 0) + (stop ? M.n_tiles : 0);
    if (lanes == 0) return hipSuccess;
    const dim3 grid((unsigned)((lanes + RTW_PARTS_BLOCK - 1) / RTW_PARTS_BLOCK));
    if (wide)
        hipLaunchKernelGGL(parts_merge_kernel<uint4>, grid, dim3(RTW_PARTS_BLOCK), 0, stream, M, (const uint32_t*)d_gathered);
    else
        hipLaunchKernelGGL(parts_merge_kernel<uint32_t>, grid, dim3(RTW_PARTS_BLOCK), 0, stream, M, (const uint32_t*)d_gathered);
    return hipGetLastError();
}

// ---- AOV records ----
int aov_parts_refuse(const char* field, int32_t at) {
    const std::string f = field ? field : "?";
    const std::string rec = "record " + std::to_string(at);
    if (f == "params")
        return fail(RTW_ERR_INVALID_ARGUMENT, "params: an AOV merge needs a frame's geometry in 8 x 8 tiles, known channels and part_count >= 1");
    if (f == "stride_bytes")
        return fail(RTW_ERR_INVALID_ARGUMENT, "stride_bytes must be a multiple of 4 and at least rtw_aov_packed_bytes");
    if (f == "samples") return fail(RTW_ERR_INVALID_ARGUMENT, rec + " does not match the others: samples differs");
    if (f == "magic")
        return fail(RTW_ERR_INVALID_ARGUMENT, rec + " is not an AOV record: magic differs (a colour accumulator's record holds 0 there)");
    return fail(RTW_ERR_INVALID_ARGUMENT, rec + " does not match the AOV accumulator: " + f + " differs");
}

// planes: the part's value planes (own slots apart) or null; hits: its hit counts
hipError_t aov_parts_pack_launch(const rtw_aov_parts_layout& L, int32_t r, uint32_t samples, const float* planes,
                                 const uint32_t* hits, void* d_packed, hipStream_t stream) {
    const uint32_t own_tiles = (uint32_t)rtw_aov_parts_tiles(&L, r);
    const uint32_t own_slots = own_tiles * RTW_AOV_PARTS_PER_TILE;
    const bool wide = aligned16(d_packed) && aligned16(planes) && aligned16(hits) && !force_dword();
    const uint32_t v = wide ? 4 : 1;
    AovPackArgs P{};
    P.planes = (const uint32_t*)planes;
    P.hits = hits;
    P.value_planes = (uint32_t)L.planes - 1;
    P.own = own_slots / v;
    P.sec = L.slots0 / v;
    const uint32_t header[RTW_PARTS_HEADER_WORDS] = {RTW_AOV_PARTS_VERSION, L.channels, (uint32_t)r, (uint32_t)L.part_count,
                                                     samples, own_slots, own_tiles, RTW_AOV_PARTS_MAGIC};
    for (int h = 0; h < RTW_PARTS_HEADER_WORDS; ++h) P.header[h] = header[h];
    // (at least one block: the header's)
    const dim3 grid(std::max(1u, (P.sec + RTW_PARTS_BLOCK - 1) / RTW_PARTS_BLOCK), (unsigned)L.planes);
    if (wide)
        hipLaunchKernelGGL(aov_parts_pack_kernel<uint4>, grid, dim3(RTW_PARTS_BLOCK), 0, stream, P, (uint32_t*)d_packed);
    else
        hipLaunchKernelGGL(aov_parts_pack_kernel<uint32_t>, grid, dim3(RTW_PARTS_BLOCK), 0, stream, P, (uint32_t*)d_packed);
    return hipGetLastError();
}

hipError_t aov_parts_merge_launch(const rtw_aov_parts_layout& L, const void* d_gathered, uint64_t stride_bytes, float* planes,
                                  uint32_t* hits, hipStream_t stream) {
    const uint32_t slots = (uint32_t)L.n_tiles * RTW_AOV_PARTS_PER_TILE;
    const bool wide = aligned16(d_gathered) && (L.part_count == 1 || stride_bytes % 16 == 0) && aligned16(planes) &&
                      aligned16(hits) && !force_dword();
    const uint32_t v = wide ? 4 : 1;
    AovMergeArgs M{};
    M.planes = (uint32_t*)planes;
    M.hits = hits;
    M.value_planes = (uint32_t)L.planes - 1;
    M.n = slots / v;
    M.sec = L.slots0 / v;
    M.part_count = (uint32_t)L.part_count;
    M.stride = stride_bytes / 4 / v;
    M.header = RTW_PARTS_HEADER_WORDS / v;
    if (M.n == 0) return hipSuccess;
    const dim3 grid((M.n + RTW_PARTS_BLOCK - 1) / RTW_PARTS_BLOCK, (unsigned)L.planes);
    if (wide)
        hipLaunchKernelGGL((aov_parts_merge_kernel<uint4, RTW_AOV_PARTS_PER_TILE / 4>), grid, dim3(RTW_PARTS_BLOCK), 0, stream, M,
                           (const uint32_t*)d_gathered);
    else
        hipLaunchKernelGGL((aov_parts_merge_kernel<uint32_t, RTW_AOV_PARTS_PER_TILE>), grid, dim3(RTW_PARTS_BLOCK), 0, stream, M,
                           (const uint32_t*)d_gathered);
    return hipGetLastError();
}

}  // namespace rtw

extern "C" RTW_API int rtw_aov_packed_bytes(const rtw_render_params* params, uint32_t channels, int32_t part_count,
                                            int64_t* bytes) {
    if (!params || !bytes) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    rtw_aov_parts_layout L;
    if (rtw_aov_parts_layout_of(params, channels, part_count, &L) != 0)
        return rtw::fail(RTW_ERR_INVALID_ARGUMENT,
                         "a packed AOV record needs a frame's geometry in 8 x 8 tiles, known channels and part_count >= 1");
    *bytes = (int64_t)(L.words * 4);
    return RTW_OK;
}

extern "C" RTW_API int rtw_aov_merge_parts_host(const rtw_render_params* params, uint32_t channels, const void* gathered,
                                                int64_t stride_bytes, int32_t part_count, float* albedo, float* normal,
                                                float* depth, uint32_t* hits, uint32_t* samples) {
    if (!params || !gathered || !hits || !samples) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    const struct {
        uint32_t bit;
        const void* p;
        const char* name;
    } want[3] = {{RTW_AOV_ALBEDO, albedo, "albedo"}, {RTW_AOV_NORMAL, normal, "normal"}, {RTW_AOV_DEPTH, depth, "depth"}};
    for (const auto& w : want)
        if (((channels & w.bit) != 0) != (w.p != nullptr))
            return rtw::fail(RTW_ERR_INVALID_ARGUMENT, std::string(w.name) + " is given exactly when the channels hold it");
    if (stride_bytes < 0 || stride_bytes % 4 != 0) return rtw::aov_parts_refuse("stride_bytes", 0);
    const char* field = nullptr;
    int32_t at = 0;
    if (rtw_aov_parts_merge(params, channels, (const uint32_t*)gathered, (uint64_t)stride_bytes / 4, part_count, (uint32_t*)albedo,
                            (uint32_t*)normal, (uint32_t*)depth, hits, samples, &field, &at) == 0)
        return RTW_OK;
    return rtw::aov_parts_refuse(field, at);
}

extern "C" RTW_API int rtw_accum_packed_bytes(const rtw_render_params* params, uint32_t flags, int32_t part_count,
                                              int64_t* bytes) {
    if (!params || !bytes) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    rtw_parts_layout L;
    if (rtw_parts_layout_of(params, flags, part_count, &L) != 0)
        return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "a packed record needs a frame's geometry, known flags and part_count >= 1");
    *bytes = (int64_t)(L.words * 4);
    return RTW_OK;
}

extern "C" RTW_API int rtw_accum_merge_parts_host(const rtw_render_params* params, uint32_t flags, const void* gathered,
                                                  int64_t stride_bytes, int32_t part_count, float* sums, float* squares,
                                                  uint32_t* kept, uint32_t* tile_stop, uint32_t* samples) {
    if (!params || !gathered || !sums || !samples) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    const struct {
        uint32_t flag;
        const void* p;
        const char* name;
    } want[3] = {{RTW_ACCUM_MOMENTS, squares, "squares"}, {RTW_ACCUM_ADAPTIVE, tile_stop, "tile_stop"}, {RTW_ACCUM_FINITE, kept, "kept"}};
    for (const auto& w : want)
        if (((flags & w.flag) != 0) != (w.p != nullptr))
            return rtw::fail(RTW_ERR_INVALID_ARGUMENT, std::string(w.name) + " is given exactly when the flags call for it");
    if (stride_bytes < 0 || stride_bytes % 4 != 0)
        return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "stride_bytes must be a multiple of 4 and at least rtw_accum_packed_bytes");
    const char* field = nullptr;
    int32_t at[2] = {0, 0};
    if (rtw_parts_merge(params, flags, (const uint32_t*)gathered, (uint64_t)stride_bytes / 4, part_count, (uint32_t*)sums,
                        (uint32_t*)squares, kept, tile_stop, samples, &field, at) == 0)
        return RTW_OK;
    return rtw::parts_refuse(field, at);
}
