// rtw_common.h -- shared host-side helpers of librtw.so (error reporting).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/rtw.h"
#include "../../include/rtw_scalar.h"

// The scene RNG handle (TRng = Xoroshiro128PlusPlus, common.rs:1).
struct rtw_rng {
    rtw_xoro s;
};

struct rtw_parts_layout;  // include/rtw_parts.h

namespace rtw {

// Thread-local last error (returned by rtw_last_error()).
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
const char* last_error();

// Descending key sort carrying values (hipcub radix sort, rtw_sort.hip).  With tmp == nullptr
// only sets *tmp_bytes.
hipError_t sort_pairs_desc(const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                           int n, void* tmp, size_t* tmp_bytes, hipStream_t stream);

// The render kernel's surface-area-heuristic tree over n leaf boxes (lo/hi: 3 floats per leaf),
// children encoded as in rtw_bvh_node (>= 0 node, < 0 leaf -1 - index).  *depth = nodes on the
// longest root-to-leaf path (rtw_sah.cpp).
int sah_build(const float* lo, const float* hi, int32_t n, std::vector<rtw_bvh_node>& nodes, int32_t* root, int* depth);
// The same with spatial splits (rtw_sah.cpp): tri = 9 floats per leaf (vertices; x = NaN: not a
// triangle, cut as a box), leaf_km = {k, m} per leaf (k < 0: never hits), at most budget x n extra
// references.  Node boxes are the unions of the references' clipped boxes below (rounded outward);
// km = 2 floats per node, the maxima of the leaf constants below.
int sah_build_split(const float* lo, const float* hi, const float* tri, const float* leaf_km, int32_t n, double budget,
                    std::vector<rtw_bvh_node>& nodes, std::vector<float>& km, int32_t* root, int* depth,
                    int depth_cap = 0);

// The pack and merge launches of rtw_accum_pack / rtw_accum_merge_parts and rtw_aov_pack / rtw_aov_merge_parts
// (rtw_parts.hip; the layout is include/rtw_parts.h's).  arrays[s]: the accumulator's device array of the
// layout's section s.  The callers have validated the sizes: the launches only choose the 16-byte or the dword path.
hipError_t parts_pack_launch(const rtw_parts_layout& L, int32_t part_index, uint32_t samples, const void* const* arrays,
                             void* d_packed, hipStream_t stream);
hipError_t parts_merge_launch(const rtw_parts_layout& L, const void* d_gathered, uint64_t stride_bytes, void* const* arrays,
                              hipStream_t stream);
// fail() with the message of a refused merge of colour (tag 0) or AOV records (the layout's tag): the field's name,
// the record (at[0]) and, for a stop, the local tile (at[1])
int parts_refuse(uint32_t tag, const char* field, const int32_t at[2]);

}  // namespace rtw
