// lane_group.hpp -- what G = 4 or 8 neighbouring lanes that cooperate on one query share: DPP butterflies (min / sum over the
// group, no LDS) and the candidate index -> map slot select chain.  Used by the iVox kNN kernel (kernels_ivox_coop.hpp, G = 4)
// and by the cell-grid kNN kernels (kernels_grid_coop.hpp, G = 8).
#pragma once
#include <hip/hip_runtime.h>

namespace fls {

// Butterfly exchange partners without LDS: lane^1 and lane^2 are quad permutes, the third pairing uses
// row_half_mirror (lane i <-> 7-i inside each group of 8) -- any perfect pairing works for a min / sum.
template <int STEP>
__device__ __forceinline__ unsigned dpp_pair_u32(const unsigned v) {
    static_assert(STEP >= 0 && STEP <= 2, "");
    if (STEP == 0) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);  // quad_perm [1,0,3,2]
    if (STEP == 1) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);  // quad_perm [2,3,0,1]
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);                // row_half_mirror
}
template <int STEP>
__device__ __forceinline__ unsigned long long dpp_pair_u64(const unsigned long long v) {
    const unsigned lo = dpp_pair_u32<STEP>((unsigned)(v & 0xffffffffull));
    const unsigned hi = dpp_pair_u32<STEP>((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
template <int G>
__device__ __forceinline__ unsigned long long group_min_u64(unsigned long long v) {
    static_assert(G == 4 || G == 8, "group size");
    unsigned long long o = dpp_pair_u64<0>(v); v = o < v ? o : v;
    o = dpp_pair_u64<1>(v); v = o < v ? o : v;
    if (G == 8) { o = dpp_pair_u64<2>(v); v = o < v ? o : v; }
    return v;
}
template <int G>
__device__ __forceinline__ unsigned group_min_u32(unsigned v) {
    static_assert(G == 4 || G == 8, "group size");
    unsigned o = dpp_pair_u32<0>(v); v = o < v ? o : v;
    o = dpp_pair_u32<1>(v); v = o < v ? o : v;
    if (G == 8) { o = dpp_pair_u32<2>(v); v = o < v ? o : v; }
    return v;
}
template <int G>
__device__ __forceinline__ int group_sum_i32(int v) {
    static_assert(G == 4 || G == 8, "group size");
    v += (int)dpp_pair_u32<0>((unsigned)v);
    v += (int)dpp_pair_u32<1>((unsigned)v);
    if (G == 8) v += (int)dpp_pair_u32<2>((unsigned)v);
    return v;
}

// candidate index -> map slot as a compare / select chain on VALUES (written as a function of scalars: a lambda
// capturing the offsets by reference made the compiler select between ADDRESSES and load through them):
// slot = idx + (begin - prefix) of the voxel the index falls in, voxel r covering [p_r, p_{r+1}) with offset o_r
template <int R>
__device__ __forceinline__ unsigned slot_select(const unsigned idx, const unsigned p1, const unsigned p2, const unsigned p3, const unsigned p4,
                                                const unsigned o0, const unsigned o1, const unsigned o2, const unsigned o3, const unsigned o4) {
    unsigned sel = R == 5 ? o4 : R == 4 ? o3 : R == 3 ? o2 : R == 2 ? o1 : o0;
    if (R > 4) sel = idx < p4 ? o3 : sel;
    if (R > 3) sel = idx < p3 ? o2 : sel;
    if (R > 2) sel = idx < p2 ? o1 : sel;
    if (R > 1) sel = idx < p1 ? o0 : sel;
    return idx + sel;
}

}  // namespace fls
