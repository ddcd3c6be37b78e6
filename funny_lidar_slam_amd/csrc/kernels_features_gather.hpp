// kernels_features_gather.hpp -- the feature clouds of the LOAM front-end assembled on the device (include/fls_features_device.h): the
// per-ring selection lists feat_select_kernel leaves (corner: [rows][120], planar: [rows][cols + 6], with their counts) become
// corner_cloud_ and planar_cloud_ in the reference's order -- ring by ring, list order within a ring (feature_extractor.cpp:158-160,
// :220) -- as x | y | z | intensity planes, beside the compacted ordered-cloud indices.
//
// One workgroup per ring.  A ring's place in the clouds is the sum of the counts of the rings before it: there are `rows` counts (16 to
// 128), so every workgroup adds them up itself (one wave reduction) and no scan launch stands between the selection and the gather.  The
// last ring's workgroup also writes the two totals, the only words the host reads.  Per point: one 4-byte index load, one 16-byte load
// of the ordered row (the rows of a ring are neighbours in the ordered cloud, so the gather walks a few cache lines forwards), five
// coalesced 4-byte stores.  No LDS tile, no reuse: the kernel moves 40 bytes per feature point.
#pragma once
#include <hip/hip_runtime.h>

namespace fls {

constexpr int kFeatGatherThreads = 256;
constexpr int kFeatCornerStride = 120;  // feat_select_kernel: at most 20 corners per sector, six sectors per ring

// one class's lists and the planes they are gathered into (capacity `cap` points per plane = rows * stride: every list full)
struct FeatGatherSide {
    const int* idx;   // [rows][stride]
    const int* cnt;   // [rows]
    int stride;
    float *x, *y, *z, *in;  // planes
    int* idx_out;           // the ordered-cloud index of every gathered point
};

// sum of v over the workgroup's threads (kFeatGatherThreads = 4 waves); every thread gets the result
__device__ __forceinline__ int feat_gather_block_sum(int v, int* smem /* [4] */) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) smem[wave] = v;
    __syncthreads();
    const int s = smem[0] + smem[1] + smem[2] + smem[3];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(kFeatGatherThreads)
feat_gather_kernel(const int* __restrict__ n_ordered, const float4* __restrict__ ordered, const int rows, const FeatGatherSide corner,
                   const FeatGatherSide planar, int* __restrict__ totals /* [2]: corner, planar */) {
    __shared__ int smem[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int N = *n_ordered;
    const FeatGatherSide side[2] = {corner, planar};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const FeatGatherSide& S = side[c];
        int before = 0;
        for (int r = tid; r < row; r += kFeatGatherThreads) before += min(max(S.cnt[r], 0), S.stride);
        const int off = feat_gather_block_sum(before, smem);
        const int cnt = min(max(S.cnt[row], 0), S.stride);  // (never beyond the list: the planes hold rows * stride points)
        if (row == rows - 1 && tid == 0) totals[c] = off + cnt;
        const int* list = S.idx + (size_t)row * S.stride;
        for (int k = tid; k < cnt; k += kFeatGatherThreads) {
            const int i = list[k];
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((unsigned)i < (unsigned)N) p = ordered[i];  // (a selection indexes the ordered cloud; anything else reads nothing)
            S.x[off + k] = p.x;
            S.y[off + k] = p.y;
            S.z[off + k] = p.z;
            S.in[off + k] = p.w;
            S.idx_out[off + k] = i;
        }
    }
}

}  // namespace fls
