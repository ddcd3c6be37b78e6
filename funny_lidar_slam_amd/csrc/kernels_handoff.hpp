// kernels_handoff.hpp -- the scan hand-off from the preprocessing handle to a matcher (fls_scan_attach_preprocessed): the cloud the
// preprocessing left in device memory becomes the matcher's resident scan x[n] | y[n] | z[n] | intensity[n] without visiting the host.
// Both kernels are pure streaming copies (16 bytes read and written per point, no reuse, no LDS): one lane per point, every load and
// store of a wave is one contiguous run.
#pragma once
#include <hip/hip_runtime.h>

namespace fls {

constexpr int kHandoffThreads = 256;

// ordered cloud (float4 rows x y z intensity) -> the four planes of the matcher's raw resident scan: one coalesced 16-byte load and
// four coalesced 4-byte stores per lane
__global__ void __launch_bounds__(kHandoffThreads) handoff_rows_kernel(const float4* __restrict__ rows, const unsigned n, float* __restrict__ x,
                                                                       float* __restrict__ y, float* __restrict__ z, float* __restrict__ in) {
    const unsigned i = blockIdx.x * unsigned(kHandoffThreads) + threadIdx.x;
    if (i >= n) return;
    const float4 p = rows[i];
    x[i] = p.x;
    y[i] = p.y;
    z[i] = p.z;
    in[i] = p.w;
}

// planar cloud (x | y | z | intensity with the producer's row stride) or the VoxelGrid's output planes -> the matcher's planes (row
// stride n).  The planes start at arbitrary multiples of 4 bytes, so the copy stays at one float per lane and plane.
__global__ void __launch_bounds__(kHandoffThreads) handoff_planes_kernel(const float* __restrict__ sx, const float* __restrict__ sy,
                                                                         const float* __restrict__ sz, const float* __restrict__ si, const unsigned n,
                                                                         float* __restrict__ x, float* __restrict__ y, float* __restrict__ z,
                                                                         float* __restrict__ in) {
    const unsigned i = blockIdx.x * unsigned(kHandoffThreads) + threadIdx.x;
    if (i >= n) return;
    x[i] = sx[i];
    y[i] = sy[i];
    z[i] = sz[i];
    in[i] = si[i];
}

// where a cloud of the preprocessing handle lies on the device: rows (ordered) or four planes (planar, planar filtered)
struct HandoffCloud {
    const float4* rows = nullptr;
    const float *x = nullptr, *y = nullptr, *z = nullptr, *in = nullptr;
    size_t n = 0;
};

// dst = x | y | z | intensity, row stride c.n, on stream s
inline void handoff_launch(const HandoffCloud& c, float* dst, hipStream_t s) {
    if (c.n == 0) return;
    const unsigned n = unsigned(c.n);
    const dim3 grid((n + kHandoffThreads - 1) / kHandoffThreads);
    if (c.rows)
        hipLaunchKernelGGL(handoff_rows_kernel, grid, dim3(kHandoffThreads), 0, s, c.rows, n, dst, dst + c.n, dst + 2 * c.n, dst + 3 * c.n);
    else
        hipLaunchKernelGGL(handoff_planes_kernel, grid, dim3(kHandoffThreads), 0, s, c.x, c.y, c.z, c.in, n, dst, dst + c.n, dst + 2 * c.n, dst + 3 * c.n);
}

}  // namespace fls
