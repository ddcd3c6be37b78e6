// kernels_debug_linalg.hpp -- test hooks of include/fls_debug_linalg.h: every kernel calls ONE routine of linalg_dev.hpp / wave_solve.hpp,
// the __forceinline__ routine itself and the way the matcher kernels call it (same translation unit, same flags: -ffp-contract=off), on
// caller-supplied inputs.  tests/test_gpu_linalg.py compares the results with the CPU restatement of the same Eigen routines bit for bit.
#pragma once
#include "kernels_knn.hpp"

namespace fls {

constexpr int kDebugLinalgBlock = 64;

// plane_fit_5x3 as plane_residual_dev (kernels_p2plane.hpp) calls it: A[col][row] in registers, one lane per system
__global__ void __launch_bounds__(kDebugLinalgBlock)
debug_plane_fit_5x3_kernel(const double* __restrict__ A, const int n, double* __restrict__ x) {
    const int s = blockIdx.x * kDebugLinalgBlock + threadIdx.x;
    if (s >= n) return;
    double a[3][5], r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 5; ++j) a[c][j] = A[(size_t)s * 15 + c * 5 + j];
    plane_fit_5x3(a, r);
#pragma unroll
    for (int c = 0; c < 3; ++c) x[(size_t)s * 3 + c] = r[c];
}

// jacobi_svd3_v as line_residual_dev (kernels_knn.hpp) calls it: C[col][row] in registers, one lane per system
__global__ void __launch_bounds__(kDebugLinalgBlock)
debug_svd3_kernel(const double* __restrict__ A, const int n, double* __restrict__ S, double* __restrict__ V) {
    const int s = blockIdx.x * kDebugLinalgBlock + threadIdx.x;
    if (s >= n) return;
    double a[3][3], sv[3], v[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) a[c][r] = A[(size_t)s * 9 + c * 3 + r];
    jacobi_svd3_v(a, sv, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        S[(size_t)s * 3 + c] = sv[c];
#pragma unroll
        for (int r = 0; r < 3; ++r) V[(size_t)s * 9 + c * 3 + r] = v[c][r];
    }
}

// lu6_solve_wave as lu_tail (kernels_knn.hpp) calls it: one wave per system, the tail's own LDS struct
__global__ void __launch_bounds__(64)
debug_lu6_kernel(const double* __restrict__ H, const double* __restrict__ b, const int n, double* __restrict__ det, double* __restrict__ inv,
                 double* __restrict__ x) {
    const int s = blockIdx.x;
    if (s >= n) return;
    __shared__ LuTailSmem sm;
    if (threadIdx.x < 36) sm.Hs[threadIdx.x] = H[(size_t)s * 36 + threadIdx.x];
    if (threadIdx.x < 6) sm.gs[threadIdx.x] = b[(size_t)s * 6 + threadIdx.x];
    __builtin_amdgcn_wave_barrier();
    const double d = lu6_solve_wave(sm.Hs, sm.inv, sm.gs, sm.xs, sm.tr);
    if (threadIdx.x < 36) inv[(size_t)s * 36 + threadIdx.x] = sm.inv[threadIdx.x];
    if (threadIdx.x < 6) x[(size_t)s * 6 + threadIdx.x] = sm.xs[threadIdx.x];
    if (threadIdx.x == 0) det[s] = d;
}

// so3_exp_dev, then mat3_mul_dev in the order of lu_tail (R * Rd) and in the order of loam_tail (Rd * R); one lane per system
__global__ void __launch_bounds__(kDebugLinalgBlock)
debug_so3_kernel(const double* __restrict__ v, const double* __restrict__ R, const int n, double* __restrict__ Rd, double* __restrict__ R_Rd,
                 double* __restrict__ Rd_R) {
    const int s = blockIdx.x * kDebugLinalgBlock + threadIdx.x;
    if (s >= n) return;
    double dx[3], rd[9], r[9], right[9], left[9];
    for (int q = 0; q < 3; ++q) dx[q] = v[(size_t)s * 3 + q];
    for (int q = 0; q < 9; ++q) r[q] = R[(size_t)s * 9 + q];
    so3_exp_dev(dx, rd);
    mat3_mul_dev(r, rd, right);
    mat3_mul_dev(rd, r, left);
    for (int q = 0; q < 9; ++q) {
        Rd[(size_t)s * 9 + q] = rd[q];
        R_Rd[(size_t)s * 9 + q] = right[q];
        Rd_R[(size_t)s * 9 + q] = left[q];
    }
}

// wave_sum_dpp as the fit kernels call it: all 64 lanes of one wave, the total is lane 63's
__global__ void __launch_bounds__(64)
debug_wave_sum_kernel(const double* __restrict__ v, const int n, double* __restrict__ total) {
    const int s = blockIdx.x;
    if (s >= n) return;
    const double t = wave_sum_dpp(v[(size_t)s * 64 + threadIdx.x]);
    if (threadIdx.x == 63) total[s] = t;
}

}  // namespace fls
