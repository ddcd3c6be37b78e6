// kernels_debug_fit.hpp -- test hooks of include/fls_debug_fit.h: every kernel calls ONE stage of the fit launch -- the __forceinline__ routine
// itself, in this translation unit and with its flags, on the LDS structs the product kernels hand it -- on caller-supplied inputs.
// tests/test_gpu_fit_stages.py compares the results with the oracle or with numpy models of the fixed summation orders.
#pragma once
#include "kernels_p2plane.hpp"
#include "kernels_knn.hpp"
#include "kernels_grid_coop.hpp"

namespace fls {

constexpr int kDebugFitBlock = 64;

// plane_residual_dev / line_residual_dev as the fit kernels call them: the neighbours, ps and pt are floats (given as doubles that hold float
// values), T a 4x4 column-major pose of which only the rotation may enter J; one lane per system.  J and d keep the canary 7.0 where the
// routine leaves them unwritten.
template <bool LINE>
__global__ void __launch_bounds__(kDebugFitBlock)
debug_residual_kernel(const double* __restrict__ nn, const double* __restrict__ ps, const double* __restrict__ pt, const double* __restrict__ T,
                      const double* __restrict__ gate, const int n, double* __restrict__ valid, double* __restrict__ J, double* __restrict__ d) {
    const int s = blockIdx.x * kDebugFitBlock + threadIdx.x;
    if (s >= n) return;
    float4 nf[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) nf[j] = make_float4((float)nn[(size_t)s * 15 + j * 3], (float)nn[(size_t)s * 15 + j * 3 + 1], (float)nn[(size_t)s * 15 + j * 3 + 2], 0.f);
    double Tl[16], Jl[6], dl = 7.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) Tl[q] = T[(size_t)s * 16 + q];
#pragma unroll
    for (int q = 0; q < 6; ++q) Jl[q] = 7.0;
    const float sx = (float)ps[(size_t)s * 3], sy = (float)ps[(size_t)s * 3 + 1], sz = (float)ps[(size_t)s * 3 + 2];
    const float tx = (float)pt[(size_t)s * 3], ty = (float)pt[(size_t)s * 3 + 1], tz = (float)pt[(size_t)s * 3 + 2];
    bool ok;
    if (LINE) ok = line_residual_dev(nf, sx, sy, sz, tx, ty, tz, Tl, gate[s], Jl, dl);
    else ok = plane_residual_dev(nf, sx, sy, sz, tx, ty, tz, Tl, gate[s], Jl, dl);
    valid[s] = ok ? 1.0 : 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) J[(size_t)s * 6 + q] = Jl[q];
    d[s] = dl;
}

// icp_point_rows as icp_knn_fit_body calls it: source point p and map point m are floats (given as doubles that hold float values); one lane per system
__global__ void __launch_bounds__(kDebugFitBlock)
debug_icp_point_rows_kernel(const double* __restrict__ T, const double* __restrict__ p, const double* __restrict__ m, const int n, double* __restrict__ J,
                            double* __restrict__ e, double* __restrict__ res) {
    const int s = blockIdx.x * kDebugFitBlock + threadIdx.x;
    if (s >= n) return;
    double Tl[16], Jl[18], el[3], rl = 7.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) Tl[q] = T[(size_t)s * 16 + q];
    const float4 mf = make_float4((float)m[(size_t)s * 3], (float)m[(size_t)s * 3 + 1], (float)m[(size_t)s * 3 + 2], 0.f);
    icp_point_rows(Tl, (float)p[(size_t)s * 3], (float)p[(size_t)s * 3 + 1], (float)p[(size_t)s * 3 + 2], mf, Jl, el, rl);
#pragma unroll
    for (int q = 0; q < 18; ++q) J[(size_t)s * 18 + q] = Jl[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) e[(size_t)s * 3 + q] = el[q];
    res[s] = rl;
}

// reduce_rank1_mfma_and_store (FORM 0), reduce_rank1_and_store (1), reduce_rank1x3_mfma_and_store (2) as the fit kernels call them: workgroups of
// four waves, case 4 blockIdx.x + wave in wave slot `wave` with the LDS row wsum[wave] and the tile mfma_tile[wave] of the product kernels.
// W = doubles of J per lane (6, or 18 for the three-row form), E = residual entries per lane (1 or 3).  The row is prefilled with 7.0.
template <int FORM>
__global__ void __launch_bounds__(256)
debug_rank1_kernel(const double* __restrict__ contrib, const double* __restrict__ J, const double* __restrict__ r, const int n, double* __restrict__ rows) {
    constexpr int W = FORM == 2 ? 18 : 6, E = FORM == 2 ? 3 : 1;
    __shared__ double wsum[4][32];
    __shared__ __attribute__((aligned(64))) double mfma_tile[4][512];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + wave;
    if (s >= n) return;  // (wave-uniform; nothing below synchronises the workgroup)
    if (lane < 32) wsum[wave][lane] = 7.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const size_t l = (size_t)s * 64 + lane;
    const bool c = contrib[l] != 0.0;
    double Jl[W], rl[E];
#pragma unroll
    for (int q = 0; q < W; ++q) Jl[q] = J[l * W + q];
#pragma unroll
    for (int q = 0; q < E; ++q) rl[q] = r[l * E + q];
    if constexpr (FORM == 0) reduce_rank1_mfma_and_store(c, Jl, rl[0], &wsum[wave][0], &mfma_tile[wave][0]);
    else if constexpr (FORM == 1) reduce_rank1_and_store(c, Jl, rl[0], &wsum[wave][0]);
    else reduce_rank1x3_mfma_and_store(c, Jl, rl, &wsum[wave][0], &mfma_tile[wave][0]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 32) rows[(size_t)s * 32 + lane] = wsum[wave][lane];
}

// reduce_partials<NT, SC1, U> as the tails call it: one workgroup of NT threads, the tail's own LDS struct (LuTailSmem: red + tot; LoamTailSmem:
// red + tot_b)
template <int NT, bool SC1, int U, class Smem>
__global__ void __launch_bounds__(NT)
debug_reduce_partials_kernel(const double* __restrict__ rows, const int nrows, double* __restrict__ tot) {
    __shared__ Smem sm;
    double* t;
    if constexpr (std::is_same<Smem, LuTailSmem>::value) t = sm.tot; else t = sm.tot_b;
    reduce_partials<NT, SC1, U>(rows, nrows, t, sm.red);
    if (threadIdx.x < 32) tot[threadIdx.x] = t[threadIdx.x];
}

// publish_row_and_arrive + fanin_last_arriver as the fused fit kernels call them: workgroup b publishes the row v(b, col) = mul (b + 1)(col + 1) + add b
// (all 32 columns); a workgroup told it is the last counts itself, sums the rows the way lu_tail<256, true> does and stores the totals.  Nothing
// here waits for another workgroup.
__global__ void __launch_bounds__(256)
debug_fanin_kernel(double* __restrict__ partials, unsigned* __restrict__ ticket, const int shards, const double mul, const double add,
                   unsigned* __restrict__ last_count, double* __restrict__ tot) {
    __shared__ unsigned s_ticket;
    __shared__ LuTailSmem sm;
    const double v = mul * (double)((blockIdx.x + 1u) * ((threadIdx.x & 31u) + 1u)) + add * (double)blockIdx.x;
    if (!publish_row_and_arrive(v, threadIdx.x < 32, partials, ticket, shards, LaunchBlocksX{}, s_ticket)) return;
    if (threadIdx.x == 0) __hip_atomic_fetch_add(last_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    reduce_partials<256, true, 32>(partials, (int)gridDim.x, sm.tot, sm.red);
    if (threadIdx.x < 32) tot[threadIdx.x] = sm.tot[threadIdx.x];
}

}  // namespace fls
