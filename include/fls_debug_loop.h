/* ============================================================================
 * fls_debug_loop.h -- test-only entry points of the stages of the loop-closure matcher (same shared library as fls_reg.h; FLS_ABI_REVISION
 * stays 9, this header has a revision of its own).  Each hook runs the production __global__ kernels of csrc/kernels_loop.hpp on the per-device
 * LoopMatcher that fls_loop_match uses, under its run mutex, with the launch geometry of LoopMatcher::run / ndt_eval / gicp_fdf and -- for the
 * three summing kernels -- through LoopMatcher::reduce(): its stream, partial rows, fan-in ticket, host-mapped result block and sequence word are
 * the production ones.  No hook resets the ticket: a launch that leaves it dirty shows in the next one.  tests/test_gpu_loop_stages.py compares
 * every stage with the CPU oracle or a numpy model instead of through the 1e-4 m pose tolerance of a whole Match.
 *
 * Clouds are float rows of `stride` floats (x, y, z first), like fls_loop_match, and are used AS GIVEN: no voxel filter.  Plain host pointers,
 * synchronous.  FLS_ERR_INVALID on a NULL pointer, a negative size, stride < 3 or a non-positive resolution / cell / distance, checked before
 * the device is looked at, with every output left alone.  Matrices are column-major.
 * ==========================================================================*/
#ifndef FLS_DEBUG_LOOP_H
#define FLS_DEBUG_LOOP_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_LOOP_REVISION 1

int fls_debug_loop_revision(void);

/* LoopMatcher::build_target(tgt, resolution), then ONE LoopMatcher::ndt_eval (ndt_p2d_kernel<want_hessian>) over src at the pose vector p
 * (x, y, z, roll, pitch, yaw), T = Translation * Rx * Ry * Rz in float as the line search forms it, gauss_d1 / gauss_d2 as ndt_align sets them.
 * -> score, grad[6], hess[36] (left alone when want_hessian == 0), pairs = the count column (contributing (point, leaf) pairs), leaves = the
 * number of leaf Gaussians, sparse = 1 when build_target chose the open-addressing leaf table.  A target without a leaf of 6 points (or without
 * a finite point): FLS_OK, leaves = 0, zero sums, no launch.  ns == 0 or nt == 0: FLS_OK, every output zero, the device is not looked at. */
fls_status fls_debug_loop_ndt(int device_id, const float* src, int ns, const float* tgt, int nt, int stride, float resolution, const double* p,
                              int want_hessian, double* score, double* grad, double* hess, int64_t* pairs, int32_t* leaves, int32_t* sparse);

/* gicp_cov_kernel over the cloud in its own cell grid (DeviceGridBuilder::run, else CellGridImage::build; host_grid = 1 forces the host
 * build) -> cov[n][9].  LoopMatcher::run never launches it below 20 points (computeCovariances refuses): n < 20 is FLS_ERR_INVALID. */
fls_status fls_debug_loop_gicp_cov(int device_id, const float* cloud, int n, int stride, float cell, double epsilon, int host_grid, double* cov);

/* gicp_corr_kernel: moved[ns] transformed by T[16] (float), 1-NN in the target's grid (cell 1.5 m, ids = cloud indices, by_id set; host_grid as
 * above), gate = float(corr_dist^2), threshold corr_dist^2, R[9] the rotation the source covariances are turned by, cov_src[ns][9],
 * cov_tgt[nt][9] -> corr[ns] (-1: none), mahal[ns][9]; the rows of mahal of unmatched points hold the NaN the hook filled them with.
 * ns == 0: FLS_OK without a launch; nt == 0: every corr -1, no launch. */
fls_status fls_debug_loop_gicp_corr(int device_id, const float* moved, int ns, const float* tgt, int nt, int stride, const float* T, const double* R,
                                    const double* cov_src, const double* cov_tgt, double corr_dist, int host_grid, int32_t* corr, double* mahal);

/* LoopMatcher::gicp_fdf (gicp_fdf_kernel<want_grad>) at x[6], T = apply_state(identity, x), over moved[ns] with the caller's corr[ns] (every
 * entry -1 or in [0, nt), anything else is FLS_ERR_INVALID) and mahal[ns][9] -> the raw reduced row of the result block: v[14] = f sum, g_t[3],
 * Racc[9], count, or v[2] = f sum, count when want_grad == 0.  ns == 0: FLS_OK, zero row, no launch. */
fls_status fls_debug_loop_gicp_fdf(int device_id, const float* moved, int ns, const float* tgt, int nt, int stride, const double* x, const int32_t* corr,
                                   const double* mahal, int want_grad, double* v);

/* loop_fitness_kernel: src[ns] transformed by T[16] (float), un-gated 1-NN in the target's grid (as fls_debug_loop_gicp_corr builds it)
 * -> sum of the squared distances, number of points that found a neighbour.  ns == 0 or nt == 0: FLS_OK, zeros, no launch. */
fls_status fls_debug_loop_fitness(int device_id, const float* src, int ns, const float* tgt, int nt, int stride, const float* T, int host_grid,
                                  double* sum_d2, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif
