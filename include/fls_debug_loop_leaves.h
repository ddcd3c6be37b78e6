/* ============================================================================
 * fls_debug_loop_leaves.h -- test-only entry points of the leaf-Gaussian build of the loop-closure matcher's NDT stages (same shared
 * library as fls_reg.h; this header has a revision of its own, fls_debug_loop.h is unchanged).  Both run on the per-device LoopMatcher
 * that fls_loop_match and fls_loop_match_device use, under its run mutex.  tests/test_gpu_loop_leaves.py compares the device build
 * (csrc/kernels_loop_leaves.hpp) with LoopMatcher::build_target on bits.
 *
 * Clouds are float rows of `stride` floats (x, y, z first), plain host pointers, used AS GIVEN: no voxel filter.  Synchronous.
 * FLS_ERR_INVALID on a NULL pointer, a negative size, stride < 3, a non-positive or non-finite resolution, on_device other than 0 / 1,
 * checked before the device is looked at.
 * ==========================================================================*/
#ifndef FLS_DEBUG_LOOP_LEAVES_H
#define FLS_DEBUG_LOOP_LEAVES_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_LOOP_LEAVES_REVISION 1

int fls_debug_loop_leaves_revision(void);

/* The leaf Gaussians of tgt at `resolution`, rows in emission order (ascending cell index among the leaves of >= 6 points), from
 * LoopMatcher::build_target (on_device == 0) or from the device build on the uploaded cloud (on_device == 1; what that build declines goes
 * through build_target and counts in fls_loop_device_stat slot 4, as in a Match).  Per row: cell[1] (i0 + i1 * div0 + i2 * div0 * div1),
 * n_points[1], mean[3], icov[9] column-major, centroid[3].  *n_leaves is always set; rows are written only when *n_leaves <= cap
 * (FLS_ERR_INVALID otherwise).  *sparse = 1 when the open-addressing leaf table was chosen (0 without leaves).  nt == 0, no finite
 * point, no leaf of 6 points, or a box of more than INT_MAX cells: FLS_OK, *n_leaves = 0. */
fls_status fls_debug_loop_leaves(int device_id, const float* tgt, int nt, int stride, float resolution, int on_device, int32_t* cell,
                                 int32_t* n_points, double* mean, double* icov, float* centroid, int cap, int32_t* n_leaves, int32_t* sparse);

/* fls_debug_loop_ndt (fls_debug_loop.h) with the leaves built on the device: the table ndt_p2d_kernel reads here is the one the device
 * build filled, as in fls_loop_match_device.  Same arguments, same outputs. */
fls_status fls_debug_loop_ndt_device(int device_id, const float* src, int ns, const float* tgt, int nt, int stride, float resolution, const double* p,
                                     int want_hessian, double* score, double* grad, double* hess, int64_t* pairs, int32_t* leaves, int32_t* sparse);

#ifdef __cplusplus
}
#endif
#endif
