/* ============================================================================
 * fls_debug_knn.h -- test-only entry points of the cooperative grid k-NN kernels of the three kd-tree kinds (same shared library as fls_reg.h;
 * FLS_ABI_REVISION stays 9, this header has a revision of its own).  Each hook builds the cell grid of the caller's map cloud the way the
 * matchers do and launches a PRODUCT instantiation of csrc/kernels_grid_coop.hpp as it is -- grid_knn_kernel<5, false> (gated),
 * grid_knn_kernel<5, false, true> (un-gated: ring walk and serial hand-off), grid_knn_dual_kernel<5, false>, icp_knn_fit_kernel -- with
 * knn_grid_blocks(nq) workgroups of 256 threads and first = 1 (the pose is T16, no state is read).  tests/test_gpu_knn_stages.py compares the
 * lists with a brute-force model bit for bit instead of through the pose and the tie budget of a whole Match.
 *
 * Clouds are float rows of `stride` floats (x, y, z first) and are used AS GIVEN: no voxel filter; the id of a map point is its row.  T16 is a
 * column-major 4x4 of doubles.  host_grid = 0: the grid is built on the device (DeviceGridBuilder::run), and on the host where that build
 * declines; 1: CellGridImage::build.  out_has_window: 1 when the grid got a dense cell window, 0 when the search goes through the hash table.
 * Plain host pointers, synchronous.  FLS_ERR_INVALID on a NULL pointer, a negative size, stride < 3, a non-finite or non-positive cell, rings
 * outside {1, 2}, a NaN gate (a non-finite or non-positive max_corr_sq) or host_grid outside {0, 1}, checked before the device is looked at,
 * with every output left alone.
 * ==========================================================================*/
#ifndef FLS_DEBUG_KNN_H
#define FLS_DEBUG_KNN_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_KNN_REVISION 1

int fls_debug_knn_revision(void);

/* The 5 nearest map points of every query T16 * query[i] (float64 products summed left to right, rounded to float).  gate is a SQUARED distance;
 * INFINITY selects the un-gated instantiation, as FeatureDev::launch does.  -> out_pts[nq][5][4]: the raw float4 rows {x, y, z, id bits}, id -1
 * marks an empty slot; out_cnt[nq]: neighbours found (<= 5); out_kth[nq]: the squared distance of the 5th (INFINITY when fewer were found).
 * nm == 0 or nq == 0: FLS_OK without a launch -- counts 0, ids -1, out_kth INFINITY, out_has_window 0. */
fls_status fls_debug_grid_knn5(int device_id, const float* map, int nm, const float* query, int nq, int stride, float cell, int rings, float gate,
                               const double* T16, int host_grid, float* out_pts, uint8_t* out_cnt, float* out_kth, int32_t* out_has_window);

/* Two searches (gated, as LoamFullMatcher runs its corner and planar classes) in ONE grid_knn_dual_kernel launch of knn_grid_blocks(nq_a) +
 * knn_grid_blocks(nq_b) workgroups, nb_a = knn_grid_blocks(nq_a); one pose for both.  A non-finite gate is FLS_ERR_INVALID (the dual kernel has
 * no un-gated form), and so is an empty map or query set on either side (the matcher launches the dual kernel only when both classes have points). */
fls_status fls_debug_grid_knn5_dual(int device_id, const float* map_a, int nm_a, const float* query_a, int nq_a, float cell_a, int rings_a, float gate_a,
                                    const float* map_b, int nm_b, const float* query_b, int nq_b, float cell_b, int rings_b, float gate_b, int stride,
                                    const double* T16, int host_grid, float* out_pts_a, uint8_t* out_cnt_a, float* out_kth_a, int32_t* out_has_window_a,
                                    float* out_pts_b, uint8_t* out_cnt_b, float* out_kth_b, int32_t* out_has_window_b);

/* icp_knn_fit_kernel with ticket = nullptr (the Gauss-Newton tail does not run), gate = float(max_corr_sq) and max_corr = max_corr_sq as
 * IcpMatcher passes them, rings = 1, the query transformed in float (xform_f).  -> out_id[nq]: the nearest map point's id where its squared
 * distance is within max_corr_sq, else -1; out_eff[nq]: 1 / 0.  nm == 0 or nq == 0: FLS_OK without a launch, ids -1, eff 0, out_has_window 0. */
fls_status fls_debug_icp_knn1(int device_id, const float* map, int nm, const float* query, int nq, int stride, float cell, double max_corr_sq,
                              const double* T16, int host_grid, int32_t* out_id, uint8_t* out_eff, int32_t* out_has_window);

#ifdef __cplusplus
}
#endif
#endif
