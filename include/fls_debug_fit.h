/* ============================================================================
 * fls_debug_fit.h -- test-only entry points of the stages of the fit launch (same shared library as fls_reg.h; FLS_ABI_REVISION stays 9,
 * this header has a revision of its own).  Each hook runs ONE routine of csrc/kernels_p2plane.hpp, kernels_knn.hpp or kernels_grid_coop.hpp
 * -- the __forceinline__ routine itself, compiled with the flags of the kernels that call it and on their LDS structs -- on caller-supplied
 * inputs, so that tests/test_gpu_fit_stages.py can compare it with the CPU oracle or a numpy model of its fixed order instead of through the
 * 1e-4 pose tolerance of a whole Match.  Same shape as fls_debug_linalg.h: plain host pointers, synchronous, FLS_ERR_INVALID on a NULL
 * pointer or a negative n (checked before the device is looked at), n == 0 is FLS_OK without a launch.  Every value is a double; where the
 * routine takes floats (neighbours, points) the doubles hold float values and the kernel converts them.  Matrices are column-major.
 * ==========================================================================*/
#ifndef FLS_DEBUG_FIT_H
#define FLS_DEBUG_FIT_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_FIT_REVISION 1
#define FLS_DEBUG_TICKET_WORDS 320 /* kTicketWords */

int fls_debug_fit_revision(void);

/* plane_residual_dev / line_residual_dev, one lane per system: nn[n][5][3] (nn[s][0] the nearest), ps[n][3] source point, pt[n][3] transformed
 * point, T[n][16], gate[n] (plane threshold / line ratio, per system) -> valid[n] (1.0 / 0.0), J[n][6], d[n] (d_abs / dist).  J and d hold
 * 7.0 wherever the routine returned without writing them. */
fls_status fls_debug_plane_residual(int device_id, const double* nn, const double* ps, const double* pt, const double* T, const double* gate, int n,
                                    double* valid, double* J, double* d);
fls_status fls_debug_line_residual(int device_id, const double* nn, const double* ps, const double* pt, const double* T, const double* gate, int n,
                                   double* valid, double* J, double* d);

/* icp_point_rows, one lane per system: T[n][16], p[n][3] source point, m[n][3] map point -> J[n][18] (3 x 6 column-major), e[n][3], res[n]. */
fls_status fls_debug_icp_point_rows(int device_id, const double* T, const double* p, const double* m, int n, double* J, double* e, double* res);

/* reduce_rank1_mfma_and_store / reduce_rank1_and_store / reduce_rank1x3_mfma_and_store, one wave per case, case s in wave slot s % 4 of workgroup
 * s / 4: contrib[n][64] (non-zero = true), J[n][64][6] and r[n][64], or J[n][64][18] and e[n][64][3] for x3 -> row[n][32], prefilled with 7.0
 * (x3 leaves column 27 to its caller). */
fls_status fls_debug_rank1_mfma(int device_id, const double* contrib, const double* J, const double* r, int n, double* row);
fls_status fls_debug_rank1_dpp(int device_id, const double* contrib, const double* J, const double* r, int n, double* row);
fls_status fls_debug_rank1x3_mfma(int device_id, const double* contrib, const double* J, const double* e, int n, double* row);

/* reduce_partials<NT, SC1, U>, one workgroup: variant 0 <256, true, 32>, 1 <512, true, 16>, 2 <512, true, 32>, 3 <1024, false, 16>;
 * rows[nrows][32] (uploaded before the launch) -> tot[32].  FLS_ERR_INVALID for any other variant. */
fls_status fls_debug_reduce_partials(int device_id, int variant, const double* rows, int nrows, double* tot);

/* publish_row_and_arrive + fanin_last_arriver: TWO launches of nblocks workgroups of 256 threads on the same ticket words, which are zeroed once
 * before the first.  In launch k workgroup b publishes row v(b, col) = (k + 1)(b + 1)(col + 1) + 1000 k b, col = 0..31; every workgroup told it
 * is the last adds one to last[k], sums the rows with reduce_partials<256, true, 32> and writes tot[k][32].  ticket[FLS_DEBUG_TICKET_WORDS]: the
 * words after both launches.  shards: 1 or 8 as the host launches pass it.  FLS_ERR_INVALID unless 1 <= nblocks <= 65535. */
fls_status fls_debug_fanin(int device_id, int nblocks, int shards, double* tot, uint32_t* last, uint32_t* ticket);

/* GnState::H (36, column-major) and GnState::g (6) of the handle's last iteration, after synchronising its stream.  FLS_ERR_STATE before the first Match. */
fls_status fls_debug_last_system(fls_handle h, double* H36, double* g6);

#ifdef __cplusplus
}
#endif
#endif
