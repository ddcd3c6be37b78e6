/* ============================================================================
 * fls_debug_tail.h -- test-only entry points of the Gauss-Newton TAILS (same shared library as fls_reg.h; FLS_ABI_REVISION stays 9, this header
 * has a revision of its own).
 *
 * Every Match ends each iteration in loam_tail (csrc/kernels_p2plane.hpp: PointToPlane_IVOX, LoamFull, the kd-tree point-to-plane kind) or in
 * lu_tail (csrc/kernels_knn.hpp: IcpOptimized in mode 0, IncrementalNDT in mode 1): sum the partial rows, assemble H and g, solve, apply the
 * step to the pose, decide whether the Match stops, write GnState, publish the mailbox.  Each hook runs ONE launch of ONE workgroup of a tail on
 * caller-supplied rows, state bytes and mailbox bytes, so that tests/test_gpu_tails.py can compare every word a tail writes (and every byte it
 * must not write) with a plain model of the reference's loop instead of through whole Matches on scenes that converge in a few well-conditioned
 * iterations.
 *
 *   variant 0: the PRODUCT kernel itself, gn_solve_loam_kernel / gn_solve_lu_kernel (1024 threads, plain loads of the rows)
 *   variant 1: a test kernel of 256 threads, variant 2: one of 512 threads.  Each loads done, the pose, last_rot / last_pos and iter the way the
 *              fused kernels do, returns when done, then calls loam_tail<NT, true> / lu_tail<NT, true> (the instantiations of the fused
 *              launches: rows read with write-through-coherent loads) on the product's own LDS struct.
 *
 * Plain host pointers, synchronous.  FLS_ERR_INVALID for a NULL T0 / state / rows, a variant outside 0..2, a mode outside 0..1, nrows (nrows_b)
 * outside 1..FLS_DEBUG_TAIL_MAX_ROWS, nrows_a outside 0..FLS_DEBUG_TAIL_MAX_ROWS or a NULL rows_a with nrows_a > 0 -- checked before the device
 * is looked at, nothing written.  The state and the mailbox are device buffers initialised from the caller's bytes (which carry the caller's
 * canary) and copied back whole after the launch; the mailbox is plain device memory.  Rows are rows[nrows][32] doubles; the device copy is
 * followed by one trip of NaN rows, so that a load past nrows shows in H instead of leaving the allocation.  nrows_a == 0 hands the kernel a
 * null rows_a, as the single-class matchers do.  mailbox may be NULL: the kernel then gets a null mailbox.  The state's device copy is followed
 * by FLS_DEBUG_TAIL_GUARD bytes up to where the log slots of iteration 255 would end; FLS_ERR_RANGE (state and mailbox still copied back) when
 * the launch changed one of them: a tail that logged past FLS_DEBUG_TAIL_MAX_ITER stays inside the allocation and is reported.
 * ==========================================================================*/
#ifndef FLS_DEBUG_TAIL_H
#define FLS_DEBUG_TAIL_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_TAIL_REVISION 1
#define FLS_DEBUG_TAIL_MAX_ITER 64    /* kMaxIter: slots of the per-iteration logs */
#define FLS_DEBUG_TAIL_MAX_ROWS 2048
#define FLS_DEBUG_TAIL_GUARD 0xC3     /* every byte behind the state's device copy before the launch */

int fls_debug_tail_revision(void);

/* GnState (csrc/device_common.hpp), field by field; matrices column-major */
typedef struct fls_debug_gn_state {
    double T[16];
    double last_rot, last_pos;
    double sum_res, sum_res2;
    double last_dx[6];
    double H[36], g[6];
    int32_t iter, done, converged, n_valid, n_valid2, pad;
    int64_t dbg[16];
    double log_T[FLS_DEBUG_TAIL_MAX_ITER][16];
    double log_res[FLS_DEBUG_TAIL_MAX_ITER];
    int32_t log_nv[FLS_DEBUG_TAIL_MAX_ITER];
} fls_debug_gn_state;

/* Mailbox (csrc/device_common.hpp), field by field */
typedef struct fls_debug_mailbox {
    double T[16];
    double sum_res, sum_res2;
    double last_dx[6];
    int32_t iter, done, converged, n_valid, n_valid2;
    uint32_t seq;
} fls_debug_mailbox;

/* One launch of the LOAM-family tail: rows_a the corner rows (NULL with nrows_a == 0), rows_b the planar rows, launch_word a LaunchWord
 * (max_iterations << 24 | exact-solver flag << 23 | match id). */
fls_status fls_debug_loam_tail(int device_id, int variant, int first, const double* T0, fls_debug_gn_state* state, const double* rows_a, int nrows_a,
                               const double* rows_b, int nrows_b, double rot_thr, double pos_thr, uint32_t launch_word, fls_debug_mailbox* mailbox);

/* One launch of the ICP (mode 0) / NDT (mode 1) tail. */
fls_status fls_debug_lu_tail(int device_id, int variant, int first, const double* T0, fls_debug_gn_state* state, const double* rows, int nrows, int mode,
                             double rot_thr, double pos_thr, int min_effective, uint32_t launch_word, fls_debug_mailbox* mailbox);

#ifdef __cplusplus
}
#endif
#endif
