/* ============================================================================
 * fls_batch.h -- C ABI of the fused batch (same shared library as fls_reg.h; FLS_ABI_REVISION stays 9, this header has a revision
 * of its own): fls_match_batch's independent registrations against the handle's current map, with the iteration launches of up to
 * n_slots jobs SHARED -- one launch per Gauss-Newton iteration for the whole group instead of one per job.
 *
 * fls_match_batch gives every job a lane (a clone of the handle with its own stream and host thread) and every lane issues its own
 * launches.  For IcpOptimized one launch of a full-size scan fills a fraction of an MI355X and half of it is the single-wave
 * Gauss-Newton tail of one workgroup; the lanes interleave whole launches, so every job still pays every launch and every tail.
 * Here the jobs of a group are the rows of one grid (csrc/kernels_grid_coop.hpp: icp_knn_fit_jobs_kernel): the tail of one job runs
 * beside the searches of the others, and a group of G jobs costs max(iterations) launches, not their sum.
 *
 * What a job computes is unchanged: what a fresh handle holding this map returns for fls_match(scan_j, T_j, update_map = 0), bit for
 * bit (pose, iterations, n_valid, status) -- no map update, no state carried from job to job, the owner's own Match state untouched.
 *
 * Kinds: FLS_ICP_OPTIMIZED has the fused form.  For every other kind the result equals fls_match_batch with n_slots lanes.
 *
 * Plain C; no exception crosses the boundary; a handle is not thread-safe.  Arguments are validated before the device is looked at.
 * ==========================================================================*/
#ifndef FLS_BATCH_H
#define FLS_BATCH_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_BATCH_REVISION 1

int fls_batch_revision(void);

/* The arguments of fls_match_batch: n_jobs scans (src0[j], n0[j] rows of stride_floats floats; src1 / n1 the second cloud of the
 * two-cloud kinds, both NULL otherwise), T = n_jobs x 16 doubles, column-major, the initial guess on entry and the result on return;
 * stats and status may be NULL.  n_slots (clamped to 1..16) = the jobs per group.
 *
 * Slots are the handle's lane clones (shared with fls_match_batch).  Per group every slot uploads and source-filters its job on its
 * own stream; the group's iteration launches follow on one batch stream, queued in chunks (the first sized by the previous group's
 * largest iteration count, then two at a time) until every job's mailbox shows that it stopped or max_iterations launches are out.
 * With more than one group a second set of n_slots clones filters the next group's scans while this group iterates.
 *
 * Jobs that do not join the shared launches: a job the single-job path rejects keeps that status (10 points or fewer:
 * FLS_ERR_INVALID); a job whose filtered scan is empty runs on the per-lane path.  Neither stops the other jobs.
 *
 * Return value -- DIFFERENT from fls_match_batch, which stops a lane at its first negative status and leaves that lane's later jobs
 * FLS_SKIPPED: here EVERY job runs, status[j] is set for all of them, and the call returns the first negative status by job index
 * (FLS_OK when there is none; FLS_NOT_CONVERGED is a per-job status, not an error).  Errors that are not a job's (no map:
 * FLS_ERR_STATE; called on a lane; a HIP error on the batch stream: FLS_ERR_DEVICE) end the call; jobs not reached stay FLS_SKIPPED.
 * FLS_ERR_INVALID: NULL handle, stride_floats < 3, NULL src0 / n0 / T with n_jobs > 0, src1 and n1 not both NULL or both set, a NULL
 * src0[j] with n0[j] > 0.  n_jobs == 0: FLS_OK, nothing is touched. */
fls_status fls_match_batch_fused(fls_handle h, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                 const size_t* n1, int stride_floats, double* T_colmajor, fls_stats* stats, int32_t* status, int n_slots);

/* counters since the handle was created: 0 shared iteration launches queued, 1 jobs that ran in shared launches, 2 jobs that took
 * the per-lane path (every job of a kind without the fused form), 3 groups.  Other slots and a NULL handle: 0. */
size_t fls_batch_stat(fls_handle h, int slot);

#ifdef __cplusplus
}
#endif
#endif
