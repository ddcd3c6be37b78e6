/* ============================================================================
 * fls_batch_ivox.h -- C ABI of the shared-launch batch of the iVox point-to-plane kind (same shared library as fls_reg.h and
 * fls_batch.h, which both stay as they are; this header has a revision of its own): fls_match_batch's independent registrations
 * against the handle's current map, with the two launches of a Gauss-Newton iteration SHARED by up to n_slots jobs.
 *
 * A single iVox registration is two launches per iteration (csrc/kernels_ivox_coop.hpp: ivox_knn_kernel, then
 * p2plane_fit_solve_kernel, whose last workgroup solves the 6x6 system).  Here the jobs of a group are the rows of one grid with a
 * job dimension (ivox_knn_jobs_kernel, p2plane_fit_solve_jobs_kernel): the serial fan-in and single-wave tail of one job run beside
 * the other jobs' work, and a group of G jobs costs max(iterations) launch pairs, not their sum.
 *
 * What a job computes is unchanged: what a fresh handle holding this map returns for fls_match(scan_j, T_j, update_map = 0), bit for
 * bit (pose, iterations, n_valid, status) -- no map update, no state carried from job to job, the owner's own Match state untouched.
 *
 * Kinds: FLS_P2PLANE_IVOX has this form.  On every other kind the call is fls_match_batch_fused (fls_batch.h).
 * fls_match_batch_fused itself keeps running iVox handles as fls_match_batch does.
 *
 * Plain C; no exception crosses the boundary; a handle is not thread-safe.  Arguments are validated before the device is looked at.
 * ==========================================================================*/
#ifndef FLS_BATCH_IVOX_H
#define FLS_BATCH_IVOX_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_BATCH_IVOX_REVISION 1

int fls_batch_ivox_revision(void);

/* The arguments of fls_match_batch_fused: n_jobs scans (src0[j], n0[j] rows of stride_floats floats; src1 / n1 NULL, or both set and
 * ignored by this kind), T = n_jobs x 16 doubles, column-major, the initial guess on entry and the result on return; stats and status
 * may be NULL.  n_slots (clamped to 1..16) = the jobs per group.
 *
 * Slots are the handle's lane clones (shared with fls_match_batch); each uploads its job's scan on its own stream.  The group's
 * launches follow on one batch stream, queued in chunks (the first sized by the previous group's largest iteration count, then two
 * iterations at a time) until every job's mailbox shows that it stopped or max_iterations iterations are out.  With more than one
 * group a second set of n_slots clones uploads the next group's scans while this group iterates.  Nothing stays queued on return.
 *
 * An iteration of a group is one kNN launch and one fit launch per workgroup-size class present in it: a job of up to 65,536 points
 * keeps the 256-thread fit workgroups the single-job path gives it, a larger one the 512-thread ones, so a mixed group queues two fit
 * launches per iteration.  A job that has stopped leaves each later launch at once.
 *
 * A job with n0[j] == 0 is answered on the host as fls_match answers it (FLS_NOT_CONVERGED, one logged iteration) and joins no
 * launch.  It does not stop the other jobs.
 *
 * Return value, as fls_match_batch_fused: EVERY job runs, status[j] is set for all of them, and the call returns the first negative
 * status by job index (FLS_OK when there is none; FLS_NOT_CONVERGED is a per-job status, not an error).  Errors that are not a
 * job's (called on a lane: FLS_ERR_STATE; a HIP error on the batch stream: FLS_ERR_DEVICE) end the call; jobs not reached stay
 * FLS_SKIPPED.  FLS_ERR_INVALID: NULL handle, stride_floats < 3, NULL src0 / n0 / T with n_jobs > 0, src1 and n1 not both NULL or
 * both set, a NULL src0[j] with n0[j] > 0.  n_jobs == 0: FLS_OK, nothing is touched. */
fls_status fls_match_batch_shared_ivox(fls_handle h, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                       const size_t* n1, int stride_floats, double* T_colmajor, fls_stats* stats, int32_t* status, int n_slots);

/* counters since the handle was created: 0 shared kNN launches queued, 1 shared fit launches queued, 2 jobs that ran in shared
 * launches, 3 jobs that ran outside them, 4 groups.  Other slots and a NULL handle: 0.  fls_batch_stat's counters are not touched
 * by fls_match_batch_shared_ivox on an iVox handle. */
size_t fls_batch_ivox_stat(fls_handle h, int slot);

#ifdef __cplusplus
}
#endif
#endif
