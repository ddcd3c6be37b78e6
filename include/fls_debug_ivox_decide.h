/* ============================================================================
 * fls_debug_ivox_decide.h -- test-only entry points of the iVox map-update DECISION (same shared library as fls_reg.h; FLS_ABI_REVISION stays 9,
 * this header has a revision of its own).
 *
 * After a converged Match in mapping mode FLS_P2PLANE_IVOX decides per source point what goes into the map, by the rule of
 * LoamPointToPlaneIVOX::AddCloudToLocalMap (loam_point_to_plane_ivox.h:79-131): code 0 drops the point, 1 is points_to_add, 2 is
 * point_no_need_downsample.  On the device that is ivox_add_decide_kernel<MATERIALIZE> (csrc/kernels_ivox_coop.hpp), which in the same launch
 * turns ids-form neighbour lists into rows, counts the two insertion codes per block, resets the batch status words and, in its speculative
 * form, decides from the Gauss-Newton state whether there is an update at all.  On the host it is ivox_decide_host (csrc/matcher_p2plane_ivox.hpp),
 * what fls_add_cloud_to_local_map runs for a later cloud that is not the resident scan.  The hooks run exactly those: the device hooks launch
 * through the functions the matcher launches through (launch_add_decide, launch_nn_materialize: one grid rule, one argument order), the host
 * hook calls the function add_cloud_impl calls.  tests/test_gpu_ivox_decide.py and tests/test_ivox_decide_cases.py compare them with the CPU
 * oracle's rule on the constructed cases of tests/ivox_decide_cases.py.
 *
 * Same shape as fls_debug_fit.h: plain host pointers, synchronous, FLS_ERR_INVALID for a NULL array, a negative size or a bad flag (checked
 * before the device is looked at, nothing written), n == 0 is FLS_OK without a launch.
 *
 * Neighbour lists, as the matcher keeps them: nn_cnt[i] bits 0-2 the count, bit 7 set when list i is in ROWS form (its points stand in
 * nn_rows[i][0..4] as x, y, z, id bits), clear when it is in IDS form (nn_ids[i][0..4] are map slots, words 5-7 belong to the kNN kernel).
 * ==========================================================================*/
#ifndef FLS_DEBUG_IVOX_DECIDE_H
#define FLS_DEBUG_IVOX_DECIDE_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_IVOX_DECIDE_REVISION 1
#define FLS_DEBUG_IVOX_DECIDE_FILL 0xA5    /* every byte of every output buffer before the launch */
#define FLS_DEBUG_IVOX_DECIDE_MAP_PAD 64   /* sentinel rows behind map_rows[n_slots] */

int fls_debug_ivox_decide_revision(void);

/* The speculative form's view of GnState: the launch runs when (done != 0 || iter >= max_iterations) && n_valid >= 50, and then takes T as the pose. */
typedef struct fls_debug_ivox_gate {
    int32_t done, iter, n_valid, max_iterations;
    double T[16];
} fls_debug_ivox_gate;

/* One launch of ivox_add_decide_kernel<materialize != 0> over m = materialize ? max(n, nn_n) : n points in ceil(m / 256) workgroups.
 *   src_xyz[n][3], T[16] (column-major), fs (filter_size_map_min)
 *   nn_rows[nn_n][5][4] and nn_cnt[nn_n]: uploaded, and read back after the launch (in/out)
 *   nn_ids[nn_n][8] or NULL (NULL: every list is taken as rows form; FLS_ERR_INVALID if a count byte then has bit 7 clear and a non-zero count)
 *   map_rows[n_slots][4] or NULL with n_slots == 0.  The device copy has FLS_DEBUG_IVOX_DECIDE_MAP_PAD more rows, each a copy of sentinel[4]:
 *     the slot bound the kernel is given is n_slots, so a kernel that ignored it would return the sentinel instead of reading unmapped memory.
 *   count != 0: lx, bt and status are passed (and must not be NULL); 0: the kernel gets null pointers and the three arrays keep the fill.
 *   gate or NULL (not speculative).  A gate with count == 0 is FLS_ERR_INVALID: a launch that skips writes the status words unconditionally.
 *   -> code[n], pw[n][4], lx[n][2], bt[ceil(m / 256)][2], status[2] = {status, apply}; each prefilled with FLS_DEBUG_IVOX_DECIDE_FILL bytes on the
 *      device, so that what the kernel did not write shows.
 * The device buffers of the lists hold max(m, nn_n) entries: for i in [nn_n, n) the materializing form may load ids row i before it finds the
 * count to be 0 (in the matcher n <= nn_n whenever that form is launched: both are the size of the scan just matched).
 * materialize == 0 with lists in ids form answers an id beyond n_slots with slot 0, not with the (0, 0, 0, id -1) row of the other form.  The
 * matcher never launches that combination: launch_decide takes the materializing form whenever a list may be in ids form (a speculative launch,
 * or nn_rows_current false) and nn_n > 0, and with nn_n == 0 every count is 0 and no neighbour is read. */
fls_status fls_debug_ivox_decide(int device_id, const float* src_xyz, int n, const double* T, double fs, float* nn_rows, uint8_t* nn_cnt, int nn_n,
                                 const uint32_t* nn_ids, const float* map_rows, int n_slots, const float* sentinel, int materialize, int count,
                                 const fls_debug_ivox_gate* gate, uint8_t* code, float* pw, uint32_t* lx, uint32_t* bt, uint32_t* status);

/* One launch of ivox_nn_materialize_kernel over nn_n lists: nn_ids[nn_n][8], nn_cnt[nn_n] (in/out), map_rows[n_slots][4] (or NULL with n_slots == 0)
 * padded with sentinel[4] rows as above, nn_rows[nn_n][5][4] (in/out).  nn_n == 0 is FLS_OK without a launch. */
fls_status fls_debug_ivox_nn_materialize(int device_id, const uint32_t* nn_ids, uint8_t* nn_cnt, int nn_n, const float* map_rows, int n_slots,
                                         const float* sentinel, float* nn_rows);

/* The rule on the host, no device: ivox_decide_host, the loop fls_add_cloud_to_local_map runs for a later cloud that is not the resident scan.
 * src_xyz[n][3], T[16], fs, nn[n][5][3], cnt[n] (plain counts) -> code[n], pw[n][3]. */
fls_status fls_debug_ivox_decide_host(const float* src_xyz, const double* T, double fs, const float* nn, const uint8_t* cnt, int n, uint8_t* code, float* pw);

#ifdef __cplusplus
}
#endif
#endif
