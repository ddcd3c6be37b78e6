/* ============================================================================
 * fls_knn_order.h -- C ABI of the neighbour ORDER of the iVox point-to-plane kind (same shared library as fls_reg.h, which stays as
 * it is; this header has a revision of its own).
 *
 * LoamPointToPlaneIVOX selects a point's five neighbours with std::nth_element calls that compare distances alone.  By default this
 * library orders candidates by (distance bits, map slot): the same five neighbours wherever no two candidates lie at exactly the same
 * float distance, in ascending order.  Two things then differ from the reference: under an exact distance tie the reference keeps
 * whichever candidate libstdc++'s introselect leaves in front, and slots 1..4 of every list are in introselect order, not ascending
 * (so the 5x3 plane fit sees its rows in another order).
 *
 * FLS_KNN_ORDER_REFERENCE replays the reference's selection itself (csrc/knn_reference_order.hpp: the 19 voxel probes in its order, a
 * voxel's points in insertion order, libstdc++'s nth_element restated): fls_get_correspondences then returns the reference's lists
 * element for element, ties included.  It is a parity mode: one lane replays one query sequentially, a Match costs several times
 * the default's.  The default order, its kernels and its results do not change.
 *
 * Limit: a query is replayed in a work array of W records (fls_knn_order_limits), which holds 5 x 18 + the points of one voxel.  A
 * query that probes a voxel of more than W - 90 points keeps the default order; fls_map_size slot 178 counts such queries, once per
 * launch (177 counts the kNN launches run in reference order).  The traffic counters of fls_set_profiling (bit 1) belong to the
 * default kernel: a reference-order Match leaves them zero.  The launch events (bit 0) time the reference-order launches as usual.
 *
 * Batches: the lane clones of fls_match_batch inherit the mode.  fls_match_batch_shared_ivox on a reference-order handle runs as
 * fls_match_batch_fused does for a kind without a shared form (the jobs on n_slots lanes).
 * FLS_IVOX_KNN_ORDER=reference in the environment at fls_create selects the mode for iVox handles.
 *
 * Plain C; no exception crosses the boundary; a handle is not thread-safe.  No call here touches the device.
 * ==========================================================================*/
#ifndef FLS_KNN_ORDER_H
#define FLS_KNN_ORDER_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_KNN_ORDER_REVISION 1

#define FLS_KNN_ORDER_DEFAULT 0   /* (distance bits, map slot): ascending, exact ties to the lower slot */
#define FLS_KNN_ORDER_REFERENCE 1 /* the reference's nth_element order */

int fls_knn_order_revision(void);

/* Selects the order of the Matches that follow (the neighbour lists an earlier Match left stay as they are).  FLS_ERR_INVALID: NULL
 * handle or unknown mode.  FLS_ERR_STATE: FLS_KNN_ORDER_REFERENCE on any kind but FLS_P2PLANE_IVOX (the kd-tree kinds' lists are
 * fully ordered already, NDT has no such order); the handle stays usable.  FLS_KNN_ORDER_DEFAULT is accepted by every kind. */
fls_status fls_set_knn_order(fls_handle h, int mode);

/* *mode = the handle's order.  FLS_ERR_INVALID: NULL handle or NULL mode. */
fls_status fls_get_knn_order(fls_handle h, int* mode);

/* *w = W, the records of one query's work array (a compile-time constant, at least 256).  FLS_ERR_INVALID: NULL w. */
fls_status fls_knn_order_limits(int* w);

#ifdef __cplusplus
}
#endif
#endif
