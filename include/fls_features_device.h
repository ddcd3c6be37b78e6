/* ============================================================================
 * fls_features_device.h -- the LOAM feature clouds kept on the device between the front end (include/fls_features.h) and Match of the
 * LoamFull kind (include/fls_reg.h).  Same shared library (libfls_reg.so); FLS_ABI_REVISION is unchanged, this header carries a
 * revision of its own.
 *
 * Default (a handle never switched on): fls_features_project* / fls_features_extract behave as fls_features.h describes -- every array
 * is downloaded eagerly, the clouds are gathered and voxel-filtered on the host.
 *
 * fls_features_keep_on_device(h, 1): from the next projection on
 *   - the projection brings back the ordered count alone; ordered cloud, depths, columns and the ring start / end indices stay in
 *     device memory;
 *   - fls_features_extract runs one more launch that gathers corner_cloud_ / planar_cloud_ (x | y | z | intensity planes and the
 *     ordered indices) from the per-ring selection lists, brings back the two sizes in one wait, and runs the two VoxelGrid filters
 *     (preprocessing.cpp:234-237) on the device, bit-identical to the host filter.  A filter the device declines (PCL's "leaf size too
 *     small" case, a cloud too large) takes the host filter for that cloud; its result is uploaded so that an attach still works;
 *   - fls_features_get downloads (or reconstructs) an array on its first request and keeps it until the next projection / extraction:
 *     every array equals what the default mode returns.
 *
 * fls_scan_attach_features hands the two clouds to a LoamFull handle device to device: afterwards the handle is in the state
 * fls_scan_upload(m, planar rows, np, corner rows, nc, 4) leaves it in, and fls_match_resident runs on it.  The copy is queued on the
 * matcher's stream behind the extraction (hipEvents, no host wait); the front end's next projection is queued behind the copy.
 * Plain C; no exception crosses the boundary; a handle is not thread-safe.
 * ==========================================================================*/
#ifndef FLS_FEATURES_DEVICE_H
#define FLS_FEATURES_DEVICE_H
#include "fls_features.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_FEATURES_DEVICE_REVISION 1

/* counters of fls_features_stat (since the handle was created) */
enum {
    FLS_FEAT_STAT_DEVICE_GATHERS = 0,   /* extractions whose clouds were gathered on the device               */
    FLS_FEAT_STAT_DEVICE_FILTERS = 1,   /* VoxelGrid filters run on the device                                 */
    FLS_FEAT_STAT_FILTER_DECLINES = 2,  /* VoxelGrid filters the device declined (host filter, result uploaded) */
    FLS_FEAT_STAT_LAZY_DOWNLOADS = 3    /* arrays downloaded because fls_features_get asked for them           */
};

int fls_features_device_revision(void);
/* on != 0: keep the arrays on the device from the next projection on; 0: the default.  A call that changes the mode withdraws the
 * current projection (fls_features_extract answers FLS_ERR_STATE until the next one). */
fls_status fls_features_keep_on_device(fls_features_handle h, int on);
/* bytes copied device -> host on behalf of the last frame so far (projection, extraction, and every download fls_features_get caused).
 * Not counted: the host-mapped mailbox through which each device VoxelGrid publishes its output size (one more host wait per filter). */
fls_status fls_features_get_host_bytes(fls_features_handle h, uint64_t* d2h_bytes);
size_t fls_features_stat(fls_features_handle h, int what);
/* filtered != 0: FLS_FEAT_PLANAR_FILTERED + FLS_FEAT_CORNER_FILTERED (what the reference hands to Match); 0: the unfiltered pair.
 * Works after an extraction in either mode (default mode: the clouds are uploaded from the handle's host copies).
 * FLS_ERR_STATE: no completed extraction, filtered with a leaf of 0, `m` is not FLS_LOAM_FULL.  FLS_ERR_INVALID: a NULL handle, handles
 * on different devices.  On any error `m` keeps its resident scan. */
fls_status fls_scan_attach_features(fls_handle m, fls_features_handle f, int filtered);

#ifdef __cplusplus
}
#endif
#endif
