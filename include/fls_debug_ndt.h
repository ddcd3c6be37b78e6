/* ============================================================================
 * fls_debug_ndt.h -- test-only read-out of the voxel map of an FLS_INCREMENTAL_NDT handle (same shared library as fls_reg.h;
 * FLS_ABI_REVISION stays 9, this header has a revision of its own, like fls_debug_fit.h).  This is what lets a test compare the voxel
 * statistics of two handles, or of a handle and the CPU oracle, array by array (the map itself travels as the image of fls_map_ndt.h).
 * ==========================================================================*/
#ifndef FLS_DEBUG_NDT_H
#define FLS_DEBUG_NDT_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_NDT_REVISION 1

int fls_debug_ndt_revision(void);

/* Every alive voxel of the handle's map in LRU order, most recently touched first: keys[n][3] voxel key, vid[n] voxel id (creation order, the
 * correspondence id), num_points[n], estimated[n] (0 / 1), pending[n] (points waiting for the next estimate, at most 8; 0 in a voxel beyond
 * ndt_max_points_in_voxel), mu[n][3], sigma[n][9] and info[n][9] (column-major).  *n receives the number of alive voxels.  A handle whose
 * map is held by the device is read by downloading its rows and ordering them by their LRU stamps, any other from the host mirror; the call
 * changes no state and no counter and does not move the map.
 * FLS_ERR_INVALID, checked before the device is looked at: a NULL handle or n, a handle of another kind, a NULL array with cap > 0.  With
 * cap smaller than the number of voxels nothing is written but *n, and the call returns FLS_ERR_NOMEM (cap == 0 with NULL arrays asks for
 * the size). */
fls_status fls_debug_ndt_voxels(fls_handle h, size_t cap, int32_t* keys, int32_t* vid, int32_t* num_points, uint8_t* estimated, uint8_t* pending,
                                double* mu, double* sigma, double* info, size_t* n);

#ifdef __cplusplus
}
#endif
#endif
