/* ============================================================================
 * fls_debug_ivox_knn.h -- test-only entry point of the iVox kNN kernel's shared-run path (csrc/kernels_ivox_coop.hpp; same shared library as
 * fls_reg.h, FLS_ABI_REVISION stays 9, fls_debug_knn.h stays at its revision 1 with its four symbols: this header has a revision of its own).
 *
 * A wave of ivox_knn_kernel / ivox_knn_jobs_kernel (brick image, not the general form) takes the shared-run path when its 16 queries form at most
 * r_max runs of equal (voxel key, brick present) and the 19-voxel neighbourhoods of those runs hold at most cap map points together.  Tests read
 * the two limits here instead of copying them.  How many waves of a counting Match (fls_set_profiling bit 1) took the path: fls_map_size slot 176.
 * ==========================================================================*/
#ifndef FLS_DEBUG_IVOX_KNN_H
#define FLS_DEBUG_IVOX_KNN_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_IVOX_KNN_REVISION 1

int fls_debug_ivox_knn_revision(void);

/* The gate's limits as compiled.  FLS_ERR_INVALID on a NULL pointer (nothing is written); needs no device. */
fls_status fls_debug_ivox_knn_limits(int* r_max, int* cap);

#ifdef __cplusplus
}
#endif
#endif
