/* ============================================================================
 * fls_debug_ivox_update.h -- test-only entry point of the iVox map update (csrc/kernels_ivox_update.hpp, csrc/ivox_map.hpp; same shared library
 * as fls_reg.h, FLS_ABI_REVISION stays 9: this header has a revision of its own).
 *
 * fls_match(update_map = 1) decides on the device which points of the matched scan go into the map (code 1: points_to_add, code 2:
 * point_no_need_downsample, code 0: dropped) and applies that batch: on the device while the device holds the map, on the host mirror otherwise
 * and whenever the device refuses the batch.  fls_debug_ivox_add_points applies a batch the CALLER has decided, through the same code: the
 * product's choice of the short or the long launch chain, its verdict, its fall-back to the sequential host replay.
 * ==========================================================================*/
#ifndef FLS_DEBUG_IVOX_UPDATE_H
#define FLS_DEBUG_IVOX_UPDATE_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_DEBUG_IVOX_UPDATE_REVISION 1

int fls_debug_ivox_update_revision(void);

/* One decided batch into the map of an FLS_P2PLANE_IVOX handle in mapping mode: world_xyz [n][3] world points, code [n] their insertion codes
 * (0 drop, 1 points_to_add, 2 point_no_need_downsample).  The code-1 points are inserted in source order, then the code-2 points (intensity 0).
 * *device_status: the status word the batch's device chain published (0: applied; a bit set: refused, see kUpd* in csrc/kernels_ivox_update.hpp),
 * 0xFFFFFFFF when no device chain ran (the host holds the map, or n is beyond the chain's 262,144 points).
 * Checked before the device is looked at -- FLS_ERR_INVALID: NULL handle, NULL arrays with n > 0, NULL device_status, a code above 2, a handle
 * of another kind; FLS_ERR_STATE: a replica, a localization-mode handle, a handle that has not taken its first cloud.
 * Returns what the product path returns: FLS_OK, or FLS_ERR_RANGE from the host replay of a key beyond the limit (each of the two lists is
 * all-or-nothing: a bad code-2 point leaves the code-1 points inserted, a bad code-1 point leaves the map unchanged). */
fls_status fls_debug_ivox_add_points(fls_handle h, const float* world_xyz, const uint8_t* code, size_t n, uint32_t* device_status);

#ifdef __cplusplus
}
#endif
#endif
