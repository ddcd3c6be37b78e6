// abi_debug_ivox_update.hpp -- include/fls_debug_ivox_update.h: one decided batch through the iVox map update (P2PlaneIvoxMatcher::debug_add_points,
// which shares apply_decided with the Match path).  Names no kernel that the map itself has not named.
#pragma once
#include "abi_common.hpp"
#include "../../include/fls_debug_ivox_update.h"

extern "C" {

int fls_debug_ivox_update_revision(void) { return FLS_DEBUG_IVOX_UPDATE_REVISION; }

fls_status fls_debug_ivox_add_points(fls_handle h, const float* world_xyz, const uint8_t* code, size_t n, uint32_t* device_status) {
    if (!h || !device_status || (n && (!world_xyz || !code)) || h->kind != FLS_P2PLANE_IVOX) return FLS_ERR_INVALID;
    for (size_t i = 0; i < n; ++i)
        if (code[i] > 2) return FLS_ERR_INVALID;
    P2PlaneIvoxMatcher& m = *static_cast<P2PlaneIvoxMatcher*>(h);
    if (m.borrowed || m.map.is_replica() || m.p.is_localization_mode || m.map.is_first) return FLS_ERR_STATE;
    return on_device(h, [&] {
        unsigned st = 0xFFFFFFFFu;
        const fls_status rc = m.debug_add_points(world_xyz, code, n, &st);
        *device_status = st;
        return rc;
    });
}

}  // extern "C"
