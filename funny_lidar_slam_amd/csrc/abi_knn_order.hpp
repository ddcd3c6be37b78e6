// abi_knn_order.hpp -- include/fls_knn_order.h: the neighbour order of the iVox point-to-plane kind.  Host code only; no call touches the device.
// Includes the reference-order kernel and its launch (kernels_ivox_knn_reforder.hpp), which this translation unit names last.
#pragma once
#include "abi_common.hpp"
#include "kernels_ivox_knn_reforder.hpp"

extern "C" {

int fls_knn_order_revision(void) { return FLS_KNN_ORDER_REVISION; }

fls_status fls_set_knn_order(fls_handle h, int mode) {
    if (!h || (mode != FLS_KNN_ORDER_DEFAULT && mode != FLS_KNN_ORDER_REFERENCE)) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { return h->set_knn_order(mode); });
}

fls_status fls_get_knn_order(fls_handle h, int* mode) {
    if (!h || !mode) return FLS_ERR_INVALID;
    *mode = h->knn_order();
    return FLS_OK;
}

fls_status fls_knn_order_limits(int* w) {
    if (!w) return FLS_ERR_INVALID;
    *w = kro::kWork;
    return FLS_OK;
}

}  // extern "C"
