// abi_debug_ivox_decide.hpp -- include/fls_debug_ivox_decide.h: the map-update decision launch, the list materialization and the host rule of
// FLS_P2PLANE_IVOX on caller-supplied arrays, through the functions the matcher itself goes through (launch_add_decide, launch_nn_materialize,
// ivox_decide_host of matcher_p2plane_ivox.hpp).  Names no kernel that the matcher has not named.
#pragma once
#include "abi_common.hpp"
#include "../../include/fls_debug_ivox_decide.h"

namespace {

template <class T>
void debug_decide_alloc_filled(DevBuf<T>& b, const size_t n) {
    b.reserve(n ? n : 1);
    FLS_HIP(hipMemset(b.p, FLS_DEBUG_IVOX_DECIDE_FILL, (n ? n : 1) * sizeof(T)));
}
template <class T, class S>
void debug_decide_upload(DevBuf<T>& b, const S* src, const size_t bytes) {
    if (bytes) FLS_HIP(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
}
// the caller's map rows with FLS_DEBUG_IVOX_DECIDE_MAP_PAD sentinel rows behind them
void debug_decide_map(DevBuf<float4>& d_map, const float* map_rows, const int n_slots, const float* sentinel) {
    const size_t rows = size_t(n_slots) + FLS_DEBUG_IVOX_DECIDE_MAP_PAD;
    std::vector<float> h(rows * 4);
    if (n_slots) std::memcpy(h.data(), map_rows, size_t(n_slots) * 4 * sizeof(float));
    for (size_t r = size_t(n_slots); r < rows; ++r) std::memcpy(&h[r * 4], sentinel, 4 * sizeof(float));
    d_map.reserve(rows);
    FLS_HIP(hipMemcpy(d_map.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
}
// the three list arrays, `cap` (>= nn_n) entries each; what lies behind nn_n is the fill
struct DebugLists {
    DevBuf<float4> rows;
    DevBuf<unsigned char> cnt;
    DevBuf<unsigned> ids;
    void upload(const float* nn_rows, const uint8_t* nn_cnt, const uint32_t* nn_ids, const size_t nn_n, const size_t cap) {
        debug_decide_alloc_filled(rows, cap * 5);
        debug_decide_alloc_filled(cnt, cap);
        debug_decide_upload(rows, nn_rows, nn_n * 5 * sizeof(float4));
        debug_decide_upload(cnt, nn_cnt, nn_n);
        if (nn_ids) {
            debug_decide_alloc_filled(ids, cap * 8);
            debug_decide_upload(ids, nn_ids, nn_n * 8 * sizeof(unsigned));
        }
    }
    void download(float* nn_rows, uint8_t* nn_cnt, const size_t nn_n) {
        if (!nn_n) return;
        FLS_HIP(hipMemcpy(nn_rows, rows.p, nn_n * 5 * sizeof(float4), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(nn_cnt, cnt.p, nn_n, hipMemcpyDeviceToHost));
    }
};

}  // namespace

extern "C" {

int fls_debug_ivox_decide_revision(void) { return FLS_DEBUG_IVOX_DECIDE_REVISION; }

fls_status fls_debug_ivox_decide(int device_id, const float* src_xyz, int n, const double* T, double fs, float* nn_rows, uint8_t* nn_cnt, int nn_n,
                                 const uint32_t* nn_ids, const float* map_rows, int n_slots, const float* sentinel, int materialize, int count,
                                 const fls_debug_ivox_gate* gate, uint8_t* code, float* pw, uint32_t* lx, uint32_t* bt, uint32_t* status) {
    if (n < 0 || nn_n < 0 || n_slots < 0 || (materialize != 0 && materialize != 1) || (count != 0 && count != 1)) return FLS_ERR_INVALID;
    if (!src_xyz || !T || !sentinel || !code || !pw) return FLS_ERR_INVALID;
    if (nn_n && (!nn_rows || !nn_cnt)) return FLS_ERR_INVALID;
    if (n_slots && !map_rows) return FLS_ERR_INVALID;
    if (count && (!lx || !bt || !status)) return FLS_ERR_INVALID;
    if (gate && !count) return FLS_ERR_INVALID;  // (a launch that skips writes the status words, which are null without counting)
    for (int i = 0; !nn_ids && i < nn_n; ++i)
        if (!(nn_cnt[i] & 0x80) && (nn_cnt[i] & 7)) return FLS_ERR_INVALID;  // an ids-form list without ids
    if (n == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        const size_t N = size_t(n), NN = size_t(nn_n), m = materialize ? std::max(N, NN) : N, nblocks = (m + 255) / 256;
        std::vector<float> planes(3 * N);  // x | y | z, as DevScan keeps the scan
        for (size_t i = 0; i < N; ++i)
            for (int a = 0; a < 3; ++a) planes[size_t(a) * N + i] = src_xyz[3 * i + size_t(a)];
        DevBuf<float> d_src;
        d_src.reserve(3 * N);
        debug_decide_upload(d_src, planes.data(), planes.size() * sizeof(float));
        DebugLists lists;
        lists.upload(nn_rows, nn_cnt, nn_ids, NN, std::max(m, NN));
        DevBuf<float4> d_map, d_pw;
        debug_decide_map(d_map, map_rows, n_slots, sentinel);
        DevBuf<unsigned char> d_code;
        DevBuf<uint2> d_lx, d_bt;
        DevBuf<unsigned> d_status;
        DevBuf<GnState> d_gn;
        debug_decide_alloc_filled(d_code, N);
        debug_decide_alloc_filled(d_pw, N);
        debug_decide_alloc_filled(d_lx, N);
        debug_decide_alloc_filled(d_bt, nblocks);
        debug_decide_alloc_filled(d_status, 2);
        if (gate) {
            std::vector<GnState> g(1);
            std::memset(static_cast<void*>(g.data()), 0, sizeof(GnState));
            g[0].done = gate->done; g[0].iter = gate->iter; g[0].n_valid = gate->n_valid;
            std::memcpy(g[0].T, gate->T, sizeof(g[0].T));
            d_gn.reserve(1);
            debug_decide_upload(d_gn, g.data(), sizeof(GnState));
        }
        launch_add_decide(DecideLaunch{d_src.p, d_src.p + N, d_src.p + 2 * N, N, T, lists.rows.p, lists.cnt.p, NN, fs, d_code.p, d_pw.p, nn_ids ? lists.ids.p : nullptr,
                                       d_map.p, unsigned(n_slots), count ? d_lx.p : nullptr, count ? d_bt.p : nullptr, count ? d_status.p : nullptr,
                                       count ? d_status.p + 1 : nullptr, gate ? d_gn.p : nullptr, gate ? int(gate->max_iterations) : 0, materialize != 0},
                          nullptr);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipDeviceSynchronize());
        lists.download(nn_rows, nn_cnt, NN);
        FLS_HIP(hipMemcpy(code, d_code.p, N, hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(pw, d_pw.p, N * sizeof(float4), hipMemcpyDeviceToHost));
        if (lx) FLS_HIP(hipMemcpy(lx, d_lx.p, N * sizeof(uint2), hipMemcpyDeviceToHost));
        if (bt) FLS_HIP(hipMemcpy(bt, d_bt.p, nblocks * sizeof(uint2), hipMemcpyDeviceToHost));
        if (status) FLS_HIP(hipMemcpy(status, d_status.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

fls_status fls_debug_ivox_nn_materialize(int device_id, const uint32_t* nn_ids, uint8_t* nn_cnt, int nn_n, const float* map_rows, int n_slots,
                                         const float* sentinel, float* nn_rows) {
    if (nn_n < 0 || n_slots < 0 || !nn_ids || !nn_cnt || !nn_rows || !sentinel || (n_slots && !map_rows)) return FLS_ERR_INVALID;
    if (nn_n == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        const size_t NN = size_t(nn_n);
        DebugLists lists;
        lists.upload(nn_rows, nn_cnt, nn_ids, NN, NN);
        DevBuf<float4> d_map;
        debug_decide_map(d_map, map_rows, n_slots, sentinel);
        launch_nn_materialize(lists.ids.p, lists.cnt.p, NN, d_map.p, unsigned(n_slots), lists.rows.p, nullptr);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipDeviceSynchronize());
        lists.download(nn_rows, nn_cnt, NN);
        return FLS_OK;
    });
}

fls_status fls_debug_ivox_decide_host(const float* src_xyz, const double* T, double fs, const float* nn, const uint8_t* cnt, int n, uint8_t* code, float* pw) {
    if (!src_xyz || !T || !nn || !cnt || !code || !pw || n < 0) return FLS_ERR_INVALID;
    if (n == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        ivox_decide_host(src_xyz, 3, size_t(n), T, fs, nn, 3, cnt, size_t(n), code, pw);
        return FLS_OK;
    });
}

}  // extern "C"
