// abi_debug_fit.hpp -- test hooks (no product path calls them): the device linear algebra (fls_debug_fullpiv_qr6 and fls_debug_ldlt6 of
// fls_reg.h, include/fls_debug_linalg.h), the stages of the fit launch (fls_debug_fit.h), the NDT voxel read-out (fls_debug_ndt.h) and the
// last normal equations of a handle.  The hooks here and in the abi_debug_*.hpp after it name their kernels in the order the code object keeps.
#pragma once
#include "abi_common.hpp"

namespace {

// inputs up, one launch, outputs down: every array holds `w` doubles per system
struct DebugIn { const double* p; int w; };
struct DebugOut { double* p; int w; };
template <typename Launch>
fls_status debug_linalg_run(int device_id, int n, const std::vector<DebugIn>& in, const std::vector<DebugOut>& out, Launch&& launch) {
    for (const DebugIn& a : in) if (!a.p) return FLS_ERR_INVALID;
    for (const DebugOut& a : out) if (!a.p) return FLS_ERR_INVALID;
    if (n < 0) return FLS_ERR_INVALID;
    if (n == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        std::vector<DevBuf<double>> din(in.size()), dout(out.size());
        std::vector<const double*> pin(in.size());
        std::vector<double*> pout(out.size());
        for (size_t i = 0; i < in.size(); ++i) {
            din[i].reserve(size_t(n) * in[i].w);
            FLS_HIP(hipMemcpy(din[i].p, in[i].p, size_t(n) * in[i].w * sizeof(double), hipMemcpyHostToDevice));
            pin[i] = din[i].p;
        }
        for (size_t i = 0; i < out.size(); ++i) { dout[i].reserve(size_t(n) * out[i].w); pout[i] = dout[i].p; }
        launch(pin.data(), pout.data());
        FLS_HIP(hipGetLastError());
        for (size_t i = 0; i < out.size(); ++i) FLS_HIP(hipMemcpy(out[i].p, dout[i].p, size_t(n) * out[i].w * sizeof(double), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}
inline dim3 debug_linalg_lanes(int n) { return dim3(unsigned((n + kDebugLinalgBlock - 1) / kDebugLinalgBlock)); }

}  // namespace

extern "C" {

fls_status fls_debug_fullpiv_qr6(int device_id, const double* H, const double* g, int n, double* x) {
    return debug_linalg_run(device_id, n, {{H, 36}, {g, 6}}, {{x, 6}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_fullpiv_qr6_kernel, dim3(unsigned(n)), dim3(64), 0, nullptr, in[0], in[1], n, out[0]);
    });
}

fls_status fls_debug_ldlt6(int device_id, const double* H, const double* g, int n, double* x, int32_t* ok) {
    if (!ok) return FLS_ERR_INVALID;
    return debug_linalg_run(device_id, n, {{H, 36}, {g, 6}}, {{x, 6}}, [&](const double* const* in, double* const* out) {
        DevBuf<int> dok;  // the one output that is not a double: fetched here, behind the launch on the same (null) stream
        dok.reserve(size_t(n));
        hipLaunchKernelGGL(debug_ldlt6_kernel, dim3(unsigned(n)), dim3(64), 0, nullptr, in[0], in[1], n, out[0], dok.p);
        FLS_HIP(hipMemcpy(ok, dok.p, size_t(n) * sizeof(int), hipMemcpyDeviceToHost));
    });
}

// ---- test hooks of the device linear-algebra primitives (include/fls_debug_linalg.h, kernels_debug_linalg.hpp) --------------------------
int fls_debug_linalg_revision(void) { return FLS_DEBUG_LINALG_REVISION; }

fls_status fls_debug_plane_fit_5x3(int device_id, const double* A, int n, double* x) {
    return debug_linalg_run(device_id, n, {{A, 15}}, {{x, 3}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_plane_fit_5x3_kernel, debug_linalg_lanes(n), dim3(kDebugLinalgBlock), 0, nullptr, in[0], n, out[0]);
    });
}

fls_status fls_debug_svd3(int device_id, const double* A, int n, double* S, double* V) {
    return debug_linalg_run(device_id, n, {{A, 9}}, {{S, 3}, {V, 9}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_svd3_kernel, debug_linalg_lanes(n), dim3(kDebugLinalgBlock), 0, nullptr, in[0], n, out[0], out[1]);
    });
}

fls_status fls_debug_lu6(int device_id, const double* H, const double* b, int n, double* det, double* inv, double* x) {
    return debug_linalg_run(device_id, n, {{H, 36}, {b, 6}}, {{det, 1}, {inv, 36}, {x, 6}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_lu6_kernel, dim3(unsigned(n)), dim3(64), 0, nullptr, in[0], in[1], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_so3(int device_id, const double* v, const double* R, int n, double* Rd, double* R_Rd, double* Rd_R) {
    return debug_linalg_run(device_id, n, {{v, 3}, {R, 9}}, {{Rd, 9}, {R_Rd, 9}, {Rd_R, 9}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_so3_kernel, debug_linalg_lanes(n), dim3(kDebugLinalgBlock), 0, nullptr, in[0], in[1], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_wave_sum(int device_id, const double* v, int n, double* total) {
    return debug_linalg_run(device_id, n, {{v, 64}}, {{total, 1}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_wave_sum_kernel, dim3(unsigned(n)), dim3(64), 0, nullptr, in[0], n, out[0]);
    });
}

// ---- test hooks of the stages of the fit launch (include/fls_debug_fit.h, kernels_debug_fit.hpp) ----------------------------------------
int fls_debug_fit_revision(void) { return FLS_DEBUG_FIT_REVISION; }

fls_status fls_debug_plane_residual(int device_id, const double* nn, const double* ps, const double* pt, const double* T, const double* gate, int n,
                                    double* valid, double* J, double* d) {
    return debug_linalg_run(device_id, n, {{nn, 15}, {ps, 3}, {pt, 3}, {T, 16}, {gate, 1}}, {{valid, 1}, {J, 6}, {d, 1}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_residual_kernel<false>, debug_linalg_lanes(n), dim3(kDebugFitBlock), 0, nullptr, in[0], in[1], in[2], in[3], in[4], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_line_residual(int device_id, const double* nn, const double* ps, const double* pt, const double* T, const double* gate, int n,
                                   double* valid, double* J, double* d) {
    return debug_linalg_run(device_id, n, {{nn, 15}, {ps, 3}, {pt, 3}, {T, 16}, {gate, 1}}, {{valid, 1}, {J, 6}, {d, 1}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_residual_kernel<true>, debug_linalg_lanes(n), dim3(kDebugFitBlock), 0, nullptr, in[0], in[1], in[2], in[3], in[4], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_icp_point_rows(int device_id, const double* T, const double* p, const double* m, int n, double* J, double* e, double* res) {
    return debug_linalg_run(device_id, n, {{T, 16}, {p, 3}, {m, 3}}, {{J, 18}, {e, 3}, {res, 1}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_icp_point_rows_kernel, debug_linalg_lanes(n), dim3(kDebugFitBlock), 0, nullptr, in[0], in[1], in[2], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_rank1_mfma(int device_id, const double* contrib, const double* J, const double* r, int n, double* row) {
    return debug_linalg_run(device_id, n, {{contrib, 64}, {J, 64 * 6}, {r, 64}}, {{row, 32}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_rank1_kernel<0>, dim3(unsigned((n + 3) / 4)), dim3(256), 0, nullptr, in[0], in[1], in[2], n, out[0]);
    });
}

fls_status fls_debug_rank1_dpp(int device_id, const double* contrib, const double* J, const double* r, int n, double* row) {
    return debug_linalg_run(device_id, n, {{contrib, 64}, {J, 64 * 6}, {r, 64}}, {{row, 32}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_rank1_kernel<1>, dim3(unsigned((n + 3) / 4)), dim3(256), 0, nullptr, in[0], in[1], in[2], n, out[0]);
    });
}

fls_status fls_debug_rank1x3_mfma(int device_id, const double* contrib, const double* J, const double* e, int n, double* row) {
    return debug_linalg_run(device_id, n, {{contrib, 64}, {J, 64 * 18}, {e, 64 * 3}}, {{row, 32}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_rank1_kernel<2>, dim3(unsigned((n + 3) / 4)), dim3(256), 0, nullptr, in[0], in[1], in[2], n, out[0]);
    });
}

fls_status fls_debug_reduce_partials(int device_id, int variant, const double* rows, int nrows, double* tot) {
    if (!rows || !tot || nrows < 0 || variant < 0 || variant > 3) return FLS_ERR_INVALID;
    if (nrows == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        // one trip of NaN rows behind the caller's: a load past nrows shows in the totals instead of leaving the allocation
        const size_t pad = size_t(32) * 32;
        std::vector<double> h((size_t(nrows) + pad) * kPartialStride, std::numeric_limits<double>::quiet_NaN());
        std::memcpy(h.data(), rows, size_t(nrows) * kPartialStride * sizeof(double));
        DevBuf<double> drows, dtot;
        drows.reserve(h.size()); dtot.reserve(32);
        FLS_HIP(hipMemcpy(drows.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        const double* r = drows.p;
        if (variant == 0) hipLaunchKernelGGL((debug_reduce_partials_kernel<256, true, 32, LuTailSmem>), dim3(1), dim3(256), 0, nullptr, r, nrows, dtot.p);
        else if (variant == 1) hipLaunchKernelGGL((debug_reduce_partials_kernel<512, true, 16, LoamTailSmem>), dim3(1), dim3(512), 0, nullptr, r, nrows, dtot.p);
        else if (variant == 2) hipLaunchKernelGGL((debug_reduce_partials_kernel<512, true, 32, LuTailSmem>), dim3(1), dim3(512), 0, nullptr, r, nrows, dtot.p);
        else hipLaunchKernelGGL((debug_reduce_partials_kernel<1024, false, 16, LoamTailSmem>), dim3(1), dim3(1024), 0, nullptr, r, nrows, dtot.p);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpy(tot, dtot.p, 32 * sizeof(double), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

fls_status fls_debug_fanin(int device_id, int nblocks, int shards, double* tot, uint32_t* last, uint32_t* ticket) {
    static_assert(FLS_DEBUG_TICKET_WORDS == kTicketWords && kPartialStride == 32, "fls_debug_fit.h states the layout");
    if (!tot || !last || !ticket || nblocks < 1 || nblocks > 65535 || shards < 1) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevBuf<double> dpart, dtot;
        DevBuf<unsigned> dticket, dlast;
        const size_t pad = size_t(32) * 8;  // (NaN rows behind the last one, as in fls_debug_reduce_partials)
        std::vector<double> h((size_t(nblocks) + pad) * kPartialStride, std::numeric_limits<double>::quiet_NaN());
        std::fill(h.begin(), h.begin() + size_t(nblocks) * kPartialStride, 0.0);
        dpart.reserve(h.size()); dtot.reserve(64); dticket.reserve(kTicketWords); dlast.reserve(2);
        FLS_HIP(hipMemcpy(dpart.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        const std::vector<double> canary(64, 7.0);
        FLS_HIP(hipMemcpy(dtot.p, canary.data(), 64 * sizeof(double), hipMemcpyHostToDevice));
        FLS_HIP(hipMemset(dticket.p, 0, kTicketWords * sizeof(unsigned)));
        FLS_HIP(hipMemset(dlast.p, 0, 2 * sizeof(unsigned)));
        for (int k = 0; k < 2; ++k) {
            hipLaunchKernelGGL(debug_fanin_kernel, dim3(unsigned(nblocks)), dim3(256), 0, nullptr, dpart.p, dticket.p, shards, double(k + 1), 1000.0 * k, dlast.p + k,
                               dtot.p + 32 * k);
            FLS_HIP(hipGetLastError());
        }
        FLS_HIP(hipMemcpy(tot, dtot.p, 64 * sizeof(double), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(last, dlast.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(ticket, dticket.p, kTicketWords * sizeof(unsigned), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

// ---- test read-out of the NDT voxel map (include/fls_debug_ndt.h) ----------------------------------------------------------------------
int fls_debug_ndt_revision(void) { return FLS_DEBUG_NDT_REVISION; }

fls_status fls_debug_ndt_voxels(fls_handle h, size_t cap, int32_t* keys, int32_t* vid, int32_t* num_points, uint8_t* estimated, uint8_t* pending,
                                double* mu, double* sigma, double* info, size_t* n) {
    if (!h || !n || h->kind != FLS_INCREMENTAL_NDT) return FLS_ERR_INVALID;
    if (cap && (!keys || !vid || !num_points || !estimated || !pending || !mu || !sigma || !info)) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        NdtMatcher& m = *static_cast<NdtMatcher*>(h);
        if (m.map.on_device()) FLS_HIP(hipSetDevice(h->device));  // (only a map that lives on the device is read from it; the host map needs none)
        *n = m.map.dump_voxels(cap, NdtMap::VoxelDump{keys, vid, num_points, estimated, pending, mu, sigma, info});
        return cap < *n ? FLS_ERR_NOMEM : FLS_OK;
    });
}

fls_status fls_debug_last_system(fls_handle h, double* H36, double* g6) {
    if (!h || !H36 || !g6) return FLS_ERR_INVALID;
    if (!h->d_state.p) return FLS_ERR_STATE;
    return on_device(h, [&] {
        FLS_HIP(hipStreamSynchronize(h->stream));
        FLS_HIP(hipMemcpy(H36, reinterpret_cast<const char*>(h->d_state.p) + offsetof(GnState, H), 36 * sizeof(double), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(g6, reinterpret_cast<const char*>(h->d_state.p) + offsetof(GnState, g), 6 * sizeof(double), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

}  // extern "C"
