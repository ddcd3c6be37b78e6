// abi_debug_tail.hpp -- test hooks of the Gauss-Newton tails (include/fls_debug_tail.h; no product path calls them).  Includes the test kernels
// (kernels_debug_tail.hpp), which this translation unit names last: the code object keeps the order of every kernel in front of them.
#pragma once
#include "abi_common.hpp"
#include "kernels_debug_tail.hpp"
#include "../../include/fls_debug_tail.h"

namespace {

// fls_debug_tail.h states the two layouts: field by field
#define FLS_TAIL_SAME(A, B, f) static_assert(offsetof(A, f) == offsetof(B, f) && sizeof(A::f) == sizeof(B::f), "fls_debug_tail.h states the layout: " #f)
static_assert(sizeof(fls_debug_gn_state) == sizeof(GnState) && alignof(fls_debug_gn_state) == alignof(GnState), "fls_debug_tail.h states the layout");
FLS_TAIL_SAME(fls_debug_gn_state, GnState, T);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, last_rot);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, last_pos);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, sum_res);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, sum_res2);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, last_dx);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, H);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, g);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, iter);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, done);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, converged);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, n_valid);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, n_valid2);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, pad);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, dbg);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, log_T);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, log_res);
FLS_TAIL_SAME(fls_debug_gn_state, GnState, log_nv);
static_assert(sizeof(fls_debug_mailbox) == sizeof(Mailbox) && alignof(fls_debug_mailbox) == alignof(Mailbox), "fls_debug_tail.h states the layout");
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, T);
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, sum_res);
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, sum_res2);
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, last_dx);
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, iter);
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, done);
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, converged);
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, n_valid);
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, n_valid2);
FLS_TAIL_SAME(fls_debug_mailbox, Mailbox, seq);
#undef FLS_TAIL_SAME
static_assert(FLS_DEBUG_TAIL_MAX_ITER == kMaxIter && kPartialStride == 32, "fls_debug_tail.h states the layout");

inline bool debug_tail_rows_ok(const double* rows, int nrows, int least) { return nrows >= least && nrows <= FLS_DEBUG_TAIL_MAX_ROWS && (rows || nrows == 0); }

// the caller's rows on the device, one trip of NaN rows behind them (as fls_debug_reduce_partials); nrows == 0: no buffer, a null pointer
inline const double* debug_tail_rows(DevBuf<double>& d, const double* rows, int nrows) {
    if (nrows == 0) return nullptr;
    const size_t pad = size_t(32) * 32;
    std::vector<double> h((size_t(nrows) + pad) * kPartialStride, std::numeric_limits<double>::quiet_NaN());
    std::memcpy(h.data(), rows, size_t(nrows) * kPartialStride * sizeof(double));
    d.reserve(h.size());
    FLS_HIP(hipMemcpy(d.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    return d.p;
}

// state and mailbox up, launch(GnState*, Mailbox* or null, Pose16), both down whole.  The state's device copy is followed by guard bytes up to
// where the log slots of iteration 255 (the most a LaunchWord allows) would end: a tail that logged without looking at kMaxIter stays inside
// the allocation and the hook reports it.
constexpr size_t kDebugTailStateBytes = offsetof(GnState, log_T) + size_t(LaunchWord::kMaxItLimit + 1) * 16 * sizeof(double);
static_assert(kDebugTailStateBytes > sizeof(GnState), "the guard lies behind the state");
template <typename Launch>
fls_status debug_tail_run(const double* T0, fls_debug_gn_state* state, fls_debug_mailbox* mailbox, Launch&& launch) {
    DevBuf<unsigned char> dst;
    DevBuf<Mailbox> dmb;
    std::vector<unsigned char> h(kDebugTailStateBytes, (unsigned char)FLS_DEBUG_TAIL_GUARD);
    std::memcpy(h.data(), state, sizeof(GnState));
    dst.reserve(h.size());
    FLS_HIP(hipMemcpy(dst.p, h.data(), h.size(), hipMemcpyHostToDevice));
    if (mailbox) {
        dmb.reserve(1);
        FLS_HIP(hipMemcpy(dmb.p, mailbox, sizeof(Mailbox), hipMemcpyHostToDevice));
    }
    Pose16 P;
    std::memcpy(P.m, T0, sizeof(P.m));
    launch(reinterpret_cast<GnState*>(dst.p), mailbox ? dmb.p : nullptr, P);
    FLS_HIP(hipGetLastError());
    FLS_HIP(hipMemcpy(h.data(), dst.p, h.size(), hipMemcpyDeviceToHost));
    std::memcpy(state, h.data(), sizeof(GnState));
    if (mailbox) FLS_HIP(hipMemcpy(mailbox, dmb.p, sizeof(Mailbox), hipMemcpyDeviceToHost));
    for (size_t k = sizeof(GnState); k < h.size(); ++k)
        if (h[k] != (unsigned char)FLS_DEBUG_TAIL_GUARD) return FLS_ERR_RANGE;
    return FLS_OK;
}

}  // namespace

extern "C" {

int fls_debug_tail_revision(void) { return FLS_DEBUG_TAIL_REVISION; }

fls_status fls_debug_loam_tail(int device_id, int variant, int first, const double* T0, fls_debug_gn_state* state, const double* rows_a, int nrows_a,
                               const double* rows_b, int nrows_b, double rot_thr, double pos_thr, uint32_t launch_word, fls_debug_mailbox* mailbox) {
    if (!T0 || !state || !rows_b || variant < 0 || variant > 2) return FLS_ERR_INVALID;
    if (!debug_tail_rows_ok(rows_a, nrows_a, 0) || !debug_tail_rows_ok(rows_b, nrows_b, 1)) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevBuf<double> da, db;
        const double* const pa = debug_tail_rows(da, rows_a, nrows_a);
        const double* const pb = debug_tail_rows(db, rows_b, nrows_b);
        return debug_tail_run(T0, state, mailbox, [&](GnState* st, Mailbox* mb, const Pose16& P) {
            const int f = first ? 1 : 0;
            if (variant == 0)
                hipLaunchKernelGGL(gn_solve_loam_kernel, dim3(1), dim3(kSolveThreads), 0, nullptr, st, f, P, pa, nrows_a, pb, nrows_b, rot_thr, pos_thr, mb,
                                   (unsigned)launch_word);
            else if (variant == 1)
                hipLaunchKernelGGL(debug_loam_tail_kernel<256>, dim3(1), dim3(256), 0, nullptr, st, f, P, pa, nrows_a, pb, nrows_b, rot_thr, pos_thr, mb,
                                   (unsigned)launch_word);
            else
                hipLaunchKernelGGL(debug_loam_tail_kernel<512>, dim3(1), dim3(512), 0, nullptr, st, f, P, pa, nrows_a, pb, nrows_b, rot_thr, pos_thr, mb,
                                   (unsigned)launch_word);
        });
    });
}

fls_status fls_debug_lu_tail(int device_id, int variant, int first, const double* T0, fls_debug_gn_state* state, const double* rows, int nrows, int mode,
                             double rot_thr, double pos_thr, int min_effective, uint32_t launch_word, fls_debug_mailbox* mailbox) {
    if (!T0 || !state || !rows || variant < 0 || variant > 2 || mode < 0 || mode > 1) return FLS_ERR_INVALID;
    if (!debug_tail_rows_ok(rows, nrows, 1)) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevBuf<double> dr;
        const double* const pr = debug_tail_rows(dr, rows, nrows);
        return debug_tail_run(T0, state, mailbox, [&](GnState* st, Mailbox* mb, const Pose16& P) {
            const int f = first ? 1 : 0;
            const LuTailArgs tail{mode, rot_thr, pos_thr, min_effective, mb, (unsigned)launch_word};
            if (variant == 0)
                hipLaunchKernelGGL(gn_solve_lu_kernel, dim3(1), dim3(kSolveThreads), 0, nullptr, st, f, P, pr, nrows, mode, rot_thr, pos_thr, min_effective, mb,
                                   (unsigned)launch_word);
            else if (variant == 1)
                hipLaunchKernelGGL(debug_lu_tail_kernel<256>, dim3(1), dim3(256), 0, nullptr, st, f, P, pr, nrows, tail);
            else
                hipLaunchKernelGGL(debug_lu_tail_kernel<512>, dim3(1), dim3(512), 0, nullptr, st, f, P, pr, nrows, tail);
        });
    });
}

}  // extern "C"
