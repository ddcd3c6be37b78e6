// kernels_debug_tail.hpp -- test kernels of include/fls_debug_tail.h: loam_tail<NT, true> and lu_tail<NT, true>, the instantiations of the fused
// launches, as ONE workgroup on caller-supplied rows.  Each kernel loads the state words the way the fused kernels do (p2plane_fit_solve_body,
// icp_knn_fit_body, ndt_lanes_kernel), returns when the Match is done and hands the tail the product's own LDS struct.  The 1024-thread
// instantiations are the product kernels gn_solve_loam_kernel / gn_solve_lu_kernel themselves: the hooks launch those.
// tests/test_gpu_tails.py compares every word of GnState and of the mailbox with the model of tests/tail_cases.py.
// Named LAST in the translation unit (fls_reg.hip), so that the code object keeps the order of every kernel in front of these.
#pragma once
#include "kernels_p2plane.hpp"
#include "kernels_knn.hpp"

namespace fls {

template <int NT>
__global__ void __launch_bounds__(NT)
debug_loam_tail_kernel(GnState* __restrict__ st, const int first, const Pose16 T0, const double* __restrict__ partials_a, const int nrows_a,
                       const double* __restrict__ partials_b, const int nrows_b, const double rot_thr, const double pos_thr, Mailbox* __restrict__ mb,
                       const unsigned match_id) {
    const int done = first ? 0 : st->done;
    double T44[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) T44[k] = first ? T0.m[k] : st->T[k];
    const double last_rot = first ? 0.0 : st->last_rot, last_pos = first ? 0.0 : st->last_pos;
    const int it = first ? 0 : st->iter;
    if (done) return;
    __shared__ LoamTailSmem sm;
    loam_tail<NT, true>(st, sm, partials_a, nrows_a, partials_b, nrows_b, rot_thr, pos_thr, T44, last_rot, last_pos, it, mb, match_id);
}

template <int NT>
__global__ void __launch_bounds__(NT)
debug_lu_tail_kernel(GnState* __restrict__ st, const int first, const Pose16 T0, const double* __restrict__ partials, const int nrows, const LuTailArgs tail) {
    const int done = first ? 0 : st->done;
    double T[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) T[k] = first ? T0.m[k] : st->T[k];
    const int it = first ? 0 : st->iter;
    if (done) return;
    __shared__ LuTailSmem sm;
    lu_tail<NT, true>(st, sm, partials, nrows, tail, T, it);
}

}  // namespace fls
