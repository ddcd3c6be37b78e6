// kernels_loop_leaves.hpp -- the leaf Gaussians of an NDT stage's target built on the device: what LoopMatcher::build_target computes
// (VoxelGridCovariance, leaf = resolution, >= 6 points per leaf, eigenvalue floor 0.01), with the same bits, from a filtered target that
// never left the device; and loop_moved_kernel, GICP's `output` cloud.  Driver: LoopMatcher::build_target_device, below.
//
//   bounds      vg_minmax (kernels_voxelgrid.hpp: integer atomics on order-encoded floats; min and max do not depend on an order), read by
//               the host, which evaluates build_target's own expressions: dx * dy * dz > INT_MAX -> no leaves, min_b, div_b, dense or sparse
//   leaf_keys   cell of a point: int(floorf(x * inv) - float(min_b)) per axis, i0 + i1 * m1 + i2 * m2; a non-finite point (or a cell outside
//               the box, which the host build would index out of bounds with) gets the sentinel `total` and is sorted behind every leaf
//   sort        {cell, point index} through the stable DevicePairSort: ascending cell, a cell's points in cloud order
//   leaf_heads  segment heads; a head whose segment holds six points or more (key[e + 5] is still its cell) counts, and the exclusive
//               scan of those counts (block-local here, the block totals through vg_scan) is the row = the rank among the leaves of
//               >= 6 points in ascending cell index: build_target's emission order
//   leaf_stats  one lane per counted head walks its segment: double sum[3], xx[9], float csum[3] in cloud order as build_target's
//               accumulate does, then loop::leaf_gaussian (loop_optim.hpp) -- the function build_target calls -- and the rows of mean / icov /
//               centroid, the cell and the point count; leaf_row[cell] = row (dense), or the open-addressing {cell, row} table (sparse)
// ORDER: every floating-point sum is one lane's sequential chain over a stably sorted segment: no floating-point atomics anywhere, the
// result does not depend on the launch geometry.  The sparse table is filled with integer compare-and-swap: a cell's SLOT depends on the
// order the lanes arrive in (the host's on insertion order), what ndt_leaf_row returns for a cell does not -- cells are unique, the table
// is at most half full.  The sparse form is built here, not declined.
// Declined (the caller takes build_target on a downloaded copy): more than 4,194,304 points, a box of INT_MAX cells or more.
// Two short host waits per build: the bounds, and the leaf count.  Included last (fls_reg.hip), like kernels_ivox_knn_reforder.hpp; the
// kernels are templates (block size, table form) because the code object lists plain kernels in front of every instantiated one: as
// templates instantiated here they come behind the kernels of the registration paths, whose addresses stay what they were.
#pragma once
#include "loop_closure.hpp"

namespace fls {

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
leaf_keys(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const int n, const VgGrid g,
          unsigned* __restrict__ key, unsigned* __restrict__ val) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float px = x[i], py = y[i], pz = z[i];
    unsigned k = g.total;
    if (vg_finite3(px, py, pz)) {
        const int i0 = (int)(floorf(px * g.inv) - (float)g.min_b[0]);
        const int i1 = (int)(floorf(py * g.inv) - (float)g.min_b[1]);
        const int i2 = (int)(floorf(pz * g.inv) - (float)g.min_b[2]);
        k = (unsigned)(i0 + i1 * g.m1 + i2 * g.m2);
        if (k > g.total) k = g.total;
    }
    key[i] = k;
    val[i] = (unsigned)i;
}

// lx[e]: block-local exclusive rank of a head of >= 6 points among such heads, ~0u for every other position; bt[block]: their number
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
leaf_heads(const unsigned* __restrict__ key, const int n, const unsigned total, unsigned* __restrict__ lx, unsigned* __restrict__ bt) {
    __shared__ unsigned wsum[BLOCK / 64];
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    unsigned head = 0u;
    if (e < n) {
        const unsigned k = key[e];
        head = (k < total && (e == 0 || key[e - 1] != k) && e + 5 < n && key[e + 5] == k) ? 1u : 0u;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = head;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned base = 0u, tot = 0u;
    for (int q = 0; q < BLOCK / 64; ++q) { const unsigned t = wsum[q]; if (q < w) base += t; tot += t; }
    if (e < n) lx[e] = head ? (base + inc - 1u) : 0xffffffffu;
    if (threadIdx.x == 0) bt[blockIdx.x] = tot;
}

struct LeafOut {
    double* mean;      // [rows][3]
    double* icov;      // [rows][9]
    float* centroid;   // [rows][3]
    int* row_cell;     // [rows]
    int* row_n;        // [rows]
    int* leaf_row;     // dense (SPARSE = false): [total], filled with -1
    int2* leaf_hash;   // sparse: [hash_mask + 1], filled with {-1, -1}
    unsigned hash_mask;
    unsigned row_cap;  // rows the arrays hold (n / 6 at least: a guard, never reached)
};

template <bool SPARSE>
__global__ void __launch_bounds__(kVgBlock)
leaf_stats(const unsigned* __restrict__ key, const unsigned* __restrict__ val, const int n, const float* __restrict__ x, const float* __restrict__ y,
           const float* __restrict__ z, const unsigned* __restrict__ lx, const unsigned* __restrict__ bt /* scanned */, const LeafOut o) {
    const int e = blockIdx.x * kVgBlock + threadIdx.x;
    if (e >= n) return;
    const unsigned l = lx[e];
    if (l == 0xffffffffu) return;
    const unsigned row = bt[e / kVgScanBlock] + l;
    if (row >= o.row_cap) return;
    const unsigned k = key[e];
    double sum[3] = {0.0, 0.0, 0.0}, xx[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    float csum[3] = {0.f, 0.f, 0.f};
    int cnt = 0;
    for (int q = e; q < n && key[q] == k; ++q) {  // LoopMatcher::build_target's accumulate, the segment in cloud order
        const unsigned p = val[q];
        const float pf[3] = {x[p], y[p], z[p]};
        const double pd[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) sum[a] += pd[a];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) xx[r + 3 * c] += pd[r] * pd[c];
        csum[0] += pf[0]; csum[1] += pf[1]; csum[2] += pf[2];
        ++cnt;
    }
    double mean[3], icov[9];
    loop::leaf_gaussian(cnt, sum, xx, mean, icov);
#pragma unroll
    for (int a = 0; a < 3; ++a) { o.mean[3 * (size_t)row + a] = mean[a]; o.centroid[3 * (size_t)row + a] = csum[a] / (float)cnt; }
#pragma unroll
    for (int a = 0; a < 9; ++a) o.icov[9 * (size_t)row + a] = icov[a];
    o.row_cell[row] = (int)k;
    o.row_n[row] = cnt;
    if (!SPARSE) { o.leaf_row[k] = (int)row; return; }
    for (unsigned h = (k * 2654435761u) & o.hash_mask;; h = (h + 1u) & o.hash_mask) {  // (= LoopMatcher::leaf_hash_of, ndt_leaf_row's probe order)
        if (atomicCAS(&o.leaf_hash[h].x, -1, (int)k) == -1) { o.leaf_hash[h].y = (int)row; return; }
    }
}

// GICP's `output`: the filtered source moved by the guess, with the function the host entry's loop calls
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
loop_moved_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const int n, const LoopMat4f T,
                  float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float o[3];
    loop_xform(T, x[i], y[i], z[i], o);
    ox[i] = o[0]; oy[i] = o[1]; oz[i] = o[2];
}

inline LoopMatcher::LeafBuild LoopMatcher::build_target_device(const float* x, const float* y, const float* z, const size_t n, const float resolution,
                                                               TargetLeaves& tl) {
    tl.rows = 0;
    tl.rows_on_host = false;
    tl.inv = 1.0f / resolution;
    const float inv = tl.inv;
    if (n == 0) return kLeavesNone;
    if (n > size_t(kVgMaxBlocks) * kVgTile) return kLeavesDeclined;
    // ---- bounds of the finite points -> the host, which decides as build_target does ------------------------------------------------
    h_leaf_hdr.reserve(2);
    d_leaf_hdr.reserve(1);
    for (int a = 0; a < 3; ++a) { h_leaf_hdr.p[0].mn[a] = 0xffffffffu; h_leaf_hdr.p[0].mx[a] = 0u; }
    h_leaf_hdr.p[0].n_out = 0u; h_leaf_hdr.p[0].n_bad = 0u;
    FLS_HIP(hipMemcpyAsync(d_leaf_hdr.p, &h_leaf_hdr.p[0], sizeof(VgHeader), hipMemcpyHostToDevice, stream));
    const int ni = int(n), nb1 = (ni + kVgBlock - 1) / kVgBlock, nb2 = (ni + kVgScanBlock - 1) / kVgScanBlock;
    hipLaunchKernelGGL(vg_minmax, dim3(unsigned(std::min(nb1, minmax_blocks(n)))), dim3(kVgBlock), 0, stream, x, y, z, ni, d_leaf_hdr.p);
    FLS_HIP(hipGetLastError());
    FLS_HIP(hipMemcpyAsync(&h_leaf_hdr.p[1], d_leaf_hdr.p, sizeof(VgHeader), hipMemcpyDeviceToHost, stream));
    FLS_HIP(hipStreamSynchronize(stream));
    const VgHeader hh = h_leaf_hdr.p[1];
    if (hh.mn[0] == 0xffffffffu) return kLeavesNone;  // no finite point
    float mn[3], mx[3];
    for (int a = 0; a < 3; ++a) { mn[a] = vg_unord(hh.mn[a]); mx[a] = vg_unord(hh.mx[a]); }
    const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1, dy = (long long)((mx[1] - mn[1]) * inv) + 1, dz = (long long)((mx[2] - mn[2]) * inv) + 1;
    if (dx * dy * dz > (long long)INT_MAX) return kLeavesNone;
    for (int a = 0; a < 3; ++a) { tl.min_b[a] = int(std::floor(mn[a] * inv)); tl.div_b[a] = int(std::floor(mx[a] * inv)) - tl.min_b[a] + 1; }
    if (tl.div_b[0] <= 0 || tl.div_b[1] <= 0 || tl.div_b[2] <= 0) return kLeavesDeclined;
    const size_t n_cells = size_t(tl.div_b[0]) * tl.div_b[1] * tl.div_b[2];
    if (n_cells >= size_t(INT_MAX)) return kLeavesDeclined;
    tl.sparse = n_cells > kMaxDenseLeafCells;
    VgGrid g;
    g.inv = inv;
    for (int a = 0; a < 3; ++a) g.min_b[a] = tl.min_b[a];
    g.m1 = tl.div_b[0];
    g.m2 = tl.div_b[0] * tl.div_b[1];
    g.total = unsigned(n_cells);
    // ---- tables and rows -----------------------------------------------------------------------------------------------------------
    const size_t row_cap = n / 6 + 1;
    tl.d_mean.reserve(3 * row_cap); tl.d_icov.reserve(9 * row_cap); tl.d_centroid.reserve(3 * row_cap);
    tl.d_row_cell.reserve(row_cap); tl.d_row_n.reserve(row_cap);
    shrink_if_oversized(tl.d_leaf_row, tl.sparse ? size_t(0) : n_cells);
    LeafOut o{tl.d_mean.p, tl.d_icov.p, tl.d_centroid.p, tl.d_row_cell.p, tl.d_row_n.p, nullptr, nullptr, 0u, unsigned(row_cap)};
    if (!tl.sparse) {
        tl.d_leaf_row.reserve(n_cells);
        FLS_HIP(hipMemsetAsync(tl.d_leaf_row.p, 0xff, n_cells * sizeof(int), stream));
        o.leaf_row = tl.d_leaf_row.p;
    } else {
        size_t hs = 1024;
        while (hs < 2 * n + 2) hs <<= 1;  // (occupied cells <= points: at most half full)
        tl.hash_mask = unsigned(hs - 1);
        tl.d_leaf_hash.reserve(hs);
        FLS_HIP(hipMemsetAsync(tl.d_leaf_hash.p, 0xff, hs * sizeof(int2), stream));
        o.leaf_hash = tl.d_leaf_hash.p;
        o.hash_mask = tl.hash_mask;
    }
    // ---- {cell, point} pairs, sorted; heads; rows ----------------------------------------------------------------------------------
    leaf_sort.prepare(n);
    d_leaf_lx.reserve(n);
    d_leaf_bt.reserve(size_t(2 * nb2));
    hipLaunchKernelGGL(leaf_keys<kVgBlock>, dim3(unsigned(nb1)), dim3(kVgBlock), 0, stream, x, y, z, ni, g, leaf_sort.k0, leaf_sort.v0);
    leaf_sort.run(DevicePairSort::passes_for((unsigned long long)n_cells), stream);  // (the sentinel `total` itself must sort)
    hipLaunchKernelGGL(leaf_heads<kVgScanBlock>, dim3(unsigned(nb2)), dim3(kVgScanBlock), 0, stream, (const unsigned*)leaf_sort.k0, ni, g.total, d_leaf_lx.p, d_leaf_bt.p);
    hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, stream, (const unsigned*)d_leaf_bt.p, d_leaf_bt.p + nb2, nb2, &d_leaf_hdr.p->n_out);
    if (tl.sparse)
        hipLaunchKernelGGL(leaf_stats<true>, dim3(unsigned(nb1)), dim3(kVgBlock), 0, stream, (const unsigned*)leaf_sort.k0, (const unsigned*)leaf_sort.v0, ni, x, y, z,
                           (const unsigned*)d_leaf_lx.p, (const unsigned*)(d_leaf_bt.p + nb2), o);
    else
        hipLaunchKernelGGL(leaf_stats<false>, dim3(unsigned(nb1)), dim3(kVgBlock), 0, stream, (const unsigned*)leaf_sort.k0, (const unsigned*)leaf_sort.v0, ni, x, y, z,
                           (const unsigned*)d_leaf_lx.p, (const unsigned*)(d_leaf_bt.p + nb2), o);
    FLS_HIP(hipGetLastError());
    FLS_HIP(hipMemcpyAsync(&h_leaf_hdr.p[1], d_leaf_hdr.p, sizeof(VgHeader), hipMemcpyDeviceToHost, stream));
    FLS_HIP(hipStreamSynchronize(stream));
    tl.rows = h_leaf_hdr.p[1].n_out;
    return tl.rows ? kLeavesBuilt : kLeavesNone;
}

// the rows of a device build on the host (fls_debug_loop_leaves; the Match itself never reads them)
inline void LoopMatcher::download_leaves(TargetLeaves& tl) {
    const size_t r = tl.rows;
    if (tl.rows_on_host) return;
    tl.rows_on_host = true;
    tl.mean.resize(3 * r); tl.icov.resize(9 * r); tl.centroid.resize(3 * r); tl.row_cell.resize(r); tl.row_n.resize(r);
    if (!r) return;
    FLS_HIP(hipMemcpyAsync(tl.mean.data(), tl.d_mean.p, 3 * r * sizeof(double), hipMemcpyDeviceToHost, stream));
    FLS_HIP(hipMemcpyAsync(tl.icov.data(), tl.d_icov.p, 9 * r * sizeof(double), hipMemcpyDeviceToHost, stream));
    FLS_HIP(hipMemcpyAsync(tl.centroid.data(), tl.d_centroid.p, 3 * r * sizeof(float), hipMemcpyDeviceToHost, stream));
    FLS_HIP(hipMemcpyAsync(tl.row_cell.data(), tl.d_row_cell.p, r * sizeof(int), hipMemcpyDeviceToHost, stream));
    FLS_HIP(hipMemcpyAsync(tl.row_n.data(), tl.d_row_n.p, r * sizeof(int), hipMemcpyDeviceToHost, stream));
    FLS_HIP(hipStreamSynchronize(stream));
}

}  // namespace fls
