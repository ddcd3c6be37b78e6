// device_voxelgrid.hpp -- host driver of the device VoxelGrid (kernels_voxelgrid.hpp; contract there).
//
// Input: x | y | z | intensity of n points, resident on the device.  Output: the filtered cloud as x | y | z | intensity
// on the device (ascending leaf index), its size on the host.  The default (exact order) is one stream of launches with ONE host
// wait, on the output size (DeviceVoxelGrid::run_fused, kernels_voxelgrid_plan.hpp); the index-order A/B form waits twice.
#pragma once
#include "kernels_voxelgrid.hpp"
#include "kernels_exactsort.hpp"
#include "kernels_voxelgrid_plan.hpp"
#include "kernels_gridbuild.hpp"
#include "matcher_base.hpp"
#include <atomic>
#include <cstdlib>
#include <climits>

namespace fls {

// blocks of vg_minmax (six header atomics each, all on one line): 48 up to 200 k points as in rounds 2-5 ("few blocks"), one per 4,096 points beyond, at
// most 256.  Round 6: 48 blocks left a 1.55 M-point keyframe deque at 127 points per thread, 58 us in the trace (17 us with 256 blocks); 256 blocks for
// EVERY size cost the 115,200-point scans 30 us of serialised atomics (the index-order A/B legs, +12 %: tools/bench_diff.py caught it).
inline int minmax_blocks(const size_t n) { return int(std::min<size_t>(256, std::max<size_t>(48, n / 4096))); }

// stable LSD radix sort of {key, value} pairs (8 bits per pass; values keep their input order among equal keys)
struct DevicePairSort {
    DevBuf<unsigned> keys, vals;  // ping | pong
    DevBuf<unsigned> hist;        // tile counts | scanned
    DevBuf<unsigned> dig_tot;     // [pass][256] keys per digit
    size_t n = 0;
    unsigned* k0 = nullptr;       // input before run(), sorted result after
    unsigned* v0 = nullptr;
    void prepare(size_t count) {
        n = count;
        keys.reserve(2 * n);
        vals.reserve(2 * n);
        k0 = keys.p;
        v0 = vals.p;
    }
    static int passes_for(unsigned long long max_key) {
        int bits = 1;
        while ((1ull << bits) <= max_key) ++bits;
        return (bits + 7) / 8;
    }
    void run(int passes, hipStream_t s) {
        const int ni = int(n), nb = (ni + kVgTile - 1) / kVgTile;
        hist.reserve(size_t(512) * nb);
        dig_tot.reserve(4 * 256);
        FLS_HIP(hipMemsetAsync(dig_tot.p, 0, 4 * 256 * sizeof(unsigned), s));
        unsigned* k1 = k0 == keys.p ? keys.p + n : keys.p;
        unsigned* v1 = v0 == vals.p ? vals.p + n : vals.p;
        for (int pass = 0; pass < passes; ++pass) {
            hipLaunchKernelGGL(vg_hist, dim3(unsigned(nb)), dim3(kVgBlock), 0, s, (const unsigned*)k0, ni, pass * 8, hist.p, nb, dig_tot.p + 256 * pass);
            hipLaunchKernelGGL(vg_scan_rows, dim3(256), dim3(kVgScanBlock), 0, s, (const unsigned*)hist.p, hist.p + 256 * nb, nb,
                               (const unsigned*)(dig_tot.p + 256 * pass));
            hipLaunchKernelGGL(vg_scatter, dim3(unsigned(nb)), dim3(kVgBlock), 0, s, (const unsigned*)k0, (const unsigned*)v0, k1, v1, ni,
                               pass * 8, (const unsigned*)(hist.p + 256 * nb), nb);
            std::swap(k0, k1);
            std::swap(v0, v1);
        }
    }
};

// std::sort's permutation of {key, value} records on the device (kernels_exactsort.hpp), in place: ONE stream of launches without a host
// round trip -- the level-synchronous top of the recursion pre-enqueued (ranges longer than kBig records), then the persistent task kernel.
// A preceding kernel initialises the state and the queue (vg_minmax_plan, EsInitArgs); run_sync() does that from the host.
// the host-mapped words of the last sort started with FLS_ES_DEBUG set (diagnostics: fls_debug_exact_sort_marks reads them from another host thread
// while a sort is in flight, so the pointer is atomic and published only in debug runs; the owner withdraws it before freeing the memory)
inline std::atomic<EsMailbox*>& es_debug_mailbox() { static std::atomic<EsMailbox*> p{nullptr}; return p; }
struct DeviceExactSort {
    // more records are declined (= kVgMaxBlocks * kVgTile, the VoxelGrid's own limit).  The pre-enqueued levels serve every size up to it (round 6;
    // until then the host steered the top of clouds beyond kEsTaskMax through a mailbox, one round trip per top-up of two levels)
    static constexpr size_t kMaxN = size_t(1) << 22;
    // Ranges longer than kBig records are partitioned LEVEL-SYNCHRONOUSLY by the whole device -- three launches per level (es_level_begin /
    // count_scatter / swap, the regime-1 kernels): one workgroup needs 3 us + 0.38 us per thousand records for a partition
    // (profiles/r05_d_ndt_global_levels.log: 47 us at 115,200), a level of launches ~16 us whatever the size.  kEsTaskMax until round 6; the deepest
    // chain of one-workgroup partitions below a 131,072-record range (~290 us at 13/16 splits) was the task kernel's critical path.  Measured with
    // the ticket queue, 32,768 / 65,536 / 131,072: planar deque 0.80 / 0.75 / 0.93 ms, IcpOptimized deque 0.48 / 0.53 / 0.65 ms, corner deque
    // 0.37 / 0.42 / 0.44 ms (profiles/r06_h_*)
    static constexpr unsigned kBig = 32768;
    DevBuf<EsSeg> seg_a, seg_b;
    DevBuf<EsWork> work;
    DevBuf<unsigned long long> tile_pub;  // es_count_scatter_kernel: a tile's published counts + the launch's epoch
    unsigned pub_epoch = 0;
    DevBuf<unsigned> tile_seg, Lp, Rl;
    DevBuf<EsState> st;
    DevBuf<EsQueue> queue;
    DevBuf<unsigned> ready;
    EsMailbox* mb_host = nullptr;
    EsMailbox* mb_dev = nullptr;
    unsigned work_cap = 0, tile_cap = 0;
    ~DeviceExactSort() {
        EsMailbox* mine = mb_host;
        es_debug_mailbox().compare_exchange_strong(mine, nullptr);
        if (mb_host) (void)hipHostFree(mb_host);
    }
    // records a workgroup of the task kernel sorts in LDS, by cloud size (kernels_exactsort.hpp, kEsLds)
    static unsigned lds_cap_for(const size_t n) { return n <= size_t(kEsTaskMax) ? unsigned(kEsLdsSmall) : unsigned(kEsLds); }
    // one workgroup per CU at most; as many as there are 2,048-record pieces -- NOT n / lds_cap: with 8,192-record LDS ranges that left the 475,200-record
    // deque of IcpOptimized to 62 workgroups, five ranges of ~76 us each in a row on the busiest one (profiles/r06_vg_large_cloud_filters.txt)
    static unsigned task_grid(const size_t n) { return unsigned(std::min<size_t>(256, std::max<size_t>(8, n / kEsLdsSmall + 4))); }
    void allocate(const size_t n) {
        if (!mb_host) {
            FLS_HIP(hipHostMalloc((void**)&mb_host, sizeof(EsMailbox), hipHostMallocMapped));
            std::memset(mb_host, 0, sizeof(EsMailbox));
            FLS_HIP(hipHostGetDevicePointer((void**)&mb_dev, mb_host, 0));
        }
        static const bool publish_dbg = std::getenv("FLS_ES_DEBUG") != nullptr;
        if (publish_dbg) es_debug_mailbox().store(mb_host, std::memory_order_release);
        work_cap = unsigned(64 * (n / kEsLdsSmall + 1) + 1024);
        tile_cap = unsigned(n / kEsTile + kEsMaxSeg + 2);
        seg_a.reserve(kEsMaxSeg); seg_b.reserve(kEsMaxSeg);
        work.reserve(work_cap);
        ready.reserve(work_cap);
        tile_seg.reserve(tile_cap);
        if (tile_pub.cap < tile_cap) {  // a fresh buffer holds epoch 0, which no launch uses (growth is rare: filled and waited for here)
            tile_pub.reserve(tile_cap);
            FLS_HIP(hipMemset(tile_pub.p, 0, tile_pub.cap * sizeof(unsigned long long)));
            FLS_HIP(hipDeviceSynchronize());
        }
        Lp.reserve(n); Rl.reserve(n);
        st.reserve(1);
        queue.reserve(1);
    }
    // fused_prepare() before the kernel that initialises the queue is queued, fused_launch() behind the kernel that writes the records.  `skip`:
    // device word, non-zero = nothing to sort.  The verdict (EsState::fail) stays on the device: the caller's last kernel forwards it.
    EsInitArgs fused_prepare(const size_t n) {
        allocate(n);
        return EsInitArgs{st.p, queue.p, ready.p, work_cap};
    }
    // The number of level-synchronous levels is a guess (the larger child keeps ~13/16 of a LiDAR range); levels that find nothing left are empty
    // launches, ranges still longer than kBig after the last one are the task kernel's (one workgroup each).
    void fused_launch(unsigned* key, unsigned* val, const size_t n, const unsigned* skip, hipStream_t s) {
        const unsigned grid = task_grid(n);
        static const bool dbg_marks = std::getenv("FLS_ES_DEBUG") != nullptr;
        if (dbg_marks) std::memset(mb_host->mark, 0, sizeof(mb_host->mark));
        EsMailbox* const dbg = dbg_marks ? mb_dev : nullptr;
        // (a single scan keeps ~13/16 of a range in the larger child; the keyframe deques beyond kEsTaskMax records -- the same surfaces many times
        // over -- split more evenly: ~0.7 measured, 15 levels for 1.55 M records where 13/16 all the way guesses 19, each empty level three launches)
        int top = 0;
        size_t m = n;
        for (; m > size_t(kEsTaskMax); m = m * 7 / 10) ++top;
        for (; m > size_t(kBig); m = m * 13 / 16) ++top;
        if (top == 0) {
            hipLaunchKernelGGL(es_task_kernel, dim3(grid), dim3(kEsTaskThreads), 0, s, key, val, work.p, ready.p, work_cap, queue.p, Lp.p, Rl.p, st.p, dbg,
                               unsigned(n), skip, lds_cap_for(n));
            return;
        }
        EsSeg* prev = seg_a.p;
        EsSeg* cur = seg_b.p;
        hipLaunchKernelGGL(es_level_begin, dim3(1), dim3(256), 0, s, key, val, unsigned(n), (const EsSeg*)prev, cur, work.p, work_cap, (const unsigned*)Lp.p,
                           (const unsigned*)Rl.p, st.p, 1, tile_seg.p, tile_cap, kBig, 0, queue.p, skip);
        for (int l = 0; l < top; ++l) {
            if (++pub_epoch == 0u) ++pub_epoch;  // (0 is what a fresh buffer holds)
            hipLaunchKernelGGL(es_count_scatter_kernel, dim3(tile_cap), dim3(kEsBlock), 0, s, (const unsigned*)key, cur, st.p, (const unsigned*)tile_seg.p,
                               tile_pub.p, pub_epoch, Lp.p, Rl.p);
            hipLaunchKernelGGL(es_swap_kernel, dim3(tile_cap), dim3(kEsBlock), 0, s, key, val, cur, (const EsState*)st.p, (const unsigned*)tile_seg.p,
                               (const unsigned*)Lp.p, (const unsigned*)Rl.p);
            std::swap(prev, cur);
            hipLaunchKernelGGL(es_level_begin, dim3(1), dim3(256), 0, s, key, val, unsigned(n), (const EsSeg*)prev, cur, work.p, work_cap, (const unsigned*)Lp.p,
                               (const unsigned*)Rl.p, st.p, 0, tile_seg.p, tile_cap, kBig, l == top - 1 ? 1 : 0, queue.p, skip);
        }
        hipLaunchKernelGGL(es_task_kernel, dim3(grid), dim3(kEsTaskThreads), 0, s, key, val, work.p, ready.p, work_cap, queue.p, Lp.p, Rl.p, st.p, dbg, 0u,
                           skip, lds_cap_for(n));
    }
    // the standalone form (test hook fls_debug_exact_sort): the initialisation vg_minmax_plan's last block does, written from the host, then the
    // same launches on the null stream and a device synchronisation.  false: declined (more than kMaxN records, or EsState::fail: introsort's
    // depth limit on a range longer than lds_cap, a table overflow)
    bool run_sync(unsigned* key, unsigned* val, const size_t n) {
        if (n < 2) return true;
        if (n > kMaxN) return false;
        const EsInitArgs ia = fused_prepare(n);
        FLS_HIP(hipMemset(ia.st, 0, sizeof(EsState)));
        FLS_HIP(hipMemset(ia.ready, 0, ia.work_cap * sizeof(unsigned)));
        const EsQueue q0{0u, 0u, 1u, 0u};
        FLS_HIP(hipMemcpy(ia.q, &q0, sizeof(EsQueue), hipMemcpyHostToDevice));
        fused_launch(key, val, n, nullptr, nullptr);
        FLS_HIP(hipDeviceSynchronize());
        print_debug_stamps();
        EsState hs;
        FLS_HIP(hipMemcpy(&hs, ia.st, sizeof(EsState), hipMemcpyDeviceToHost));
        return hs.fail == 0u;
    }
    void print_wg_profile() {
        if (!mb_host) return;
        {  // where the workgroups of the task kernel spent their time (100 MHz ticks -> us)
            double w = 0, g = 0, l = 0, wmax = 0, bmax = 0; unsigned nt = 0, used = 0;
            for (int b = 0; b < 256; ++b) {
                const unsigned* q = mb_host->wg[b];
                if (!q[0] && !q[1] && !q[2]) continue;
                ++used; w += q[0]; g += q[1]; l += q[2]; nt += q[3];
                wmax = std::max(wmax, double(q[0])); bmax = std::max(bmax, double(q[1]) + double(q[2]));
            }
            if (used)
                std::fprintf(stderr, "[fls exact sort] task kernel, %u workgroups, mean per workgroup [us]: waiting for tasks %.1f, partitions out of global memory %.1f, LDS ranges %.1f; "
                             "busiest workgroup %.1f us busy, longest wait %.1f us; %u tasks popped\n", used, 0.01 * w / used, 0.01 * g / used, 0.01 * l / used, 0.01 * bmax, 0.01 * wmax, nt);
            // the eight busiest workgroups, one by one
            std::vector<int> order;
            for (int b = 0; b < 256; ++b) if (mb_host->wg[b][1] || mb_host->wg[b][2]) order.push_back(b);
            std::sort(order.begin(), order.end(), [&](int a, int b) { return mb_host->wg[a][1] + mb_host->wg[a][2] > mb_host->wg[b][1] + mb_host->wg[b][2]; });
            for (size_t i = 0; i < order.size() && i < 8; ++i) {
                const unsigned* q = mb_host->wg[order[i]];
                std::fprintf(stderr, "[fls exact sort]   workgroup %3d: %u tasks, wait %.1f, global %.1f, LDS %.1f us | longest LDS range %.1f us (%u records) | longest global chain %.1f us (from %u records)\n",
                             order[i], q[3], 0.01 * q[0], 0.01 * q[1], 0.01 * q[2], 0.01 * q[4], q[5], 0.01 * q[6], q[7]);
            }
            std::memset(mb_host->wg, 0, sizeof(mb_host->wg));
        }
    }
    // FLS_ES_DEBUG: stage stamps of the last sort
    void print_debug_stamps() {
        static const bool dbg = std::getenv("FLS_ES_DEBUG") && std::atoi(std::getenv("FLS_ES_DEBUG")) != 0;
        if (dbg && mb_host) {
            const unsigned* mk = mb_host->mark;
            auto us = [&](int a, int b) { return mk[a] && mk[b] ? 0.01 * double(int(mk[b] - mk[a])) : -1.0; };
            std::fprintf(stderr, "[fls exact sort] workgroup 0, first task [us]: pop->start %.1f, global partitions %.1f, LDS load %.1f, phase A (workgroup partitions) %.1f, phase B (wave tasks) %.1f, "
                         "ranks + write-back %.1f\n", us(0, 2), us(2, 9), us(9, 10), us(10, 3), us(3, 4), us(5, 6));
            for (int i = 0; i < 32 && mb_host->lvl[i][0]; ++i) {
                const unsigned* q = mb_host->lvl[i];
                auto d = [&](int a, int b) { return 0.01 * double(int(q[b] - q[a])); };
                std::fprintf(stderr, "[fls exact sort]   global partition %2d: %6u records | median %.1f | count %.1f | lists %.1f | swaps %.1f | cut + push %.1f | total %.1f us\n", i, q[0], d(1, 2), d(2, 3),
                             d(3, 4), d(4, 5), d(5, 6), d(1, 6));
            }
            std::memset(mb_host->lvl, 0, sizeof(mb_host->lvl));
            print_wg_profile();
        }
    }
};

// FLS_DEVICE_VOXELGRID: 1 (default) the device filters, leaf sums in std::sort's order = bit-identical to pcl::VoxelGrid (round 4);
// 0 the exact host filter (worker pool); 2 the device filters with the round-2/3 contract (stable radix sort: leaf sums in ascending
// point index, last-bit differences on leaves of three or more points) -- A/B only.
inline int device_voxelgrid_mode() {
    if (const char* e = std::getenv("FLS_DEVICE_VOXELGRID")) { const int v = std::atoi(e); return v < 0 ? 0 : v > 2 ? 1 : v; }
    return 1;
}

struct DeviceVoxelGrid {
    DevicePairSort sort;
    DeviceExactSort exact;
    bool exact_order = device_voxelgrid_mode() != 2;  // centroids summed in std::sort's order; false: ascending point index
    DevBuf<unsigned> lx, bt;        // bt: block totals | scanned
    DevBuf<float4> sorted;          // the points in sorted order
    DevBuf<float> out;            // x | y | z | i, capacity n each
    DevBuf<VgHeader> d_hdr;       // run_index_order
    PinnedBuf<VgHeader> h_hdr;    // [0] = init template, [1] = read-back
    // the uninterrupted form (kernels_voxelgrid_plan.hpp): plan + accumulators on the device, the verdict in a host-mapped mailbox
    DevBuf<VgPlan> d_plan;
    DevBuf<VgAccum> d_acc;
    VgMailbox* vmb_host = nullptr;
    VgMailbox* vmb_dev = nullptr;
    unsigned vseq = 0;
    size_t n_in = 0, n_out = 0;
    ~DeviceVoxelGrid() { if (vmb_host) (void)hipHostFree(vmb_host); }
    DeviceVoxelGrid() = default;
    DeviceVoxelGrid(const DeviceVoxelGrid&) = delete;
    DeviceVoxelGrid& operator=(const DeviceVoxelGrid&) = delete;
    const float* ox() const { return out.p; }
    const float* oy() const { return out.p + n_in; }
    const float* oz() const { return out.p + 2 * n_in; }
    const float* oi() const { return out.p + 3 * n_in; }

    // false: not applicable (empty, too large, or PCL's "leaf size too small" case) -- the caller takes the host path
    bool run(const float* x, const float* y, const float* z, const float* in, size_t n, float leaf, hipStream_t s) {
        n_in = n;
        n_out = 0;
        if (n == 0 || n > size_t(kVgMaxBlocks) * kVgTile) return false;  // (= DeviceExactSort::kMaxN)
        return exact_order ? run_fused(x, y, z, in, n, leaf, s) : run_index_order(x, y, z, in, n, leaf, s);
    }

    // FLS_DEVICE_VOXELGRID=2 only (A/B): the round-2/3 form -- stable radix sort, leaf sums in ascending point index (kernels_voxelgrid.hpp
    // CONTRACT) -- with two short host waits: the bounds (they decide the number of radix passes and the "leaf size too small" refusal,
    // voxel_grid.hpp:69-74) and the output size
    bool run_index_order(const float* x, const float* y, const float* z, const float* in, size_t n, float leaf, hipStream_t s) {
        h_hdr.reserve(2);
        d_hdr.reserve(1);
        for (int a = 0; a < 3; ++a) { h_hdr.p[0].mn[a] = 0xffffffffu; h_hdr.p[0].mx[a] = 0u; }
        h_hdr.p[0].n_out = 0u; h_hdr.p[0].n_bad = 0u;
        FLS_HIP(hipMemcpyAsync(d_hdr.p, &h_hdr.p[0], sizeof(VgHeader), hipMemcpyHostToDevice, s));
        const int ni = int(n);
        const int nb1 = (ni + kVgBlock - 1) / kVgBlock, nb2 = (ni + kVgScanBlock - 1) / kVgScanBlock;
        hipLaunchKernelGGL(vg_minmax, dim3(unsigned(std::min(nb1, minmax_blocks(n)))), dim3(kVgBlock), 0, s, x, y, z, ni, d_hdr.p);
        FLS_HIP(hipMemcpyAsync(&h_hdr.p[1], d_hdr.p, sizeof(VgHeader), hipMemcpyDeviceToHost, s));
        FLS_HIP(hipStreamSynchronize(s));
        const VgHeader& hh = h_hdr.p[1];
        if (hh.mn[0] == 0xffffffffu) return false;  // no finite point: the host path returns the empty cloud
        const float inv = 1.0f / leaf;
        float mn[3], mx[3];
        for (int a = 0; a < 3; ++a) { mn[a] = vg_unord(hh.mn[a]); mx[a] = vg_unord(hh.mx[a]); }
        const float ex = (mx[0] - mn[0]) * inv, ey = (mx[1] - mn[1]) * inv, ez = (mx[2] - mn[2]) * inv;
        if (!(ex < 2147483648.0f && ey < 2147483648.0f && ez < 2147483648.0f)) return false;  // (one extent of 2^31 leaves is already beyond INT_MAX; keeps the products inside int64)
        const long long dx = (long long)ex + 1, dy = (long long)ey + 1, dz = (long long)ez + 1;
        if (dx * dy > (long long)INT_MAX || dx * dy * dz > (long long)INT_MAX) return false;
        VgGrid g;
        g.inv = inv;
        long long div_b[3];
        for (int a = 0; a < 3; ++a) {
            g.min_b[a] = int(std::floor(mn[a] * inv));
            div_b[a] = (long long)int(std::floor(mx[a] * inv)) - g.min_b[a] + 1;
        }
        const long long total = div_b[0] * div_b[1] * div_b[2];
        if (total <= 0 || total >= (long long)INT_MAX) return false;
        g.m1 = int(div_b[0]);
        g.m2 = int(div_b[0] * div_b[1]);
        g.total = unsigned(total);
        const int passes = DevicePairSort::passes_for((unsigned long long)total);  // the sentinel `total` itself must sort

        sort.prepare(n);
        lx.reserve(n);
        bt.reserve(size_t(2 * nb2));
        sorted.reserve(n);
        out.reserve(4 * n);
        hipLaunchKernelGGL(vg_index, dim3(unsigned(nb1)), dim3(kVgBlock), 0, s, x, y, z, ni, g, sort.k0, sort.v0);
        sort.run(passes, s);
        unsigned* const k0 = sort.k0;
        unsigned* const v0 = sort.v0;
        hipLaunchKernelGGL(vg_heads, dim3(unsigned(nb2)), dim3(kVgScanBlock), 0, s, (const unsigned*)k0, (const unsigned*)v0, ni, g.total, x, y, z, in,
                           sorted.p, lx.p, bt.p);
        hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, s, (const unsigned*)bt.p, bt.p + nb2, nb2, &d_hdr.p->n_out);
        hipLaunchKernelGGL(vg_centroid, dim3(unsigned(nb1)), dim3(kVgBlock), 0, s, (const unsigned*)k0, (const float4*)sorted.p, ni,
                           (const unsigned*)lx.p, (const unsigned*)(bt.p + nb2), out.p, out.p + n, out.p + 2 * n, out.p + 3 * n);
        FLS_HIP(hipMemcpyAsync(&h_hdr.p[1], d_hdr.p, sizeof(VgHeader), hipMemcpyDeviceToHost, s));
        FLS_HIP(hipStreamSynchronize(s));
        FLS_HIP(hipGetLastError());
        n_out = h_hdr.p[1].n_out;
        return true;
    }

    // One uninterrupted stream of launches (kernels_voxelgrid_plan.hpp): bounds + plan + sort-queue initialisation, leaf indices, the exact
    // sort, run heads, offsets + verdict to the mailbox, centroids.  The host waits ONCE, on a host-mapped word the offsets kernel writes --
    // before the centroid kernel has finished; whatever the caller queues next on `s` is ordered behind it.  Every exact-order call, n = 1
    // included: a single point needs no sort, and the EsState vg_minmax_plan zeroes tells the later kernels that none failed.
    bool run_fused(const float* x, const float* y, const float* z, const float* in, size_t n, float leaf, hipStream_t s) {
        if (!vmb_host) {
            FLS_HIP(hipHostMalloc((void**)&vmb_host, sizeof(VgMailbox), hipHostMallocMapped));
            std::memset(vmb_host, 0, sizeof(VgMailbox));
            FLS_HIP(hipHostGetDevicePointer((void**)&vmb_dev, vmb_host, 0));
        }
        if (!d_acc.p) {  // armed once; the last block of every vg_minmax_plan re-arms it
            d_acc.reserve(1);
            d_plan.reserve(1);
            FLS_HIP(hipMemsetAsync(d_acc.p, 0, sizeof(VgAccum), s));  // (the ticket; the rows are written before they are read)
            FLS_HIP(hipStreamSynchronize(s));
        }
        const int ni = int(n);
        const int nb1 = (ni + kVgBlock - 1) / kVgBlock, nb2 = (ni + kVgScanBlock - 1) / kVgScanBlock;
        sort.prepare(n);
        lx.reserve(n);
        bt.reserve(size_t(2 * nb2));
        sorted.reserve(n);
        out.reserve(4 * n);
        const EsInitArgs es = exact.fused_prepare(n);
        vseq = (vseq + 1u) & 0x7fffffffu;
        if (!vseq) vseq = 1u;
        const float inv = 1.0f / leaf;
        // (the reference sorts the FINITE points only: a cloud with a non-finite point is the host's, refuse_bad = 1)
        // (blocks: 48 in rounds 2-4 -- "few blocks: six header atomics each" -- left a 115,200-point scan to 12 k threads, 11-12 us in the trace
        // of the call; 160 blocks = three points per thread and < 1,000 atomics)
        const int mm_blocks = int(std::min<size_t>(kVgMinmaxMaxBlocks, std::max<size_t>(160, n / 4096)));  // (one row per block, no atomics but the ticket: more blocks for the keyframe deques)
        hipLaunchKernelGGL(vg_minmax_plan, dim3(unsigned(std::min(nb1, mm_blocks))), dim3(kVgBlock), 0, s, x, y, z, ni, inv, 1, d_acc.p, d_plan.p, es);
        hipLaunchKernelGGL(vg_index_plan, dim3(unsigned(nb1)), dim3(kVgBlock), 0, s, x, y, z, ni, (const VgPlan*)d_plan.p, sort.k0, sort.v0);
        if (n >= 2) exact.fused_launch(sort.k0, sort.v0, n, &d_plan.p->status, s);
        hipLaunchKernelGGL(vg_heads_plan, dim3(unsigned(nb2)), dim3(kVgScanBlock), 0, s, (const unsigned*)sort.k0, (const unsigned*)sort.v0, ni, (const VgPlan*)d_plan.p,
                           (const EsState*)exact.st.p, x, y, z, in, sorted.p, lx.p, bt.p);
        hipLaunchKernelGGL(vg_scan_publish, dim3(1), dim3(kVgScanBlock), 0, s, (const unsigned*)bt.p, bt.p + nb2, nb2, (const VgPlan*)d_plan.p, (const EsState*)exact.st.p,
                           vmb_dev, vseq);
        hipLaunchKernelGGL(vg_centroid_plan, dim3(unsigned(nb1)), dim3(kVgBlock), 0, s, (const unsigned*)sort.k0, (const float4*)sorted.p, ni, (const VgPlan*)d_plan.p,
                           (const EsState*)exact.st.p, (const unsigned*)lx.p, (const unsigned*)(bt.p + nb2), out.p, out.p + n, out.p + 2 * n, out.p + 3 * n);
        FLS_HIP(hipGetLastError());
        const auto published = [&] { return __atomic_load_n(&vmb_host->seq, __ATOMIC_ACQUIRE) == vseq; };
        if (!spin_until(s, published) && !published()) FLS_HIP(hipErrorUnknown);  // (the stream went idle without a verdict)
        exact.print_debug_stamps();
        if (vmb_host->status != kVgOk || vmb_host->sort_fail != 0u) {
            FLS_HIP(hipStreamSynchronize(s));  // (the staging the caller reuses; the refused call is rare)
            return false;
        }
        n_out = vmb_host->n_out;
        return true;
    }

    // the filtered cloud on the host (map updates keep their clouds there)
    std::vector<PtI> download(hipStream_t s, std::vector<float>& tmp) const {
        std::vector<PtI> c(n_out);
        if (n_out == 0) return c;
        tmp.resize(4 * n_out);
        for (int a = 0; a < 4; ++a)
            FLS_HIP(hipMemcpyAsync(tmp.data() + size_t(a) * n_out, out.p + size_t(a) * n_in, n_out * sizeof(float), hipMemcpyDeviceToHost, s));
        FLS_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; i < n_out; ++i) c[i] = PtI{tmp[i], tmp[n_out + i], tmp[2 * n_out + i], tmp[3 * n_out + i]};
        return c;
    }
};

// ---------------------------------------------------------------------------------------------
// The kd-tree kinds' cell grid built on the device (kernels_gridbuild.hpp): exact, so it is the default
// (FLS_DEVICE_GRID_BUILD=0 restores the host build).  Input: the map cloud as x | y | z planes resident on the device.
// One short host wait (the bounds decide the window).  false: declined (empty, a non-finite point, cells outside the key
// range, a window larger than kMaxWindowCells) -- the caller takes the host build, which also produces the error codes.
// ---------------------------------------------------------------------------------------------
struct DeviceGridBuilder {
    DevicePairSort sort;
    DevBuf<VgHeader> d_hdr;
    PinnedBuf<VgHeader> h_hdr;
    unsigned long long builds = 0, declined = 0;
    bool run(CellGridImage& g, const float* x, const float* y, const float* z, size_t n, float cell_size, int n_rings, bool with_by_id, hipStream_t s) {
        if (n == 0 || n > size_t(kVgMaxBlocks) * kVgTile) { ++declined; return false; }
        h_hdr.reserve(2);
        d_hdr.reserve(1);
        for (int a = 0; a < 3; ++a) { h_hdr.p[0].mn[a] = 0xffffffffu; h_hdr.p[0].mx[a] = 0u; }
        h_hdr.p[0].n_out = 0u; h_hdr.p[0].n_bad = 0u;
        FLS_HIP(hipMemcpyAsync(d_hdr.p, &h_hdr.p[0], sizeof(VgHeader), hipMemcpyHostToDevice, s));
        const int ni = int(n), nb = (ni + kVgBlock - 1) / kVgBlock;
        hipLaunchKernelGGL(vg_minmax, dim3(unsigned(std::min(nb, minmax_blocks(n)))), dim3(kVgBlock), 0, s, x, y, z, ni, d_hdr.p);
        FLS_HIP(hipMemcpyAsync(&h_hdr.p[1], d_hdr.p, sizeof(VgHeader), hipMemcpyDeviceToHost, s));
        FLS_HIP(hipStreamSynchronize(s));
        const VgHeader& hh = h_hdr.p[1];
        if (hh.n_bad != 0u || hh.mn[0] == 0xffffffffu) { ++declined; return false; }
        const double inv = 1.0 / double(cell_size);
        CgWindow w;
        w.inv_cell = inv;
        int mn[3], mx[3];
        for (int a = 0; a < 3; ++a) {  // floor(double(p) * inv), cg_keys' expression, is monotone in p: the extreme cells come from the extreme coordinates
            const double lo = std::floor(double(vg_unord(hh.mn[a])) * inv), hi = std::floor(double(vg_unord(hh.mx[a])) * inv);
            if (!(std::fabs(lo) < double(kKeyLimit) && std::fabs(hi) < double(kKeyLimit))) { ++declined; return false; }
            mn[a] = int(lo); mx[a] = int(hi);
        }
        size_t nc = 1;
        for (int a = 0; a < 3; ++a) nc *= size_t(mx[a] - mn[a] + 1);
        if (nc > GridImage::kMaxWindowCells) { ++declined; return false; }
        w.ox = mn[0]; w.oy = mn[1]; w.oz = mn[2];
        w.nx = mx[0] - mn[0] + 1; w.ny = mx[1] - mn[1] + 1; w.nz = mx[2] - mn[2] + 1;
        sort.prepare(n);
        g.d_pts.reserve(n);
        g.d_cells.reserve(nc);
        g.d_table.reserve(1);  // (never probed: every search kernel takes the window path when the window exists)
        FLS_HIP(hipMemsetAsync(g.d_cells.p, 0, nc * sizeof(uint2), s));
        hipLaunchKernelGGL(cg_keys, dim3(unsigned(nb)), dim3(kVgBlock), 0, s, x, y, z, ni, w, sort.k0, sort.v0);
        sort.run(DevicePairSort::passes_for((unsigned long long)(nc - 1)), s);
        hipLaunchKernelGGL(cg_fill, dim3(unsigned(nb)), dim3(kVgBlock), 0, s, (const unsigned*)sort.k0, (const unsigned*)sort.v0, ni, x, y, z, g.d_pts.p, g.d_cells.p);
        hipLaunchKernelGGL(cg_count, dim3(unsigned(nb)), dim3(kVgBlock), 0, s, (const unsigned*)sort.k0, ni, g.d_cells.p);
        if (with_by_id) {
            g.d_by_id.reserve(n);
            hipLaunchKernelGGL(cg_by_id, dim3(unsigned(nb)), dim3(kVgBlock), 0, s, x, y, z, ni, g.d_by_id.p);
        }
        FLS_HIP(hipGetLastError());
        g.cell = cell_size;
        g.inv_cell = inv;
        g.rings = n_rings;
        g.table.clear(); g.pts.clear(); g.cells.clear();
        g.mask = 0;
        g.used = n;
        g.have_window = true;
        g.win_o[0] = w.ox; g.win_o[1] = w.oy; g.win_o[2] = w.oz;
        g.win_n[0] = w.nx; g.win_n[1] = w.ny; g.win_n[2] = w.nz;
        g.n_cells = 0;  // (not counted on this path)
        ++builds;
        return true;
    }
};

// the source-scan filter of the kd-tree / NDT matchers (icp_optimized.h:57, incremental_ndt.h:232): on the device (default), the
// host std::sort path with FLS_DEVICE_VOXELGRID=0 and for whatever the device declines.  With the device path the filtered cloud
// stays on the device; the host copy is fetched only when a map update needs it.
struct SourceFilter {
    bool on_device = true;
    DevScan raw;
    DeviceVoxelGrid vg;
    bool resident = false;  // `source` has not been downloaded yet
    std::vector<float> tmp;
    unsigned long long device_runs = 0, host_runs = 0;
    void init() {
        on_device = device_voxelgrid_mode() != 0;
    }
    void filter(const float* s0, size_t n0, int stride, float leaf, hipStream_t s, DevScan& scan, std::vector<PtI>& source) {
        resident = false;
        raw_pending = false;
        if (on_device && n0 != 0) {
            raw.upload_raw(s0, n0, stride, s, true);
            if (vg.run(raw.x.p, raw.y.p, raw.z.p, raw.xyz.p + 3 * n0, n0, leaf, s)) {
                scan.n = vg.n_out;
                scan.host.clear();
                scan.x.p = const_cast<float*>(vg.ox());
                scan.y.p = const_cast<float*>(vg.oy());
                scan.z.p = const_cast<float*>(vg.oz());
                source.clear();
                resident = true;
                ++device_runs;
                return;
            }
        }
        source = voxel_grid_strided(s0, n0, stride, leaf);
        scan.upload(source, s);
        ++host_runs;
    }
    // fls_scan_upload_raw: the RAW scan stays resident (x | y | z | intensity of raw_n points) and every fls_match_resident runs the source
    // filter itself, like the reference's Match does (icp_optimized.h:57, incremental_ndt.h:231-232) -- what bench.py times for configs[0] / [2]
    bool raw_pending = false;
    bool withdrawn = false;  // between fls_scan_upload_raw and the next Match: no filtered scan is resident
    size_t raw_n = 0;
    float raw_leaf = 0.f;
    std::vector<float> raw_host;  // packed xyzi rows of the raw scan: only what the device declines goes back to the host filter
    void upload_raw_only(const float* s0, size_t n0, int stride, float leaf, hipStream_t s, DevScan& scan, std::vector<PtI>& source) {
        // the filtered scan of the PREVIOUS upload is gone from here on (fitness / correspondences / a map update between this call and
        // the next fls_match_resident must not see the old scan): nothing is resident until refilter() has run
        resident = false;
        scan.n = 0;
        scan.host.clear();
        source.clear();
        withdrawn = true;
        raw_pending = true;
        raw_n = n0;
        raw_leaf = leaf;
        raw_host.resize(4 * n0);
        for (size_t i = 0; i < n0; ++i) {
            const float* q = s0 + i * size_t(stride);
            raw_host[4 * i] = q[0]; raw_host[4 * i + 1] = q[1]; raw_host[4 * i + 2] = q[2]; raw_host[4 * i + 3] = intensity_of(q, stride);
        }
        if (n0) { raw.upload_raw(s0, n0, stride, s, true); FLS_HIP(hipStreamSynchronize(s)); }
    }
    // the same state from a cloud that is already on this device (fls_scan_attach_preprocessed): the copy kernel fills `raw`, nothing
    // is synchronised, and raw_host is fetched only if the device filter declines
    void attach_raw_only(const HandoffCloud& c, float leaf, hipStream_t s, DevScan& scan, std::vector<PtI>& source) {
        resident = false;
        scan.n = 0;
        scan.host.clear();
        source.clear();
        withdrawn = true;
        raw_pending = true;
        raw_n = c.n;
        raw_leaf = leaf;
        raw_host.clear();
        raw.attach_device(c, s, /*want_host=*/false);
    }
    const float* raw_rows(hipStream_t s) {
        if (raw.stage_stale) {
            raw.fetch_stage(s);
            raw_host.resize(4 * raw_n);
            const float* st = raw.stage.p;
            for (size_t i = 0; i < raw_n; ++i) {
                raw_host[4 * i] = st[i]; raw_host[4 * i + 1] = st[raw_n + i]; raw_host[4 * i + 2] = st[2 * raw_n + i]; raw_host[4 * i + 3] = st[3 * raw_n + i];
            }
        }
        return raw_host.data();
    }
    void refilter(hipStream_t s, DevScan& scan, std::vector<PtI>& source) {
        resident = false;
        withdrawn = false;
        if (on_device && raw_n != 0 && vg.run(raw.x.p, raw.y.p, raw.z.p, raw.xyz.p + 3 * raw_n, raw_n, raw_leaf, s)) {
            scan.n = vg.n_out;
            scan.host.clear();
            scan.x.p = const_cast<float*>(vg.ox());
            scan.y.p = const_cast<float*>(vg.oy());
            scan.z.p = const_cast<float*>(vg.oz());
            source.clear();
            resident = true;
            ++device_runs;
            return;
        }
        source = voxel_grid_strided(raw_rows(s), raw_n, 4, raw_leaf);
        scan.upload(source, s);
        ++host_runs;
    }
    void materialize(hipStream_t s, std::vector<PtI>& source) {
        if (!resident) return;
        source = vg.download(s, tmp);
        resident = false;
    }
};

}  // namespace fls
