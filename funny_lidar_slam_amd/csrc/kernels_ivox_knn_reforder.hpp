// kernels_ivox_knn_reforder.hpp -- ivox_knn_reforder_kernel: the iVox kNN launch in the REFERENCE's neighbour order (fls_knn_order.h,
// FLS_KNN_ORDER_REFERENCE), and its launch from P2PlaneIvoxMatcher::match_launch.
//
// A parity mode: one lane replays one query's GetClosestPoint sequentially through knn_reference_order.hpp -- the 19 probes in the reference's
// order, every voxel's points in slot (= insertion) order, libstdc++'s nth_element on records {d2, map slot} -- so that the list a point gets is
// the reference's under exact distance ties too, slots 1..4 in introselect order.  The work array is indexed at run time and would be scratch as
// a private array: it lies in LDS, record j of lane l at work[j * 32 + l], 32 queries x kro::kWork records x 8 bytes = 64 KiB per 32-thread
// workgroup.  Output contract: ivox_knn_kernel's ids form (nn_ids[q][0..4] map slots, ~0u behind the count; nn_cnt[q]; the FIRST duties; st->done;
// a query without candidates leaves its list alone), so the fit launch, ivox_nn_materialize_kernel and the map-update decision run unchanged.
// A query that probes a voxel of more than kro::kVoxelLimit points is not replayed: it gets the default kernel's (d2 bits, slot) list and
// *fallbacks counts it.  The max_range gate d2 < 25 is applied always.
// This header is included last (fls_reg.hip), so that the code object keeps the order of the kernels in front of it.
#pragma once
#include "matcher_p2plane_ivox.hpp"
#include "knn_reference_order.hpp"

namespace fls {

constexpr int kKnnRefQueries = 32;  // queries (= threads) per workgroup
static_assert(sizeof(kro::Rec) == 8 && kKnnRefQueries * kro::kWork * sizeof(kro::Rec) <= 65536, "one workgroup's work arrays fit 64 KiB of LDS");

// the probe order of the replay is the default kernel's (kernels_ivox_coop.hpp packs the same table)
constexpr bool kro_probe_order_is_nearby18() {
    for (int k = 0; k < kro::kProbes; ++k) {
        int dx = 0, dy = 0, dz = 0;
        kro::nearby18(k, dx, dy, dz);
        if ((dz * kBrickStored + dy) * kBrickStored + dx != nearby18_slab(k)) return false;
    }
    return true;
}
static_assert(kro_probe_order_is_nearby18(), "knn_reference_order.hpp and kernels_ivox_coop.hpp visit the 19 voxels in one order");

template <bool DENSE, bool FIRST, bool GEN>
__global__ void __launch_bounds__(kKnnRefQueries)
ivox_knn_reforder_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, const int n,
                         const GnState* __restrict__ st, const Pose16 T0, const DevGrid grid, const BrickDir bd, const float inv_res,
                         unsigned char* __restrict__ nn_cnt, unsigned char* __restrict__ flag, unsigned* __restrict__ nn_ids /* [n][8] */,
                         const int nn_prev, float* __restrict__ dev_copy /* FIRST, may be null: as ivox_knn_kernel's */,
                         unsigned long long* __restrict__ fallbacks) {
    __shared__ kro::Rec work[kro::kWork * kKnnRefQueries];
    const int q = blockIdx.x * kKnnRefQueries + threadIdx.x;
    if (q >= n) return;
    if (!FIRST && st->done) return;
    double T[12];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) T[c * 3 + r] = FIRST ? T0.m[c * 4 + r] : st->T[c * 4 + r];
    const float px = sx[q], py = sy[q], pz = sz[q];
    if (FIRST) {
        if (dev_copy) { dev_copy[q] = px; dev_copy[(size_t)n + q] = py; dev_copy[2 * (size_t)n + q] = pz; }
        flag[q] = 0;
        if (q >= nn_prev) nn_cnt[q] = 0;
    }
    const double x = px, y = py, z = pz;
    const float ptx = (float)(((T[0] * x + T[3] * y) + T[6] * z) + T[9]);
    const float pty = (float)(((T[1] * x + T[4] * y) + T[7] * z) + T[10]);
    const float ptz = (float)(((T[2] * x + T[5] * y) + T[8] * z) + T[11]);
    const float fx = roundf(ptx * inv_res), fy = roundf(pty * inv_res), fz = roundf(ptz * inv_res);
    if (!(fabsf(fx) < (float)kKeyLimit && fabsf(fy) < (float)kKeyLimit && fabsf(fz) < (float)kKeyLimit)) return;  // beyond the key range: no voxel
    const int kx = (int)fx, ky = (int)fy, kz = (int)fz;

    // the voxel look-up of the image's form: {begin, count}, count = 0 on a miss
    bool have = false;
    unsigned cbase = 0u;
    if (DENSE) {  // brick image: one directory look-up, every probe a slab offset from the query's own cell (as ivox_knn_body)
        const int bx = kx >> kBrickLog, by = ky >> kBrickLog, bz = kz >> kBrickLog;
        const unsigned long long bkey = pack_key(bx, by, bz);
        unsigned h = brick_hash(bx, by, bz) & bd.mask;
        HashEntry be = bd.table[h];
        while (be.key != bkey && be.key != kEmptyKey) {
            h = (h + 1) & bd.mask;
            be = bd.table[h];
        }
        have = be.key == bkey && be.begin < bd.n_cap;
        cbase = (have ? be.begin : 0u) * kBrickStride +
                brick_slab_index((kx & (kBrickSide - 1)) + 1, (ky & (kBrickSide - 1)) + 1, (kz & (kBrickSide - 1)) + 1);
    }
    auto lookup = [&](const int vx, const int vy, const int vz, unsigned& begin, unsigned& count) {
        if (DENSE) {
            if (!have) { count = 0u; return; }
            const int off = ((vz - kz) * kBrickStored + (vy - ky)) * kBrickStored + (vx - kx);  // (always inside the slab)
            const uint2 e = bd.cells[cbase + (unsigned)off];
            begin = e.x;
            count = e.y;
        } else {
            const unsigned long long key = pack_key(vx, vy, vz);
            unsigned h = hash_key(key) & grid.mask;
            HashEntry ek = grid.table[h];
            while (ek.key != key && ek.key != kEmptyKey) {
                h = (h + 1) & grid.mask;
                ek = grid.table[h];
            }
            const bool hit = ek.key == key;
            begin = hit ? ek.begin : 0u;
            count = hit ? ek.count : 0u;
        }
    };
    auto map_pt = [&](const unsigned s) -> float4 {
        if (GEN) return grid.pts[s];
        return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(grid.pts) + (s << 4));  // (32-bit byte offset, as ivox_knn_body)
    };
    auto point = [&](const unsigned s, float& ox, float& oy, float& oz) {
        const float4 p = map_pt(s);
        ox = p.x; oy = p.y; oz = p.z;
    };

    const kro::Strided w{&work[threadIdx.x], kKnnRefQueries};
    int cnt = kro::closest_points(w, ptx, pty, ptz, kx, ky, kz, lookup, point);
    unsigned sid[5] = {~0u, ~0u, ~0u, ~0u, ~0u};
    if (cnt < 0) {
        // a voxel the work array cannot hold: the default order, the five smallest keys {d2 bits : slot} (named scalars: nothing indexed at run time)
        atomicAdd(fallbacks, 1ull);
        constexpr unsigned long long kNone = ~0ull;
        unsigned long long t0 = kNone, t1 = kNone, t2 = kNone, t3 = kNone, t4 = kNone;
        for (int k = 0; k < kro::kProbes; ++k) {
            int ox, oy, oz;
            kro::nearby18(k, ox, oy, oz);
            unsigned begin = 0u, count = 0u;
            lookup(kx + ox, ky + oy, kz + oz, begin, count);
            for (unsigned s = begin; s != begin + count; ++s) {
                const float4 p = map_pt(s);
                const float d2 = kro::dist2(p.x, p.y, p.z, ptx, pty, ptz);
                if (!(d2 < kro::kMaxRange2)) continue;
                unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | s, lo;
                lo = key < t0 ? key : t0; key = key < t0 ? t0 : key; t0 = lo;
                lo = key < t1 ? key : t1; key = key < t1 ? t1 : key; t1 = lo;
                lo = key < t2 ? key : t2; key = key < t2 ? t2 : key; t2 = lo;
                lo = key < t3 ? key : t3; key = key < t3 ? t3 : key; t3 = lo;
                t4 = key < t4 ? key : t4;
            }
        }
        cnt = (t0 != kNone) + (t1 != kNone) + (t2 != kNone) + (t3 != kNone) + (t4 != kNone);
        sid[0] = (unsigned)t0; sid[1] = (unsigned)t1; sid[2] = (unsigned)t2; sid[3] = (unsigned)t3; sid[4] = (unsigned)t4;  // (kNone's low word is ~0u)
    } else {
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (j < cnt) sid[j] = w[j].payload;
    }
    if (cnt == 0) return;  // no candidate: nothing is written (ivox_map.cpp:21-23)
    *reinterpret_cast<uint4*>(nn_ids + (size_t)q * 8) = make_uint4(sid[0], sid[1], sid[2], sid[3]);
    nn_ids[(size_t)q * 8 + 4] = sid[4];
    nn_cnt[q] = (unsigned char)cnt;
}

// the kNN launch of one iteration in reference order (match_launch; e0 / e1: the profiling events of the dispatch, or null)
inline void P2PlaneIvoxMatcher::launch_knn_reforder(const MatchPlan& m, const bool first, const float* src_x, const float* src_y, const float* src_z,
                                                    float* dev_copy, hipEvent_t e0, hipEvent_t e1) {
    const unsigned blocks = unsigned((m.n + size_t(kKnnRefQueries) - 1) / size_t(kKnnRefQueries));
    with_bools([&](auto DENSE, auto FIRST, auto GEN) {
        hipExtLaunchKernelGGL((ivox_knn_reforder_kernel<DENSE.value, FIRST.value, GEN.value>), dim3(blocks), dim3(kKnnRefQueries), 0, stream, e0, e1, 0,
                              src_x, src_y, src_z, int(m.n), (const GnState*)d_state.p, m.T0, m.v.g, m.v.win, m.v.inv_resolution, d_nn_cnt.p, d_flag.p,
                              d_nn_ids.p, nn_prev, dev_copy, d_ref_fallbacks.p);
    }, m.v.dense, first, m.v.general);
    ++n_ref_launches;
}

}  // namespace fls
