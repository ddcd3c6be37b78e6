// knn_reference_order.hpp -- the neighbour selection of LoamPointToPlaneIVOX as the reference performs it, restated once for host and device.
//
// The reference selects a query's five neighbours with std::nth_element calls on records compared by distance alone
// (src/ivox_map/ivox_map.cpp:6-37, src/ivox_map/voxel_grid_node.cpp:23-42): which of several candidates at exactly the same distance is
// kept, and the order of slots 1..4 of a list, are whatever libstdc++'s introselect leaves behind.  This header restates that algorithm
// from its behaviour (as kernels_exactsort.hpp / host_parallel.hpp do for std::sort) and GetClosestPoint on top of it; the check is the
// toolchain's own std::nth_element (tests/host/knn_reference_order_model_test.cpp).
//
//   nth_element(a, n, nth)   introselect with depth limit 2 floor(lg n); median of three of (first + 1, mid, last - 1) moved to first,
//                            unguarded partition around it; ranges of <= 3 insertion-sorted; at depth 0 heap-select of [first, nth + 1)
//                            over the range and a swap of first and nth
//   closest_points(...)      the 19 NEARBY18 voxels in the reference's order; per hit voxel every point in slot (= insertion) order with
//                            d2 < max_range^2 is pushed, more than old + 5 held -> nth_element(old, old + 4, end), keep old + 5; at the end
//                            more than 5 held -> nth_element(0, 4, end), keep 5; then nth_element(0, 0, end)
//
// No HIP runtime call, no allocation: the work array is the caller's, reached through any type with operator[] that yields Rec& (a plain
// pointer on the host, a strided view of LDS on the device); the voxel look-up and the point fetch are the caller's too.
#pragma once

#if defined(__HIPCC__)
#define FLS_KRO_FN __host__ __device__ inline
#else
#define FLS_KRO_FN inline
#endif

namespace fls {
namespace kro {

struct Rec {
    float d2;          // the only thing compared
    unsigned payload;  // map slot (device), any tag (tests)
};

constexpr int kK = 5;            // neighbours kept (NUM_MATCH_POINTS)
constexpr int kProbes = 19;      // NEARBY18 + the centre
constexpr int kWork = 256;       // W: records of one query's work array
constexpr int kVoxelLimit = kWork - kK * (kProbes - 1);  // a voxel of more points than this cannot be held behind 18 truncated ones
constexpr float kMaxRange2 = 25.0f;  // max_range 5.0 squared
static_assert(kWork >= 256 && kVoxelLimit > kK, "the per-query limit W");

// NEARBY18 (ivox_map.cpp:50-54), 2 bits per entry (value + 1): the packing of kernels_ivox_coop.hpp::nearby18
FLS_KRO_FN constexpr void nearby18(const int k, int& dx, int& dy, int& dz) {
    constexpr unsigned long long DX = 0x1548889561ull, DY = 0x895429495ull, DZ = 0x282956155ull;
    dx = (int)((DX >> (2 * k)) & 3ull) - 1;
    dy = (int)((DY >> (2 * k)) & 3ull) - 1;
    dz = (int)((DZ >> (2 * k)) & 3ull) - 1;
}

// a view of every `stride`-th record from `base` on (the device keeps record j of lane l at work[j * lanes + l])
struct Strided {
    Rec* base;
    int stride;
    FLS_KRO_FN Rec& operator[](const int i) const { return base[i * stride]; }
};

template <class A>
FLS_KRO_FN void swap_rec(A a, const int i, const int j) {
    const Rec t = a[i];
    a[i] = a[j];
    a[j] = t;
}

// [first, last) sorted by insertion: an element below the first goes to the front by a block move, any other sinks unguarded
template <class A>
FLS_KRO_FN void insertion_sort(A a, const int first, const int last) {
    if (first == last) return;
    for (int i = first + 1; i != last; ++i) {
        const Rec v = a[i];
        if (v.d2 < a[first].d2) {
            for (int j = i; j > first; --j) a[j] = a[j - 1];
            a[first] = v;
        } else {
            int j = i;
            while (v.d2 < a[j - 1].d2) {
                a[j] = a[j - 1];
                --j;
            }
            a[j] = v;
        }
    }
}

// max-heap on [first, first + len): the hole sinks along the larger children to a leaf, then `v` rises from there
template <class A>
FLS_KRO_FN void adjust_heap(A a, const int first, int hole, const int len, const Rec v) {
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (a[first + child].d2 < a[first + child - 1].d2) --child;
        a[first + hole] = a[first + child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        a[first + hole] = a[first + child - 1];
        hole = child - 1;
    }
    int parent = (hole - 1) / 2;
    while (hole > top && a[first + parent].d2 < v.d2) {
        a[first + hole] = a[first + parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    a[first + hole] = v;
}

// the `middle - first` smallest of [first, last) into the heap [first, middle)
template <class A>
FLS_KRO_FN void heap_select(A a, const int first, const int middle, const int last) {
    const int len = middle - first;
    if (len >= 2) {
        for (int parent = (len - 2) / 2;; --parent) {
            adjust_heap(a, first, parent, len, a[first + parent]);
            if (parent == 0) break;
        }
    }
    for (int i = middle; i < last; ++i) {
        if (a[i].d2 < a[first].d2) {
            const Rec v = a[i];
            a[i] = a[first];
            adjust_heap(a, first, 0, len, v);
        }
    }
}

// the median of a[x], a[y], a[z] swapped into a[result]
template <class A>
FLS_KRO_FN void move_median_to_first(A a, const int result, const int x, const int y, const int z) {
    const float fx = a[x].d2, fy = a[y].d2, fz = a[z].d2;
    int m;
    if (fx < fy) m = fy < fz ? y : fx < fz ? z : x;
    else m = fx < fz ? x : fy < fz ? z : y;
    swap_rec(a, result, m);
}

// std::nth_element(a + first, a + nth, a + last) of libstdc++; *depth_hits (may be null) counts the calls that reached the depth-limit branch
template <class A>
FLS_KRO_FN void nth_element(A a, int first, const int nth, int last, int* depth_hits = nullptr) {
    if (first == last || nth == last) return;
    int depth = 0;
    for (unsigned n = (unsigned)(last - first); n > 1u; n >>= 1) ++depth;  // floor(lg n)
    depth *= 2;
    while (last - first > 3) {
        if (depth == 0) {
            heap_select(a, first, nth + 1, last);
            swap_rec(a, first, nth);
            if (depth_hits) ++*depth_hits;
            return;
        }
        --depth;
        move_median_to_first(a, first, first + 1, first + (last - first) / 2, last - 1);
        const float pivot = a[first].d2;  // (the pivot's record stays at `first` through the partition)
        int lo = first + 1, hi = last;
        for (;;) {
            while (a[lo].d2 < pivot) ++lo;
            --hi;
            while (pivot < a[hi].d2) --hi;
            if (!(lo < hi)) break;
            swap_rec(a, lo, hi);
            ++lo;
        }
        if (lo <= nth) first = lo;
        else last = lo;
    }
    insertion_sort(a, first, last);
}

// d2 of a candidate as the reference's float squaredNorm evaluates it
FLS_KRO_FN float dist2(const float px, const float py, const float pz, const float qx, const float qy, const float qz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return dx * dx + (dy * dy + dz * dz);
}

// IVoxMap::GetClosestPoint for the query (qx, qy, qz) of voxel (kx, ky, kz).
//   lookup(vx, vy, vz, begin, count)  the voxel's slot range; count = 0 where the map has no such voxel
//   point(slot, x, y, z)              the map point in a slot
// Returns the number of neighbours (0..5), their records in work[0, n) in the reference's order; 0 = no candidate (the caller writes nothing).
// -1: a probed voxel holds more than kVoxelLimit points, the work array cannot be guaranteed to hold the query: nothing is selected.
template <class A, class Lookup, class Point>
FLS_KRO_FN int closest_points(A work, const float qx, const float qy, const float qz, const int kx, const int ky, const int kz, Lookup&& lookup,
                              Point&& point) {
    int held = 0;
    for (int k = 0; k < kProbes; ++k) {
        int ox, oy, oz;
        nearby18(k, ox, oy, oz);
        unsigned begin = 0u, count = 0u;
        lookup(kx + ox, ky + oy, kz + oz, begin, count);
        if (count == 0u) continue;
        if (count > (unsigned)kVoxelLimit) return -1;
        const int old = held;  // (<= 5 per voxel probed so far: old + count <= kWork)
        for (unsigned s = begin; s != begin + count; ++s) {
            float x, y, z;
            point(s, x, y, z);
            const float d2 = dist2(x, y, z, qx, qy, qz);
            if (d2 < kMaxRange2) {
                work[held] = Rec{d2, s};
                ++held;
            }
        }
        if (held > old + kK) {
            nth_element(work, old, old + kK - 1, held);
            held = old + kK;
        }
    }
    if (held == 0) return 0;
    if (held > kK) {
        nth_element(work, 0, kK - 1, held);
        held = kK;
    }
    nth_element(work, 0, 0, held);
    return held;
}

}  // namespace kro
}  // namespace fls
