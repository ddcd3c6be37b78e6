// kernels_ivox_blob.hpp -- the FLSIVOX1 blob (include/fls_map_ivox.h) packed from and unpacked into the device image of the iVox map, without the
// host mirror.  IvoxMap::export_blob_device / import_blob_device (ivox_map.hpp) drive the launches; the stable radix sort and the one-workgroup
// scan are the bulk build's (DevicePairSort, vg_scan).
//
// Export (the image is the map, the stream idle):
//   ivox_list_alive_kernel   the alive voxels as {key, begin, count, cap_log2, stamp}, in any order (kernels_ivox_update.hpp)
//   ivbx_stamp_keys   <V>    low words of the stamps as sort keys      -> DevicePairSort (ivbx_stamp_hi + a second stable round for stamps beyond 2^32)
//   ivbx_counts       <V>    counts in LRU order, block-local prefixes + block totals    -> vg_scan over the totals
//   ivbx_pack         <8 V>  eight lanes per voxel: the voxel record, then its `count` rows gathered from pts[begin ..]
// Import (nothing of the handle changes before the host has read the report of the checks):
//   ivbl_check        <V>    per record: count >= 1 and <= n_points, the key canonical; brick extent; sum of the counts; source prefixes + block totals -> vg_scan
//   ivbl_keys         <V>    brick-major sort key relative to the extent, value = blob position   -> DevicePairSort (ivb_gather_hi for a wide key)
//   ivbl_layout       <V>    sorted neighbours with equal keys (a voxel listed twice), own-brick heads, capacities: prefixes + block totals -> vg_scan
//   ivbl_cells        <V>    per voxel in layout order: bricks, cell record + halo mirrors, capacity, stamp = blob position + 1 (ivb_cell_write)
//   ivbl_points       <8 V>  eight lanes per voxel in blob order: its rows from the blob into its region, slack filled
// The records sit in a staging buffer shifted by 8 bytes against the blob (its header is 56 bytes), so every access below is a 16-byte one.
#pragma once
#include "kernels_ivox_build.hpp"
#include "ivox_blob.hpp"
#include <climits>

namespace fls {

constexpr int kIvblLanes = 8;  // lanes that move one voxel's rows
enum : unsigned { kIvblZeroCount = 1u, kIvblBadKey = 2u, kIvblDuplicate = 4u, kIvblBadCount = 8u };

// what the checks of an import, and the totals of an export, leave for the host (one small copy)
struct IvblReport {
    unsigned flag, own_bricks, used, n_listed;
    unsigned long long count_sum;
    int bmin[3], bmax[3];
};

__device__ __forceinline__ unsigned ivbl_count_of(const ulonglong2 r) { return (unsigned)r.y; }  // {key, count | pad << 32}

// ---- export ----
__global__ void __launch_bounds__(kIvbBlock)
ivbx_stamp_keys(const IvoxAliveRec* __restrict__ rec, const unsigned n, unsigned* __restrict__ klo, unsigned* __restrict__ val) {
    const unsigned i = blockIdx.x * kIvbBlock + threadIdx.x;
    if (i >= n) return;
    klo[i] = (unsigned)rec[i].stamp;
    val[i] = i;
}
__global__ void __launch_bounds__(kIvbBlock)
ivbx_stamp_hi(const IvoxAliveRec* __restrict__ rec, const unsigned* __restrict__ order, const unsigned n, unsigned* __restrict__ key) {
    const unsigned j = blockIdx.x * kIvbBlock + threadIdx.x;
    if (j < n) key[j] = (unsigned)(rec[order[j]].stamp >> 32);
}
__global__ void __launch_bounds__(kIvbBlock)
ivbx_counts(const IvoxAliveRec* __restrict__ rec, const unsigned* __restrict__ order, const unsigned n, unsigned* __restrict__ lx, unsigned* __restrict__ bt,
            IvblReport* __restrict__ rep) {
    __shared__ unsigned wsum[kIvbBlock / 64][1];
    const unsigned j = blockIdx.x * kIvbBlock + threadIdx.x;
    unsigned c[1] = {j < n ? rec[order[j]].count : 0u}, tot[1];
    block_excl_scan<1>(c, tot, wsum);
    if (j < n) lx[j] = c[0];
    if (threadIdx.x == 0) { bt[blockIdx.x] = tot[0]; atomicAdd(&rep->count_sum, (unsigned long long)tot[0]); }
}
// voxel j of the LRU order (oldest first): record j of the blob, its rows behind those of the voxels before it.  Nothing is written beyond
// n_points rows, nothing read beyond the point array, whatever the records say (the host compares the totals before it hands the blob out).
__global__ void __launch_bounds__(kIvbBlock)
ivbx_pack(const IvoxAliveRec* __restrict__ rec, const unsigned* __restrict__ order, const unsigned n, const unsigned* __restrict__ lx,
          const unsigned* __restrict__ bts /* scanned */, const float4* __restrict__ pts, const unsigned long long pts_cap, ulonglong2* __restrict__ out_vox,
          float4* __restrict__ out_pts, const unsigned long long n_points) {
    const unsigned g = blockIdx.x * kIvbBlock + threadIdx.x, j = g / kIvblLanes, sub = g % kIvblLanes;
    if (j >= n) return;
    const IvoxAliveRec r = rec[order[j]];
    const unsigned long long dst = (unsigned long long)bts[j / kIvbBlock] + lx[j];
    if (sub == 0u) out_vox[j] = make_ulonglong2(r.key, (unsigned long long)r.count);
    for (unsigned k = sub; k < r.count; k += kIvblLanes)
        if ((unsigned long long)r.begin + k < pts_cap && dst + k < n_points) out_pts[dst + k] = pts[r.begin + k];
}

// ---- import ----
__device__ __forceinline__ int ivbl_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ int ivbl_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}
// record k: its count and key checked, the brick extent of the canonical keys, the sum of the counts in 64 bits, and the exclusive prefix of
// the counts (where voxel k's rows start in the blob).  A count beyond n_points cannot be part of a valid blob: it is flagged and left out of
// the prefixes, so that no 32-bit block total wraps (256 counts of at most 2^22).
__global__ void __launch_bounds__(kIvbBlock)
ivbl_check(const ulonglong2* __restrict__ vox, const unsigned n, const unsigned long long n_points, unsigned* __restrict__ lsrc, unsigned* __restrict__ bt,
           IvblReport* __restrict__ rep) {
    __shared__ unsigned wsum[kIvbBlock / 64][1];
    const unsigned k = blockIdx.x * kIvbBlock + threadIdx.x;
    const bool in = k < n;
    const ulonglong2 r = in ? vox[k] : make_ulonglong2(0ull, 0ull);
    unsigned cnt = ivbl_count_of(r), flag = 0u;
    if (in && cnt == 0u) flag |= kIvblZeroCount;
    if (in && (unsigned long long)cnt > n_points) { flag |= kIvblBadCount; cnt = 0u; }
    int x = 0, y = 0, z = 0;
    const bool canon = in && ivox_key_canonical(r.x, x, y, z);
    if (in && !canon) flag |= kIvblBadKey;
    int lo[3], hi[3];
    lo[0] = canon ? x >> kBrickLog : INT_MAX; lo[1] = canon ? y >> kBrickLog : INT_MAX; lo[2] = canon ? z >> kBrickLog : INT_MAX;
    hi[0] = canon ? x >> kBrickLog : INT_MIN; hi[1] = canon ? y >> kBrickLog : INT_MIN; hi[2] = canon ? z >> kBrickLog : INT_MIN;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = ivbl_wave_min(lo[a]);
        hi[a] = ivbl_wave_max(hi[a]);
        if (lane == 0 && lo[a] != INT_MAX) { atomicMin(&rep->bmin[a], lo[a]); atomicMax(&rep->bmax[a], hi[a]); }
    }
    if (flag != 0u) atomicOr(&rep->flag, flag);
    unsigned c[1] = {cnt}, tot[1];
    block_excl_scan<1>(c, tot, wsum);
    if (in) lsrc[k] = c[0];
    if (threadIdx.x == 0) { bt[blockIdx.x] = tot[0]; atomicAdd(&rep->count_sum, (unsigned long long)tot[0]); }
}

__global__ void __launch_bounds__(kIvbBlock)
ivbl_keys(const ulonglong2* __restrict__ vox, const unsigned n, const IvbExtent e, unsigned* __restrict__ klo, unsigned* __restrict__ khi /* null: the key fits 32 bits */,
          unsigned* __restrict__ val) {
    const unsigned k = blockIdx.x * kIvbBlock + threadIdx.x;
    if (k >= n) return;
    int x, y, z;
    unpack_key(vox[k].x, x, y, z);
    const unsigned long long sk = ivox_brick_major_key(x, y, z, e.bmin[0], e.bmin[1], e.bmin[2], e.bx_bits, e.by_bits);
    klo[k] = (unsigned)sk;
    if (khi != nullptr) khi[k] = (unsigned)(sk >> 32);
    val[k] = k;
}

// layout position j (the voxels sorted brick-major; order[j] = blob position): two neighbours with one key are a voxel listed twice (the sort
// key is a bijection of the canonical keys inside the extent); own-brick heads; region capacities as block-local prefixes + block totals
__global__ void __launch_bounds__(kIvbBlock)
ivbl_layout(const ulonglong2* __restrict__ vox, const unsigned* __restrict__ order, const unsigned n, unsigned* __restrict__ lcap, unsigned* __restrict__ btc,
            IvblReport* __restrict__ rep) {
    __shared__ unsigned wsum[kIvbBlock / 64][2];
    const unsigned j = blockIdx.x * kIvbBlock + threadIdx.x;
    unsigned v[2] = {0u, 0u}, tot[2];
    if (j < n) {
        const ulonglong2 r = vox[order[j]];
        const unsigned long long kp = j > 0u ? vox[order[j - 1u]].x : ~0ull;  // (~0 is no packed key: 63 bits)
        if (r.x == kp) atomicOr(&rep->flag, kIvblDuplicate);
        v[0] = upd_cap_for(ivbl_count_of(r));
        v[1] = (j == 0u || ivb_brick_of(r.x) != ivb_brick_of(kp)) ? 1u : 0u;
    }
    block_excl_scan<2>(v, tot, wsum);
    if (j < n) lcap[j] = v[0];
    if (threadIdx.x == 0) { btc[blockIdx.x] = tot[0]; atomicAdd(&rep->own_bricks, tot[1]); }
}

// ivb_cells with the voxels given: count from the record, LRU stamp = blob position + 1.  vbegin is indexed by BLOB position (ivbl_points walks the blob).
__global__ void __launch_bounds__(kIvbBlock)
ivbl_cells(const ulonglong2* __restrict__ vox, const unsigned* __restrict__ order, const unsigned n, const unsigned* __restrict__ lcap,
           const unsigned* __restrict__ btcs /* scanned */, const IvoxUpdArrays a, IvoxUpdState* __restrict__ st, unsigned* __restrict__ vbegin) {
    const unsigned j = blockIdx.x * kIvbBlock + threadIdx.x;
    if (j >= n) return;
    const unsigned k = order[j], begin = btcs[blockIdx.x] + lcap[j];
    const ulonglong2 r = vox[k];
    vbegin[k] = begin;
    ivb_cell_write(a, st, r.x, begin, ivbl_count_of(r), (unsigned long long)k + 1ull);
}

// voxel k of the blob: its rows into its region, the slack rows {0, 0, 0, -1} behind them
__global__ void __launch_bounds__(kIvbBlock)
ivbl_points(const ulonglong2* __restrict__ vox, const float4* __restrict__ rows, const unsigned n, const unsigned long long n_points, const unsigned* __restrict__ lsrc,
            const unsigned* __restrict__ bts /* scanned */, const unsigned* __restrict__ vbegin, float4* __restrict__ pts, const unsigned long long pts_cap) {
    const unsigned g = blockIdx.x * kIvbBlock + threadIdx.x, k = g / kIvblLanes, sub = g % kIvblLanes;
    if (k >= n) return;
    const unsigned cnt = ivbl_count_of(vox[k]), cap = upd_cap_for(cnt), begin = vbegin[k];
    const unsigned long long src = (unsigned long long)bts[k / kIvbBlock] + lsrc[k];
    for (unsigned q = sub; q < cap; q += kIvblLanes) {
        const unsigned long long slot = (unsigned long long)begin + q;
        if (slot >= pts_cap) break;
        pts[slot] = (q < cnt && src + q < n_points) ? rows[src + q] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    }
}

}  // namespace fls
