// kernels_ivox_build.hpp -- the iVox map built from a whole cloud on the device: what IVoxMap::AddPoints (src/ivox_map/ivox_map.cpp:122-143)
// followed by IvoxImage::build_from_ivox leaves when the cloud goes into an EMPTY map and no LRU eviction happens ("closed form"):
//   * the voxels are the distinct keys; a voxel's points are its members in cloud order, ids = cloud indices
//   * the image holds the voxels in (brick z, y, x, then z, y, x) order, each in a region of cap_for(count) slots, back to back from slot 0
//   * LRU order = order of the voxels' LAST members: the stamp of a voxel is that index + 1
// so the build is a stable sort of (brick-major voxel key, cloud index) and a few scans.  IvoxMap::bulk_build drives it:
//   ivb_keys     <n>   voxel key + sort key per point (extent-relative, so the radix sort runs only the passes the extent has bits for); range flag
//   DevicePairSort     stable LSD radix sort (a key wider than 32 bits takes a second round on ivb_gather_hi's keys)
//   ivb_heads    <n>   segment heads and own-brick heads, block-local prefixes + block totals      -> vg_scan over the totals
//   ivb_voxels   <n>   voxel index per sorted position, first position per voxel
//   ivb_caps     <n>   per voxel: count, region capacity, block-local prefix + block totals        -> vg_scan over the totals
//   ivb_report   <1>   {flag, V, used, own bricks} to the host-mapped mailbox: the one host wait (declines, point array and brick pool sizes)
//   ivb_cells    <n>   per voxel: its bricks found or created (brick_find_or_create), cell record + halo mirrors, capacity, stamp (ivb_cell_write)
//   ivb_points   <n>   points into their regions, slack filled
// The per-position launches are sized by n (the host does not know V before the mailbox); threads beyond V leave at once.
#pragma once
#include "kernels_ivox_update.hpp"
#include "kernels_voxelgrid.hpp"

namespace fls {

constexpr int kIvbBlock = 256;

// where the bricks of the cloud start and how many bits each brick axis needs: the sort key is
// (((bz * 2^by_bits + by) * 2^bx_bits + bx) << 9) | lz << 6 | ly << 3 | lx   with b = brick coordinate - bmin, l = voxel inside the brick
struct IvbExtent { int bmin[3]; int bx_bits, by_bits; };

struct IvbMailbox { unsigned flag, n_voxels, own_bricks, seq; unsigned long long used; };

__global__ void __launch_bounds__(kIvbBlock)
ivb_keys(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const int n, const float inv_res, const IvbExtent e,
         unsigned long long* __restrict__ vkey, unsigned* __restrict__ klo, unsigned* __restrict__ khi /* null: the key fits 32 bits */,
         unsigned* __restrict__ val, unsigned* __restrict__ flag) {
    const int i = blockIdx.x * kIvbBlock + threadIdx.x;
    if (i >= n) return;
    // IVoxMap::Pos2Grid (ivox_map.cpp:145-147) as HostIvox::key_of evaluates it: round half away from zero of the float product
    const float fx = roundf(x[i] * inv_res), fy = roundf(y[i] * inv_res), fz = roundf(z[i] * inv_res);
    const bool ok = fabsf(fx) < (float)kKeyLimit && fabsf(fy) < (float)kKeyLimit && fabsf(fz) < (float)kKeyLimit;  // (false for NaN)
    if (!ok) atomicOr(flag, 1u);  // (the whole build is declined: the host path reports FLS_ERR_RANGE)
    const int kx = ok ? (int)fx : 0, ky = ok ? (int)fy : 0, kz = ok ? (int)fz : 0;
    const unsigned long long bx = (unsigned)((kx >> kBrickLog) - e.bmin[0]), by = (unsigned)((ky >> kBrickLog) - e.bmin[1]), bz = (unsigned)((kz >> kBrickLog) - e.bmin[2]);
    const unsigned local = (unsigned)(((kz & (kBrickSide - 1)) << (2 * kBrickLog)) | ((ky & (kBrickSide - 1)) << kBrickLog) | (kx & (kBrickSide - 1)));
    const unsigned long long sk = ((((bz << e.by_bits) | by) << e.bx_bits | bx) << (3 * kBrickLog)) | local;
    vkey[i] = pack_key(kx, ky, kz);
    klo[i] = (unsigned)sk;
    if (khi != nullptr) khi[i] = (unsigned)(sk >> 32);
    val[i] = (unsigned)i;
}

// second sort round of a wide key: the high words in the order the first round left
__global__ void __launch_bounds__(kIvbBlock)
ivb_gather_hi(const unsigned* __restrict__ khi, const unsigned* __restrict__ order, const int n, unsigned* __restrict__ key) {
    const int j = blockIdx.x * kIvbBlock + threadIdx.x;
    if (j < n) key[j] = khi[order[j]];
}

__device__ __forceinline__ unsigned long long ivb_brick_of(const unsigned long long vkey) {  // the packed key with the voxel-in-brick bits cleared
    return vkey & ~((7ull << 42) | (7ull << 21) | 7ull);
}

// sorted position j: does a voxel start here, does a brick start here.  lx: block-local exclusive counts; bt: block totals, voxel heads in
// [0, nblk), brick heads in [nblk, 2 nblk) -- one scan over both planes gives V at the seam
__global__ void __launch_bounds__(kIvbBlock)
ivb_heads(const unsigned long long* __restrict__ vkey, const unsigned* __restrict__ order, const int n, uint2* __restrict__ lx, unsigned* __restrict__ bt) {
    __shared__ unsigned wsum[kIvbBlock / 64][2];
    const int j = blockIdx.x * kIvbBlock + threadIdx.x;
    unsigned v[2] = {0u, 0u}, tot[2];
    if (j < n) {
        const unsigned long long k = vkey[order[j]], kp = j > 0 ? vkey[order[j - 1]] : ~0ull;  // (~0 is no packed key: 63 bits)
        v[0] = k != kp ? 1u : 0u;
        v[1] = (j == 0 || ivb_brick_of(k) != ivb_brick_of(kp)) ? 1u : 0u;
    }
    const unsigned head = v[0];
    block_excl_scan<2>(v, tot, wsum);
    if (j < n) lx[j] = make_uint2(v[0] | (head << 31), v[1]);
    if (threadIdx.x == 0) { bt[blockIdx.x] = tot[0]; bt[gridDim.x + blockIdx.x] = tot[1]; }
}

// voxel index of every sorted position; first position of every voxel (first[V] = n closes the last segment)
__global__ void __launch_bounds__(kIvbBlock)
ivb_voxels(const uint2* __restrict__ lx, const unsigned* __restrict__ bts /* scanned */, const int n, unsigned* __restrict__ vidx, unsigned* __restrict__ first) {
    const int j = blockIdx.x * kIvbBlock + threadIdx.x;
    if (j >= n) return;
    const unsigned l = lx[j].x, head = l >> 31;
    const unsigned v = bts[blockIdx.x] + (l & 0x7fffffffu) + head - 1u;  // (position 0 is a head: never underflows)
    vidx[j] = v;
    if (head) first[v] = (unsigned)j;
    if (j == n - 1) first[v + 1u] = (unsigned)n;
}

// per voxel: region capacity, block-local exclusive prefix and block totals of the capacities
__global__ void __launch_bounds__(kIvbBlock)
ivb_caps(const unsigned* __restrict__ first, const unsigned* __restrict__ n_voxels, unsigned* __restrict__ lcap, unsigned* __restrict__ btc) {
    __shared__ unsigned wsum[kIvbBlock / 64][1];
    const unsigned v = blockIdx.x * kIvbBlock + threadIdx.x, V = *n_voxels;
    unsigned c[1] = {v < V ? upd_cap_for(first[v + 1u] - first[v]) : 0u}, tot[1];
    block_excl_scan<1>(c, tot, wsum);
    if (v < V) lcap[v] = c[0];
    if (threadIdx.x == 0) btc[blockIdx.x] = tot[0];
}

__global__ void ivb_report(const unsigned* __restrict__ flag, const unsigned* __restrict__ n_voxels, const unsigned* __restrict__ heads_total,
                           const unsigned* __restrict__ used, IvbMailbox* __restrict__ mb, const unsigned seq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    __hip_atomic_store(&mb->flag, *flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&mb->n_voxels, *n_voxels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&mb->own_bricks, *heads_total - *n_voxels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&mb->used, (unsigned long long)*used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(&mb->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// one voxel: its own brick and the neighbours whose halo mirrors it exist from here on (created empty if need be: the pool is pre-zeroed);
// its cell record {begin, count} in the primary cell and the mirrors; region capacity; LRU stamp.  A full pool or directory raises
// kUpdArrayFull in the state (the host grows the pool and runs the launch again).
__device__ __forceinline__ void ivb_cell_write(const IvoxUpdArrays& a, IvoxUpdState* __restrict__ st, const unsigned long long key, const unsigned begin,
                                               const unsigned cnt, const unsigned long long stamp) {
    int kx, ky, kz;
    unpack_key(key, kx, ky, kz);
    const int bx = kx >> kBrickLog, by = ky >> kBrickLog, bz = kz >> kBrickLog;
    const int lx = kx & (kBrickSide - 1), ly = ky & (kBrickSide - 1), lz = kz & (kBrickSide - 1);
    const unsigned bi = brick_find_or_create(a, st, bx, by, bz);
    if (bi >= a.n_bricks_cap) return;  // (kUpdArrayFull is raised)
    bool all = true;
    unsigned* const row = a.nbr + (size_t)bi * 32u;
    brick_for_each_mirror(lx, ly, lz, [&](const int dx, const int dy, const int dz) {
        const unsigned nb = brick_find_or_create(a, st, bx + dx, by + dy, bz + dz);
        if (nb < a.n_bricks_cap) row[brick_nbr_code(dx, dy, dz)] = nb; else all = false;
    });
    if (!all) return;
    const unsigned cell = bi * kBrickStride + brick_slab_index(lx + 1, ly + 1, lz + 1);
    const uint2 rec = make_uint2(begin, cnt);
    a.cells[cell] = rec;
    brick_write_mirrors(a, cell, rec);
    a.cap_log2[cell] = (unsigned char)upd_log2(upd_cap_for(cnt));
    a.stamp[cell] = stamp;
}
// voxel v of the sorted cloud: LRU stamp = index of its last member + 1 (the voxels of a blob bring their own counts and stamps:
// kernels_ivox_blob.hpp's ivbl_cells)
__global__ void __launch_bounds__(kIvbBlock)
ivb_cells(const unsigned long long* __restrict__ vkey, const unsigned* __restrict__ order, const unsigned* __restrict__ first, const unsigned n_voxels,
          const unsigned* __restrict__ lcap, const unsigned* __restrict__ btcs /* scanned */, const IvoxUpdArrays a, IvoxUpdState* __restrict__ st,
          unsigned* __restrict__ vbegin) {
    const unsigned v = blockIdx.x * kIvbBlock + threadIdx.x;
    if (v >= n_voxels) return;
    const unsigned f = first[v], cnt = first[v + 1u] - f, begin = btcs[blockIdx.x] + lcap[v];
    vbegin[v] = begin;
    ivb_cell_write(a, st, vkey[order[f]], begin, cnt, (unsigned long long)order[f + cnt - 1u] + 1ull);  // (stable sort: the last member of the segment is the last inserted)
}

// sorted position j -> its slot; the first member of a voxel also fills the region's slack
__global__ void __launch_bounds__(kIvbBlock)
ivb_points(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const unsigned* __restrict__ order, const int n,
           const unsigned* __restrict__ vidx, const unsigned* __restrict__ first, const unsigned* __restrict__ vbegin, float4* __restrict__ pts,
           const unsigned long long pts_cap) {
    const int j = blockIdx.x * kIvbBlock + threadIdx.x;
    if (j >= n) return;
    const unsigned v = vidx[j], f = first[v], begin = vbegin[v], i = order[j];
    const unsigned long long slot = (unsigned long long)begin + ((unsigned)j - f);
    if (slot < pts_cap) pts[slot] = make_float4(x[i], y[i], z[i], __int_as_float((int)i));
    if ((unsigned)j == f) {
        const unsigned cnt = first[v + 1u] - f, cap = upd_cap_for(cnt);
        for (unsigned k = cnt; k < cap; ++k)
            if ((unsigned long long)begin + k < pts_cap) pts[begin + k] = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    }
}

}  // namespace fls
