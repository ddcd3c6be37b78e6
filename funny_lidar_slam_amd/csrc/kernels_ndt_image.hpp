// kernels_ndt_image.hpp -- the flat image of the NDT voxel map (include/fls_map_ndt.h, ndt_image.hpp) written from and read into the device
// rows of kernels_ndt_update.hpp.
//   ndt_image_pack_kernel          rows, in the LRU order a stamp sort gave (ndt_evict_keys + DevicePairSort: alive rows first, oldest first),
//                                  gathered into the arrays of one contiguous image
//   ndt_image_check_unpack_kernel  the per-voxel checks of an import, and the arrays scattered into row buffers (row r = entry r, stamp r + 1)
//   ndt_table_rehash_check_kernel  ndt_table_rehash_kernel for keys nobody vouches for: a key met twice is reported, not probed past
// Both image kernels give every element of the wide fields (192 B of pending points, 72 B each of sigma and info, 24 B of mu per voxel) a
// lane of its own: consecutive lanes read consecutive doubles of a row and write consecutive doubles of the image (one lane walking a whole
// row would touch a new 64 B line of every array per step).  The index space is [narrow | points | mu | sigma | info]: n lanes for the five
// narrow fields, then 24 n, 3 n, 9 n and 9 n.
#pragma once
#include "kernels_ndt_update.hpp"
#include "ndt_image.hpp"

namespace fls {

static_assert(kNdtImageCarry == kNdtCarry, "an image entry carries what a device row carries");
constexpr int kNdtImageLanesPerVoxel = 1 + kNdtCarry * 3 + 3 + 9 + 9;  // 46

// reasons an import is refused for (bits of the status word)
constexpr unsigned kNdtImgBadKey = 1u, kNdtImgBadEstimated = 2u, kNdtImgBadPending = 4u, kNdtImgBadCount = 8u, kNdtImgBadVid = 16u, kNdtImgNotFinite = 32u,
                   kNdtImgDuplicateKey = 64u;

// offsets of ndt_image.hpp's layout as a launch argument
struct NdtImageOffsets {
    unsigned long long key, num_points, vid, estimated, pending, points, mu, sigma, info;
};
inline NdtImageOffsets ndt_image_offsets(const NdtImageLayout& L) {
    return NdtImageOffsets{L.key, L.num_points, L.vid, L.estimated, L.pending, L.points, L.mu, L.sigma, L.info};
}

// which field a lane serves: f = 0 narrow, 1 points, 2 mu, 3 sigma, 4 info; r = entry; e = element inside the entry's field
__device__ __forceinline__ void ndt_image_lane(const unsigned long long t, const unsigned long long n, int& f, unsigned long long& r, unsigned& e) {
    constexpr unsigned long long P = (unsigned long long)kNdtCarry * 3ull;
    if (t < n) { f = 0; r = t; e = 0u; return; }
    unsigned long long u = t - n;
    if (u < P * n) { f = 1; r = u / P; e = (unsigned)(u % P); return; }
    u -= P * n;
    if (u < 3ull * n) { f = 2; r = u / 3ull; e = (unsigned)(u % 3ull); return; }
    u -= 3ull * n;
    if (u < 9ull * n) { f = 3; r = u / 9ull; e = (unsigned)(u % 9ull); return; }
    u -= 9ull * n;
    f = 4; r = u / 9ull; e = (unsigned)(u % 9ull);
}

// image <- rows.  order[0, n): the alive rows, least recently touched first.  The image's padding is zero already (the caller cleared it).
__global__ void __launch_bounds__(256)
ndt_image_pack_kernel(const NdtRows R, const unsigned* __restrict__ order, const unsigned long long n, const int max_points, unsigned char* __restrict__ img,
                      const NdtImageOffsets o) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (t >= n * (unsigned long long)kNdtImageLanesPerVoxel) return;
    int f;
    unsigned long long r;
    unsigned e;
    ndt_image_lane(t, n, f, r, e);
    const size_t row = order[r];
    if (f == 0) {
        const int np = R.num_points[row];
        const unsigned char est = R.estimated[row] ? 1 : 0;
        const bool saturated = est && np > max_points;  // its list is never read again: no pending points (fls_debug_ndt_voxels' rule)
        ((unsigned long long*)(img + o.key))[r] = R.key[row];
        ((int*)(img + o.num_points))[r] = np;
        ((int*)(img + o.vid))[r] = R.vid[row];
        img[o.estimated + r] = est;
        img[o.pending + r] = saturated ? (unsigned char)0 : R.carry_cnt[row];
    } else if (f == 1) {
        const bool saturated = R.estimated[row] && R.num_points[row] > max_points;
        const unsigned cc = saturated ? 0u : (unsigned)R.carry_cnt[row];
        ((double*)(img + o.points))[r * (kNdtCarry * 3) + e] = e < 3u * cc ? R.carry[row * (kNdtCarry * 3) + e] : 0.0;
    } else if (f == 2) {
        ((double*)(img + o.mu))[r * 3 + e] = R.mu[row * 3 + e];
    } else if (f == 3) {
        ((double*)(img + o.sigma))[r * 9 + e] = R.sigma[row * 9 + e];
    } else {
        ((double*)(img + o.info))[r * 9 + e] = R.info[row * 9 + e];
    }
}

__device__ __forceinline__ bool ndt_image_finite(const double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and the infinities

// rows <- image, with the per-voxel checks (*status collects the reasons; the caller drops the rows unless it stays 0).  The rows take the
// entries in image order: row r = entry r, stamp r + 1; hslot comes from the table build, the touch words are cleared by the caller.
__global__ void __launch_bounds__(256)
ndt_image_check_unpack_kernel(const unsigned char* __restrict__ img, const NdtImageOffsets o, const unsigned long long n, const int max_points, const int next_vid,
                              const NdtRows R, unsigned* __restrict__ status) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (t >= n * (unsigned long long)kNdtImageLanesPerVoxel) return;
    int f;
    unsigned long long r;
    unsigned e;
    ndt_image_lane(t, n, f, r, e);
    unsigned bad = 0u;
    if (f == 0) {
        const unsigned long long key = ((const unsigned long long*)(img + o.key))[r];
        const int np = ((const int*)(img + o.num_points))[r], vid = ((const int*)(img + o.vid))[r];
        const unsigned char est = img[o.estimated + r], pend = img[o.pending + r];
        int kx, ky, kz;
        unpack_key(key, kx, ky, kz);
        // kEmptyKey, kNdtTombKey and kNdtDeadKey carry bit 63, which no packed key does
        if ((key >> 63) != 0ull || !(abs(kx) < kKeyLimit && abs(ky) < kKeyLimit && abs(kz) < kKeyLimit)) bad |= kNdtImgBadKey;
        if (est > 1) bad |= kNdtImgBadEstimated;
        if (pend > kNdtCarry || (pend > 0 && est == 1 && np > max_points)) bad |= kNdtImgBadPending;
        if (np < 0) bad |= kNdtImgBadCount;
        if (vid < 0 || vid >= next_vid) bad |= kNdtImgBadVid;
        R.key[r] = key;
        R.num_points[r] = np;
        R.vid[r] = vid;
        R.estimated[r] = est ? 1 : 0;
        R.carry_cnt[r] = pend > kNdtCarry ? (unsigned char)kNdtCarry : pend;
        R.stamp[r] = r + 1ull;
        R.hslot[r] = 0u;
    } else if (f == 1) {
        R.carry[r * (kNdtCarry * 3) + e] = ((const double*)(img + o.points))[r * (kNdtCarry * 3) + e];
    } else if (f == 2) {
        const double v = ((const double*)(img + o.mu))[r * 3 + e];
        if (img[o.estimated + r] && !ndt_image_finite(v)) bad |= kNdtImgNotFinite;
        R.mu[r * 3 + e] = v;
    } else if (f == 3) {
        R.sigma[r * 9 + e] = ((const double*)(img + o.sigma))[r * 9 + e];
    } else {
        const double v = ((const double*)(img + o.info))[r * 9 + e];
        if (img[o.estimated + r] && !ndt_image_finite(v)) bad |= kNdtImgNotFinite;
        R.info[r * 9 + e] = v;
    }
    if (bad) atomicOr(status, bad);
}

// ndt_table_rehash_kernel for rows read from an image: every row is alive, a key already in the table is reported.  It runs behind the
// per-voxel checks whatever they found (one status word, read once): the table holds more entries than rows, so every probe ends, and a
// reserved key only lands in a table that is dropped with its rows.
__global__ void __launch_bounds__(256)
ndt_table_rehash_check_kernel(HashEntry* __restrict__ table, const unsigned mask, const NdtRows r, const unsigned n_rows, unsigned* __restrict__ status) {
    const unsigned row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const unsigned long long key = r.key[row];
    unsigned h = hash_key(key) & mask;
    for (;;) {
        const unsigned long long old = atomicCAS(&table[h].key, kEmptyKey, key);
        if (old == kEmptyKey) break;
        if (old == key) { atomicOr(status, kNdtImgDuplicateKey); return; }
        h = (h + 1) & mask;
    }
    table[h].begin = row;
    table[h].count = r.estimated[row] ? 1u : 0u;
    r.hslot[row] = h;
}

}  // namespace fls
