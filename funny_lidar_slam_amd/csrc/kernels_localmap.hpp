// kernels_localmap.hpp -- the kernels of the device local-map source (include/fls_localmap.h, host side: localmap.hpp): the crop box of
// Localization::LoadLocalMap over the resident global map, SplitMap::Split's stable partition into tiles, the stitch of the resident tiles
// and the coordinate bounds of a cloud that goes into the iVox map without visiting the host.
//
// All of them are streaming passes over x | y | z | intensity planes: no reuse, no arithmetic to speak of; the work is the launch count and
// keeping every load and store of a wave one contiguous run.  The planes start at arbitrary multiples of 4 bytes (a plane's offset is
// the cloud's point count), so an access stays at one float per lane and plane, kLmPerThread of them in flight per lane, as in kf_merge_kernel.
//
//   crop     lm_crop_count (kept points per tile of kLmTile points: ballot + popcount) -> lm_scan_counts (one workgroup: exclusive scan of
//            the tile counts, the total) -> lm_crop_scatter (the same predicate again; a kept point's place is its tile's offset + the
//            counts of the wave-rows before it in the tile + the kept lanes below it).  The block -> output mapping is fixed by the scan:
//            no look-back between workgroups, no atomic decides an order.
//   split    lm_tile_minmax (tile indices in double, their bounds, the range check) -> lm_tile_keys (biased key gx' * span_y + gy', value =
//            point index) -> DevicePairSort (stable) -> lm_tile_heads (run detection: {key, first position} appended per run; the host
//            sorts the few runs by key, so the append order is immaterial) -> lm_gather4 (the four planes in tile order)
//   stitch   lm_stitch: kf_merge_kernel without the transform, one launch over a segment table built on the host
//   bounds   lm_bounds: min / max of three planes, one launch (ordered-uint atomics on six words zeroed beforehand)
#pragma once
#include "device_common.hpp"
#include "host_util.hpp"
#include "kernels_voxelgrid.hpp"  // vg_ord / vg_unord

namespace fls {

constexpr int kLmThreads = 256;
constexpr int kLmPerThread = 4;
constexpr int kLmWaves = kLmThreads / 64;
constexpr unsigned kLmTile = unsigned(kLmThreads) * kLmPerThread;  // points per workgroup
constexpr int kLmScanThreads = 1024;
constexpr int kLmWindow = 64;       // stitch: segments staged in LDS at a time
constexpr int kLmMaxBlocks = 2048;  // grid-stride passes (the reductions)

// the crop box: the six edges (double) cast to float, as CropBox::setMin / setMax get them
struct LmBox { float mn[3], mx[3]; };

// pcl::CropBox's test (no transform, not negative): a point exactly on a face is kept
__host__ __device__ __forceinline__ bool lm_in_box(const LmBox& b, const float x, const float y, const float z) {
    return !(x < b.mn[0] || y < b.mn[1] || z < b.mn[2] || x > b.mx[0] || y > b.mx[1] || z > b.mx[2]);
}

// SplitMap::Split / LoadLocalMap: floor((v - grid_size / 2) / grid_size) in double.  false: the index does not fit an int (or v is not finite)
__host__ __device__ __forceinline__ bool lm_tile_index(const double v, const double grid, const double half, int& out) {
    const double f = floor((v - half) / grid);
    if (!(f >= -2147483648.0 && f <= 2147483647.0)) return false;
    out = int(f);
    return true;
}

// ---- crop ----------------------------------------------------------------------------------------------------------------------------------
// counts[b] = points of tile b inside the box
__global__ void __launch_bounds__(kLmThreads) lm_crop_count_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                                  const unsigned n, const LmBox box, unsigned* __restrict__ counts) {
    __shared__ unsigned s_w[kLmWaves];
    const unsigned base = blockIdx.x * kLmTile + threadIdx.x;
    float px[kLmPerThread], py[kLmPerThread], pz[kLmPerThread];
#pragma unroll
    for (int k = 0; k < kLmPerThread; ++k) {  // all loads first
        const unsigned p = base + unsigned(k) * kLmThreads;
        const bool in = p < n;
        px[k] = in ? x[p] : 0.f; py[k] = in ? y[p] : 0.f; pz[k] = in ? z[p] : 0.f;
    }
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < kLmPerThread; ++k) {
        const unsigned p = base + unsigned(k) * kLmThreads;
        const bool keep = p < n && lm_in_box(box, px[k], py[k], pz[k]);
        c += unsigned(__popcll(__ballot(keep)));
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int q = 0; q < kLmWaves; ++q) t += s_w[q];
        counts[blockIdx.x] = t;
    }
}

// offs[b] = sum of counts[0, b), *total = the sum of all: ONE workgroup, every thread a contiguous run of the counts
__global__ void __launch_bounds__(kLmScanThreads) lm_scan_counts_kernel(const unsigned* __restrict__ counts, unsigned* __restrict__ offs, const unsigned nb,
                                                                       unsigned* __restrict__ total) {
    __shared__ unsigned wsum[kLmScanThreads / 64][1];
    const unsigned per = (nb + kLmScanThreads - 1) / kLmScanThreads;
    const unsigned b0 = min(nb, threadIdx.x * per), b1 = min(nb, b0 + per);
    unsigned v[1] = {0u}, tot[1];
    for (unsigned b = b0; b < b1; ++b) v[0] += counts[b];
    block_excl_scan<1>(v, tot, wsum);
    unsigned run = v[0];
    for (unsigned b = b0; b < b1; ++b) { offs[b] = run; run += counts[b]; }
    if (threadIdx.x == 0) *total = tot[0];
}

// the kept points of tile b to [offs[b], offs[b] + counts[b]) in cloud order.  Inside a tile the points run wave-row by wave-row: point
// base + k * kLmThreads + tid belongs to row (k, wave), so its place is the counts of the rows before it + the kept lanes below it.
__global__ void __launch_bounds__(kLmThreads) lm_crop_scatter_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                                    const float* __restrict__ in, const unsigned n, const LmBox box,
                                                                    const unsigned* __restrict__ offs, const unsigned total, float* __restrict__ ox,
                                                                    float* __restrict__ oy, float* __restrict__ oz, float* __restrict__ oi) {
    __shared__ unsigned s_row[kLmPerThread * kLmWaves];
    const unsigned base = blockIdx.x * kLmTile + threadIdx.x;
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float px[kLmPerThread], py[kLmPerThread], pz[kLmPerThread], pi[kLmPerThread];
#pragma unroll
    for (int k = 0; k < kLmPerThread; ++k) {
        const unsigned p = base + unsigned(k) * kLmThreads;
        const bool in_range = p < n;
        px[k] = in_range ? x[p] : 0.f; py[k] = in_range ? y[p] : 0.f; pz[k] = in_range ? z[p] : 0.f; pi[k] = in_range ? in[p] : 0.f;
    }
    bool keep[kLmPerThread];
    unsigned below[kLmPerThread];
#pragma unroll
    for (int k = 0; k < kLmPerThread; ++k) {
        const unsigned p = base + unsigned(k) * kLmThreads;
        keep[k] = p < n && lm_in_box(box, px[k], py[k], pz[k]);
        const unsigned long long m = __ballot(keep[k]);
        below[k] = unsigned(__popcll(m & ((1ull << lane) - 1ull)));
        if (lane == 0) s_row[k * kLmWaves + int(w)] = unsigned(__popcll(m));
    }
    __syncthreads();
    const unsigned block_off = offs[blockIdx.x];
    unsigned before = 0;
    int q = 0;
#pragma unroll
    for (int k = 0; k < kLmPerThread; ++k) {
        for (const int end = k * kLmWaves + int(w); q < end; ++q) before += s_row[q];
        const unsigned o = block_off + before + below[k];
        if (keep[k] && o < total) { ox[o] = px[k]; oy[o] = py[k]; oz[o] = pz[k]; oi[o] = pi[k]; }
    }
}

// ---- bounds ------------------------------------------------------------------------------------------------------------------------------------
// enc[0..2] = ~vg_ord(min), enc[3..5] = vg_ord(max) of x, y, z by atomicMax on words zeroed beforehand; NaN is ignored as by `v < mn` / `v > mx`
__global__ void __launch_bounds__(kLmThreads) lm_bounds_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                              const unsigned n, unsigned* __restrict__ enc) {
    __shared__ float s_red[kLmWaves][6];
    const float inf = __builtin_inff();
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    for (unsigned i = blockIdx.x * kLmThreads + threadIdx.x; i < n; i += gridDim.x * kLmThreads) {
        const float v[3] = {x[i], y[i], z[i]};
#pragma unroll
        for (int a = 0; a < 3; ++a) { if (v[a] < mn[a]) mn[a] = v[a]; if (v[a] > mx[a]) mx[a] = v[a]; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float a_mn = __shfl_xor(mn[a], o, 64), a_mx = __shfl_xor(mx[a], o, 64);
            if (a_mn < mn[a]) mn[a] = a_mn;
            if (a_mx > mx[a]) mx[a] = a_mx;
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_red[threadIdx.x >> 6][a] = mn[a]; s_red[threadIdx.x >> 6][3 + a] = mx[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = int(threadIdx.x);
        float v = s_red[0][a];
        for (int q = 1; q < kLmWaves; ++q) { const float t = s_red[q][a]; if (a < 3 ? t < v : t > v) v = t; }
        atomicMax(&enc[a], a < 3 ? ~vg_ord(v) : vg_ord(v));
    }
}

// ---- split -----------------------------------------------------------------------------------------------------------------------------------
// mm = {min gx, max gx, min gy, max gy} (initialised to INT_MAX / INT_MIN pairs), *bad = points whose index does not fit an int
__global__ void __launch_bounds__(kLmThreads) lm_tile_minmax_kernel(const float* __restrict__ x, const float* __restrict__ y, const unsigned n, const double grid,
                                                                   const double half, int* __restrict__ mm, unsigned* __restrict__ bad) {
    int lo[2] = {2147483647, 2147483647}, hi[2] = {-2147483647 - 1, -2147483647 - 1};
    unsigned nbad = 0;
    for (unsigned i = blockIdx.x * kLmThreads + threadIdx.x; i < n; i += gridDim.x * kLmThreads) {
        int gx, gy;
        if (!lm_tile_index(double(x[i]), grid, half, gx) || !lm_tile_index(double(y[i]), grid, half, gy)) { ++nbad; continue; }
        lo[0] = min(lo[0], gx); hi[0] = max(hi[0], gx);
        lo[1] = min(lo[1], gy); hi[1] = max(hi[1], gy);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 2; ++a) { lo[a] = min(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = max(hi[a], __shfl_xor(hi[a], o, 64)); }
        nbad += __shfl_xor(nbad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {  // (one wave's five atomics; at most kLmMaxBlocks * kLmWaves waves)
        atomicMin(&mm[0], lo[0]); atomicMax(&mm[1], hi[0]);
        atomicMin(&mm[2], lo[1]); atomicMax(&mm[3], hi[1]);
        if (nbad) atomicAdd(bad, nbad);
    }
}

// key = (gx - min gx) * span_y + (gy - min gy): ascending keys are LessGridIndex order; value = the point's index
__global__ void __launch_bounds__(kLmThreads) lm_tile_keys_kernel(const float* __restrict__ x, const float* __restrict__ y, const unsigned n, const double grid,
                                                                 const double half, const int min_gx, const int min_gy, const unsigned span_y,
                                                                 unsigned* __restrict__ keys, unsigned* __restrict__ vals) {
    const unsigned i = blockIdx.x * kLmThreads + threadIdx.x;
    if (i >= n) return;
    int gx = min_gx, gy = min_gy;
    (void)lm_tile_index(double(x[i]), grid, half, gx);
    (void)lm_tile_index(double(y[i]), grid, half, gy);
    keys[i] = unsigned(gx - min_gx) * span_y + unsigned(gy - min_gy);
    vals[i] = i;
}

// heads[*n_heads++] = {key, position} for the first position of every run of equal keys (any order: the host sorts by key)
__global__ void __launch_bounds__(kLmThreads) lm_tile_heads_kernel(const unsigned* __restrict__ keys, const unsigned n, uint2* __restrict__ heads,
                                                                  unsigned* __restrict__ n_heads, const unsigned cap) {
    const unsigned i = blockIdx.x * kLmThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned k = keys[i];
    if (i != 0 && keys[i - 1] == k) return;
    const unsigned slot = atomicAdd(n_heads, 1u);
    if (slot < cap) heads[slot] = make_uint2(k, i);
}

// out[j] = in[idx[j]] for the four planes (idx: a permutation of [0, n))
__global__ void __launch_bounds__(kLmThreads) lm_gather4_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                               const float* __restrict__ in, const unsigned* __restrict__ idx, const unsigned n,
                                                               float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz, float* __restrict__ oi) {
    const unsigned j = blockIdx.x * kLmThreads + threadIdx.x;
    if (j >= n) return;
    const unsigned i = idx[j];
    if (i >= n) return;
    ox[j] = x[i]; oy[j] = y[i]; oz[j] = z[i]; oi[j] = in[i];
}

// ---- stitch ----------------------------------------------------------------------------------------------------------------------------------
// one resident tile's (filtered) cloud and where its points go
struct LmSegment {
    const float *x, *y, *z, *in;
    unsigned start;  // exclusive prefix of the counts
    unsigned n;
};

// The output is cut into tiles of kLmTile points, one workgroup each; tile_first[b]: the segment that holds output point b * kLmTile.  A
// workgroup stages the segments its tile overlaps in LDS, window by window, and every lane finds its point's segment by a binary search.
__global__ void __launch_bounds__(kLmThreads) lm_stitch_kernel(const LmSegment* __restrict__ segs, const unsigned n_seg, const unsigned* __restrict__ tile_first,
                                                              const unsigned total, float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz,
                                                              float* __restrict__ oi) {
    __shared__ LmSegment s_seg[kLmWindow];
    __shared__ unsigned s_start[kLmWindow + 1];
    const unsigned tid = threadIdx.x;
    const unsigned tile_begin = blockIdx.x * kLmTile;
    const unsigned tile_end = total - tile_begin < kLmTile ? total : tile_begin + kLmTile;
    unsigned pos = tile_begin;
    for (unsigned base = tile_first[blockIdx.x]; pos < tile_end && base < n_seg;) {
        const unsigned w = n_seg - base < unsigned(kLmWindow) ? n_seg - base : unsigned(kLmWindow);
        __syncthreads();  // (the previous window's readers)
        if (tid < w) {
            s_seg[tid] = segs[base + tid];
            s_start[tid] = segs[base + tid].start;
        } else if (tid == w) {
            s_start[w] = base + w < n_seg ? segs[base + w].start : total;
        }
        __syncthreads();
        const unsigned lim = s_start[w] < tile_end ? s_start[w] : tile_end;  // this window's share of the tile: [pos, lim)
        for (unsigned p0 = pos + tid; p0 < lim; p0 += kLmTile) {
            float vx[kLmPerThread] = {}, vy[kLmPerThread] = {}, vz[kLmPerThread] = {}, vi[kLmPerThread] = {};
#pragma unroll
            for (int k = 0; k < kLmPerThread; ++k) {  // all loads first
                const unsigned p = p0 + unsigned(k) * kLmThreads;
                if (p >= lim) continue;
                unsigned lo = 0, hi = w;  // the last j in [0, w) with s_start[j] <= p: never an empty segment, since p < s_start[w]
                while (hi - lo > 1) {
                    const unsigned mid = (lo + hi) >> 1;
                    if (s_start[mid] <= p) lo = mid; else hi = mid;
                }
                const unsigned i = p - s_start[lo];
                if (i >= s_seg[lo].n) continue;
                vx[k] = s_seg[lo].x[i]; vy[k] = s_seg[lo].y[i]; vz[k] = s_seg[lo].z[i]; vi[k] = s_seg[lo].in[i];
            }
#pragma unroll
            for (int k = 0; k < kLmPerThread; ++k) {
                const unsigned p = p0 + unsigned(k) * kLmThreads;
                if (p >= lim) continue;
                ox[p] = vx[k]; oy[p] = vy[k]; oz[p] = vz[k]; oi[p] = vi[k];
            }
        }
        pos = lim;
        base += w;
    }
}

// the bounds launch with its six words: lo / hi of x | y | z (n > 0), one wait
struct DeviceBounds {
    DevBuf<unsigned> d_enc;
    PinnedBuf<unsigned> h_enc;
    void run(const float* x, const float* y, const float* z, const size_t n, hipStream_t s, float (&lo)[3], float (&hi)[3]) {
        d_enc.reserve(6);
        h_enc.reserve(6);
        FLS_HIP(hipMemsetAsync(d_enc.p, 0, 6 * sizeof(unsigned), s));
        const unsigned nb = unsigned(std::min<size_t>(kLmMaxBlocks, (n + kLmThreads - 1) / kLmThreads));
        hipLaunchKernelGGL(lm_bounds_kernel, dim3(nb), dim3(kLmThreads), 0, s, x, y, z, unsigned(n), d_enc.p);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpyAsync(h_enc.p, d_enc.p, 6 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        FLS_HIP(hipStreamSynchronize(s));
        for (int a = 0; a < 3; ++a) { lo[a] = vg_unord(~h_enc.p[a]); hi[a] = vg_unord(h_enc.p[3 + a]); }
    }
};

}  // namespace fls
