// kernels_keyframes.hpp -- the sub-map assembly of the keyframe store (fls_keyframes_merge): every selected keyframe's cloud
// transformed by its pose, the results back to back, in ONE launch whatever the number of keyframes (a dependent launch costs ~4.9 us,
// a GetSubMap sub-map has 41 segments).
//
// Pure streaming, no reuse: 16 bytes read and 16 written per point.  The output is cut into tiles of kKfTile points, one workgroup per
// tile -- NOT one workgroup per keyframe: the clouds differ in size.  A workgroup stages the segments its tile overlaps in LDS (pointers,
// the exclusive prefix of the counts, R and t cast to float) and every lane finds its point's segment by a binary search of that prefix.
// The first segment of a tile comes with the table (the host builds the table anyway); a tile that overlaps more than kKfWindow
// segments -- many tiny keyframes -- takes them window by window.  Every load and store of a wave is one contiguous run within a
// segment: one float per lane and plane (the planes start at arbitrary multiples of 4 bytes), one float4 per lane for row output.
//
// The arithmetic is xform_f / load_rt_float of kernels_knn.hpp (TransformPointCloud(.., Mat4d), pointcloud_utility.h:141-158).
#pragma once
#include "kernels_knn.hpp"

namespace fls {

constexpr int kKfThreads = 256;
constexpr int kKfPerThread = 4;
constexpr unsigned kKfTile = unsigned(kKfThreads) * kKfPerThread;  // output points per workgroup
constexpr int kKfWindow = 64;                                      // segments staged in LDS at a time

// one selected keyframe: its cloud (four planes on the device), where its points go, its pose as the caller gave it
struct KfSegment {
    const float *x, *y, *z, *in;
    double T[16];      // column-major
    unsigned start;    // exclusive prefix of the counts = index of its first output point
    unsigned n;
};

struct KfSegmentLds {
    const float *x, *y, *z, *in;
    RtFloat rt;
};

// ROWS: out = float4 rows (what the caller downloads); otherwise ox | oy | oz | oi planes (what DeviceVoxelGrid::run reads).
// tile_first[b]: the segment that holds output point b * kKfTile.  total = sum of the counts (> 0).
template <bool ROWS>
__global__ void __launch_bounds__(kKfThreads) kf_merge_kernel(const KfSegment* __restrict__ segs, const unsigned n_seg, const unsigned* __restrict__ tile_first,
                                                             const unsigned total, float4* __restrict__ rows, float* __restrict__ ox,
                                                             float* __restrict__ oy, float* __restrict__ oz, float* __restrict__ oi) {
    __shared__ KfSegmentLds s_seg[kKfWindow];
    __shared__ unsigned s_start[kKfWindow + 1];
    const unsigned tid = threadIdx.x;
    const unsigned tile_begin = blockIdx.x * kKfTile;
    const unsigned tile_end = total - tile_begin < kKfTile ? total : tile_begin + kKfTile;
    unsigned pos = tile_begin;
    for (unsigned base = tile_first[blockIdx.x]; pos < tile_end && base < n_seg;) {
        const unsigned w = n_seg - base < unsigned(kKfWindow) ? n_seg - base : unsigned(kKfWindow);
        __syncthreads();  // (the previous window's readers)
        if (tid < w) {
            const KfSegment& g = segs[base + tid];
            s_seg[tid].x = g.x; s_seg[tid].y = g.y; s_seg[tid].z = g.z; s_seg[tid].in = g.in;
            s_seg[tid].rt = load_rt_float(g.T);
            s_start[tid] = g.start;
        } else if (tid == w) {
            s_start[w] = base + w < n_seg ? segs[base + w].start : total;
        }
        __syncthreads();
        const unsigned lim = s_start[w] < tile_end ? s_start[w] : tile_end;  // this window's share of the tile: [pos, lim)
        for (unsigned p0 = pos + tid; p0 < lim; p0 += kKfTile) {
            float x[kKfPerThread], y[kKfPerThread], z[kKfPerThread], in[kKfPerThread];
            unsigned seg[kKfPerThread];
#pragma unroll
            for (int k = 0; k < kKfPerThread; ++k) {  // all loads first
                const unsigned p = p0 + unsigned(k) * kKfThreads;
                if (p >= lim) continue;
                unsigned lo = 0, hi = w;  // the last j in [0, w) with s_start[j] <= p: never an empty segment, since p < s_start[w]
                while (hi - lo > 1) {
                    const unsigned mid = (lo + hi) >> 1;
                    if (s_start[mid] <= p) lo = mid; else hi = mid;
                }
                seg[k] = lo;
                const unsigned i = p - s_start[lo];
                x[k] = s_seg[lo].x[i]; y[k] = s_seg[lo].y[i]; z[k] = s_seg[lo].z[i]; in[k] = s_seg[lo].in[i];
            }
#pragma unroll
            for (int k = 0; k < kKfPerThread; ++k) {
                const unsigned p = p0 + unsigned(k) * kKfThreads;
                if (p >= lim) continue;
                float tx, ty, tz;
                xform_f(s_seg[seg[k]].rt, x[k], y[k], z[k], tx, ty, tz);
                if (ROWS) {
                    rows[p] = make_float4(tx, ty, tz, in[k]);
                } else {
                    ox[p] = tx; oy[p] = ty; oz[p] = tz; oi[p] = in[k];
                }
            }
        }
        pos = lim;
        base += w;
    }
}

}  // namespace fls
