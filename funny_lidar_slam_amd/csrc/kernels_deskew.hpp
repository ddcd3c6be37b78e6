// kernels_deskew.hpp -- IMU de-skew of a raw scan on the device, the per-scan loop of PreProcessing::Run() that feeds Match:
//   LidarDistortionCorrector::SetRefTime / ProcessPoint   src/lidar/lidar_distortion_corrector.cpp:19-63   (q_ref_inv: host; points: deskew_point_kernel)
//   DataSearcher::SearchNearestTwoData                     include/common/data_searcher.h:100-134          deskew_bracket
//   the non-LOAM loop (range gate, de-skew, ordered / planar) src/slam/preprocessing.cpp:181-223            deskew_point / deskew_scan / deskew_write
//   PointcloudProjector::Project with a moving sensor       src/loam/pointcloud_projector.cpp:58-112        feat_project_deskew + deskew_apply_kernel
// The IMU segment (IMUDataSearcher::GetDataSegment, slerp with glibc acos / sin) is built on the host (preprocess_host.hpp).
//
// f64 operation order.  Eigen is not part of this build, so the order below is this library's model of Eigen 3.3.7 compiled for
// x86-64 (SSE2, -O3, no FMA); the device and the host evaluate exactly this sequence (-ffp-contract=off, Makefile), and the test model
// (tests/host/deskew_model.cpp) restates it independently:
//   nlerp(a, b, t)       c_k = a_k * (1 - t) + b_k * t                     per coefficient, (1 - t) rounded once
//   squaredNorm(q)       (x*x + z*z) + (y*y + w*w)                          (two-lane packet reduction; dot(a, b) likewise)
//   normalized(q)        q_k / sqrt(squaredNorm(q))   if squaredNorm > 0    (a division, not a multiply by the reciprocal)
//   inverse(q)           (-x, -y, -z, w)_k / squaredNorm(q)                 if squaredNorm > 0, else 0
//   a * b (quaternions)  x = (aw*bx + ay*bz) - (az*by - ax*bw)              (Geometry_SSE.h quat_product<double>: two packets)
//                        y = (aw*by + ay*bw) + (az*bx - ax*bz)
//                        z = (aw*bz - ay*bx) + (az*bw + ax*by)
//                        w = (aw*bw - ay*by) - (az*bz + ax*bx)
//   q * p (_transformVector)  uv = v x p;  uv = uv + uv;  r = (p + w * uv) + v x uv,   (a x b) = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx)
//   R * p + t (T.block<3,3>)  r_i = (R_i0*p0 + (R_i1*p1 + R_i2*p2)) + t_i   (coefficient-wise lazy product: unrolled halving sum)
//   point                      (float) ((q_ref_inv * q_curr) * (R * p + t))
// f64 division and sqrt are the correctly rounded sequences (v_div_scale / v_div_fmas / v_div_fixup; the ocml sqrt with its
// refinement), never a bare v_rcp_f64.
//
// Compaction: three launches (per-block counts, one-block exclusive scan, order-preserving write by ballot prefix sums).  No launch
// relies on the order in which workgroups are dispatched.
#pragma once
#include "kernels_features.hpp"

namespace fls {

constexpr int kDeskewThreads = 256;
constexpr int kDeskewMaxSeg = 1024;  // IMU samples in one segment (LDS: 40 B each); 5 s of a 200 Hz IMU

// raw point layout incl. the per-point time (float seconds) and the width of the ring field (1 or 2 bytes, 0 = none)
struct DeskewRawDev { unsigned stride, off_xyz, off_i, off_ring, ring_bytes, off_time; };

struct DeskewParamsDev {
    unsigned n;                 // raw points
    int n_seg;                  // samples in the IMU segment (>= 2)
    unsigned long long ref_us;  // SetRefTime(header stamp)
    double qri[4];              // q_ref_inv, xyzw
    double R[9], t[3];          // T_lidar_to_imu: R row-major, t
    float min_dist, max_dist;
    int gate;                   // 1: range gate first (non-LOAM kinds); 0: de-skew every point (LoamFull: the projector gates)
    unsigned jump_span;         // lidar_point_jump_span (>= 1)
};

// static_cast<int64_t>(double) as x86-64 executes it (cvttsd2si): out of range or NaN -> INT64_MIN
__host__ __device__ __forceinline__ long long deskew_trunc_i64(const double v) {
    return (v >= -9223372036854775808.0 && v < 9223372036854775808.0) ? (long long)v : (long long)(0x8000000000000000ull);
}
// ProcessPoint's t = uint64(int64(ref) + int64(relative_time * 1.0e6)) (two's complement wrap)
__host__ __device__ __forceinline__ unsigned long long deskew_point_time(const unsigned long long ref, const float rel) {
    return ref + (unsigned long long)deskew_trunc_i64((double)rel * 1.0e6);
}

__host__ __device__ __forceinline__ double deskew_sqnorm(const double* q) { return (q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]); }

// MotionInterpolator::InterpolateQuaternionLerp(a, b, ratio): nlerp, then .normalized()
__host__ __device__ __forceinline__ void deskew_nlerp(const double* a, const double* b, const double t, double* q) {
    const double s = 1.0 - t;
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = a[c] * s + b[c] * t;
    const double n2 = deskew_sqnorm(q);
    if (n2 > 0.0) {
        const double r = sqrt(n2);
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = q[c] / r;
    }
}

__host__ __device__ __forceinline__ void deskew_inverse(const double* q, double* o) {
    const double n2 = deskew_sqnorm(q);
    if (n2 > 0.0) { o[0] = -q[0] / n2; o[1] = -q[1] / n2; o[2] = -q[2] / n2; o[3] = q[3] / n2; }
    else { o[0] = o[1] = o[2] = o[3] = 0.0; }
}

__host__ __device__ __forceinline__ void deskew_qmul(const double* a, const double* b, double* o) {
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    o[0] = (aw * bx + ay * bz) - (az * by - ax * bw);
    o[1] = (aw * by + ay * bw) + (az * bx - ax * bz);
    o[2] = (aw * bz - ay * bx) + (az * bw + ax * by);
    o[3] = (aw * bw - ay * by) - (az * bz + ax * bx);
}

__host__ __device__ __forceinline__ void deskew_rotate(const double* q, const double* p, double* r) {
    const double vx = q[0], vy = q[1], vz = q[2], w = q[3];
    double ux = vy * p[2] - vz * p[1], uy = vz * p[0] - vx * p[2], uz = vx * p[1] - vy * p[0];
    ux = ux + ux; uy = uy + uy; uz = uz + uz;
    r[0] = (p[0] + w * ux) + (vy * uz - vz * uy);
    r[1] = (p[1] + w * uy) + (vz * ux - vx * uz);
    r[2] = (p[2] + w * uz) + (vx * uy - vy * ux);
}

// SearchNearestTwoData on a strictly increasing segment of m >= 2 samples: left index of the bracket, -1 outside.  The binary search
// returns what the reference's backward linear scan returns: the rightmost ts <= t, with the two end cases of the reference.
__host__ __device__ __forceinline__ int deskew_bracket(const unsigned long long* ts, const int m, const unsigned long long t) {
    if (t < ts[0] || t > ts[m - 1]) return -1;
    if (t == ts[0]) return 0;           // (front, front + 1)
    if (t == ts[m - 1]) return m - 2;   // (back - 1, back)
    int lo = 0, hi = m - 1;             // ts[lo] <= t < ts[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ts[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// ProcessPoint: false when t falls outside the segment
__host__ __device__ __forceinline__ bool deskew_process(const unsigned long long* ts, const double* qs, const int m, const DeskewParamsDev& P,
                                                        const float x, const float y, const float z, const float rel, float& xo, float& yo,
                                                        float& zo) {
    const unsigned long long t = deskew_point_time(P.ref_us, rel);
    const int l = deskew_bracket(ts, m, t);
    if (l < 0) return false;
    const double ratio = (double)(t - ts[l]) / (double)(ts[l + 1] - ts[l]);
    double qc[4], q[4];
    deskew_nlerp(qs + 4 * l, qs + 4 * (l + 1), ratio, qc);
    deskew_qmul(P.qri, qc, q);
    const double p[3] = {(double)x, (double)y, (double)z};
    double pi[3], r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pi[i] = (P.R[3 * i] * p[0] + (P.R[3 * i + 1] * p[1] + P.R[3 * i + 2] * p[2])) + P.t[i];
    deskew_rotate(q, pi, r);
    xo = (float)r[0]; yo = (float)r[1]; zo = (float)r[2];
    return true;
}

// the segment into LDS: ts[m] then q[4m] (dynamic shared memory, m * 40 bytes)
__device__ __forceinline__ void deskew_stage_segment(const unsigned long long* __restrict__ seg_t, const double* __restrict__ seg_q, const int m,
                                                     unsigned long long*& ts, double*& qs) {
    extern __shared__ double deskew_lds[];
    qs = deskew_lds;
    ts = (unsigned long long*)(deskew_lds + 4 * m);
    for (int k = threadIdx.x; k < m; k += blockDim.x) ts[k] = seg_t[k];
    for (int k = threadIdx.x; k < 4 * m; k += blockDim.x) qs[k] = seg_q[k];
    __syncthreads();
}

// pass 1: gate + de-skew of every raw point.  corr[k] = corrected xyz + intensity, flag[k] = bit 0 kept, bit 1 kept and k % span == 0;
// blk_cnt[b] = (kept, planar) of the block
__global__ void __launch_bounds__(kDeskewThreads)
deskew_point_kernel(const unsigned char* __restrict__ raw, const DeskewRawDev L, const DeskewParamsDev P, const unsigned long long* __restrict__ seg_t,
                    const double* __restrict__ seg_q, float4* __restrict__ corr, unsigned char* __restrict__ flag, uint2* __restrict__ blk_cnt) {
    unsigned long long* ts;
    double* qs;
    deskew_stage_segment(seg_t, seg_q, P.n_seg, ts, qs);
    __shared__ unsigned wsum[2][kDeskewThreads / 64];
    const unsigned k = blockIdx.x * kDeskewThreads + threadIdx.x;
    unsigned f = 0;
    if (k < P.n) {
        const unsigned char* q = raw + (size_t)k * L.stride;
        const float x = *(const float*)(q + L.off_xyz), y = *(const float*)(q + L.off_xyz + 4), z = *(const float*)(q + L.off_xyz + 8);
        const float it = *(const float*)(q + L.off_i), rel = *(const float*)(q + L.off_time);
        bool pass = true;
        if (P.gate) {
            const float d = depth_of(x, y, z);  // preprocessing.cpp:192-196
            pass = !(d < P.min_dist || d > P.max_dist);
        }
        float xo, yo, zo;
        if (pass && deskew_process(ts, qs, P.n_seg, P, x, y, z, rel, xo, yo, zo)) {
            corr[k] = make_float4(xo, yo, zo, it);
            f = 1u | ((k % P.jump_span) == 0u ? 2u : 0u);
        }
        flag[k] = (unsigned char)f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned c0 = (unsigned)__popcll(__ballot(f & 1u)), c1 = (unsigned)__popcll(__ballot(f & 2u));
    if (lane == 0) { wsum[0][wave] = c0; wsum[1][wave] = c1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned a = 0, b = 0;
        for (int w = 0; w < kDeskewThreads / 64; ++w) { a += wsum[0][w]; b += wsum[1][w]; }
        blk_cnt[blockIdx.x] = make_uint2(a, b);
    }
}

// pass 2: exclusive scan of the block counts (one workgroup, chunks of 1024 in order); tot = (kept, planar)
__global__ void __launch_bounds__(1024)
deskew_scan_kernel(const uint2* __restrict__ blk_cnt, const unsigned nb, uint2* __restrict__ blk_off, unsigned* __restrict__ tot) {
    __shared__ unsigned s0[1024], s1[1024];
    __shared__ unsigned carry0, carry1;
    if (threadIdx.x == 0) { carry0 = 0; carry1 = 0; }
    __syncthreads();
    for (unsigned base = 0; base < nb; base += 1024) {
        const unsigned b = base + threadIdx.x;
        const uint2 c = b < nb ? blk_cnt[b] : make_uint2(0u, 0u);
        s0[threadIdx.x] = c.x; s1[threadIdx.x] = c.y;
        __syncthreads();
        for (unsigned o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
            const unsigned a0 = threadIdx.x >= o ? s0[threadIdx.x - o] : 0u, a1 = threadIdx.x >= o ? s1[threadIdx.x - o] : 0u;
            __syncthreads();
            s0[threadIdx.x] += a0; s1[threadIdx.x] += a1;
            __syncthreads();
        }
        if (b < nb) blk_off[b] = make_uint2(carry0 + s0[threadIdx.x] - c.x, carry1 + s1[threadIdx.x] - c.y);
        __syncthreads();
        if (threadIdx.x == 1023) { carry0 += s0[1023]; carry1 += s1[1023]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { tot[0] = carry0; tot[1] = carry1; }
}

// pass 3: order-preserving write.  ordered = xyzi AoS + raw index; planar = SoA x | y | z | i with row stride `cap` (DeviceVoxelGrid's input)
__global__ void __launch_bounds__(kDeskewThreads)
deskew_write_kernel(const unsigned char* __restrict__ flag, const float4* __restrict__ corr, const unsigned n, const uint2* __restrict__ blk_off,
                    float4* __restrict__ ordered, int* __restrict__ ordered_idx, float* __restrict__ planar, const size_t cap) {
    __shared__ unsigned wsum[2][kDeskewThreads / 64];
    const unsigned k = blockIdx.x * kDeskewThreads + threadIdx.x;
    const unsigned f = k < n ? flag[k] : 0u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long m0 = __ballot(f & 1u), m1 = __ballot(f & 2u);
    if (lane == 0) { wsum[0][wave] = (unsigned)__popcll(m0); wsum[1][wave] = (unsigned)__popcll(m1); }
    __syncthreads();
    if (!f) return;
    const uint2 off = blk_off[blockIdx.x];
    unsigned b0 = off.x, b1 = off.y;
    for (int w = 0; w < wave; ++w) { b0 += wsum[0][w]; b1 += wsum[1][w]; }
    const float4 v = corr[k];
    const unsigned i = b0 + (unsigned)__popcll(m0 & below);
    ordered[i] = v;
    ordered_idx[i] = (int)k;
    if (f & 2u) {
        const size_t j = b1 + (unsigned)__popcll(m1 & below);
        planar[j] = v.x; planar[cap + j] = v.y; planar[2 * cap + j] = v.z; planar[3 * cap + j] = v.w;
    }
}

// LoamFull with de-skew, first half (pointcloud_projector.cpp:58-112): as feat_project_kernel, but a point whose ProcessPoint failed
// (flag bit 0 clear: pass 1 with gate = 0) never claims its cell, so the next return in stream order can
__global__ void __launch_bounds__(256)
feat_project_deskew_kernel(const unsigned char* __restrict__ raw, const unsigned n, const DeskewRawDev L, const FeatParamsDev p,
                           const unsigned char* __restrict__ flag, unsigned* __restrict__ owner) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n || !(flag[k] & 1u)) return;
    const unsigned char* q = raw + (size_t)k * L.stride;
    const float x = *(const float*)(q + L.off_xyz), y = *(const float*)(q + L.off_xyz + 4), z = *(const float*)(q + L.off_xyz + 8);
    const int row = L.ring_bytes == 1 ? (int)*(q + L.off_ring) : (int)*(const unsigned short*)(q + L.off_ring);
    const float d = depth_of(x, y, z);
    if (d < p.min_dist || d > p.max_dist) return;  // :66-68
    int col = (int)roundf(div_rn(fast_atan2f_dev(y, x), p.h_res)) + p.cols / 2;  // :69-70
    if (col >= p.cols) col -= p.cols;
    if (row >= p.rows || row < 0 || col < 0 || col >= p.cols) return;  // :87-88
    atomicMin(&owner[(size_t)row * p.cols + col], k);
}

// LoamFull with de-skew, after feat_compact_kernel: the stored xyz of every ordered point is its corrected xyz (:107-110); depth,
// column and intensity stay the raw point's
__global__ void __launch_bounds__(256)
deskew_apply_kernel(const int* __restrict__ n_ordered, const int* __restrict__ raw_index, const float4* __restrict__ corr, float4* __restrict__ ordered) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= *n_ordered) return;
    const float4 c = corr[raw_index[i]];
    float4 o = ordered[i];
    o.x = c.x; o.y = c.y; o.z = c.z;
    ordered[i] = o;
}

}  // namespace fls
