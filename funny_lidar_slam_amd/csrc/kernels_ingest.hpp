// kernels_ingest.hpp -- a lidar driver's message into the unified PointXYZIRT cloud on the device (include/fls_ingest.h):
//   PreProcessing::ConvertMessageToCloud     src/slam/preprocessing.cpp:262-511   ingest_count / deskew_scan / ingest_write
//   PreProcessing::ComputePointOffsetTime    src/slam/preprocessing.cpp:513-552   ingest_ring_first / ingest_base / ingest_ring_scan
//   GetLidarPointMinMaxOffsetTime            src/slam/preprocessing.cpp:554-570   ingest_minmax / ingest_summary
// The converted cloud (32-byte rows, DeskewRawDev {32, 0, 16, 20, 1, 24}) is the `raw` of the kernels of kernels_deskew.hpp.
//
// Compaction: per-block counts, the one-block exclusive scan of kernels_deskew.hpp, order-preserving write by ballot prefix sums.
// No launch relies on the order in which workgroups are dispatched; the only atomics are atomicMin, whose result has no order.
//
// Message loads tolerate any alignment (the packed Livox row is 22 bytes): a field is read with one load where its address is
// aligned and byte by byte where it is not.
//
// yaw.  A(y, x) = ingest_atan2 below is this library's model of the atan2f ComputePointOffsetTime calls: an f64 atan2 written out as
// a fixed sequence of IEEE operations (argument reduction at 7/16, 11/16, 19/16, 39/16 and an odd degree-23 polynomial, the classic
// table-free libm construction), no ocml / libm call, correctly rounded divisions, no FMA contraction (-ffp-contract=off).  Its
// error is below 1e-12 rad; yaw = (double)(float)A(y, x).  tests/host/ingest_model.cpp restates it independently.
//
// ComputePointOffsetTime is sequential per ring: t' = (t < last) ? t + P : t; last = t'.  As a function of `last` that update is a
// step function (thr, lo, hi): last > thr ? hi : lo, with thr = lo = t and hi = t + P.  Step functions are closed under composition,
// g o f = (thr_f, g(lo_f), g(hi_f)), and composition is associative, so every ring is one scan in stream order (ingest_ring_scan).
#pragma once
#include "kernels_deskew.hpp"

namespace fls {

constexpr int kIngestThreads = 256;       // count / write / base / minmax kernels
constexpr int kIngestRingThreads = 1024;  // one workgroup per ring
constexpr int kIngestRingItems = 4;       // consecutive points per thread: a chunk is 4096 points
constexpr unsigned kIngestNone = 0xFFFFFFFFu;

enum { kSensorVelodyne = 0, kSensorOuster = 1, kSensorAvia = 2, kSensorRoboSense = 3, kSensorLeiShen = 4, kSensorMid360 = 5, kSensorNone = 6 };

struct IngestDev {
    unsigned n;  // message points
    int sensor, drop_nonfinite;
    unsigned step, off_x, off_y, off_z, off_i, off_ring, off_time, off_tag, off_line;
    int vsn;
    float lower_angle, v_res;
    double scale;
};

// the mailbox the host reads before it builds the IMU segment
struct IngestMail {
    unsigned n_conv, timeless, nonfinite, pad;
    float t_min, t_max, t_last, pad2;
    double t0;
};

static_assert(sizeof(IngestMail) == 40, "the summary the host reads back");

struct IngestMinMax { float mn, mx; unsigned imn, imx; };

// ---- A(y, x) ------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ double ingest_atan_pos(double x) {  // atan of x >= 0 (not NaN)
    const double hi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
    const double lo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
    int id;
    if (x >= 73786976294838206464.0) return hi[3] + lo[3];  // 2^66
    if (x < 0.4375) {
        if (x < 1.862645149230957e-09) return x;  // 2^-29
        id = -1;
    } else if (x < 1.1875) {
        if (x < 0.6875) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); }
        else { id = 1; x = (x - 1.0) / (x + 1.0); }
    } else if (x < 2.4375) { id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); }
    else { id = 3; x = -1.0 / x; }
    const double z = x * x, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                      w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                      w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (id < 0) return x - x * (s1 + s2);
    return hi[id] - ((x * (s1 + s2) - lo[id]) - x);
}

__host__ __device__ __forceinline__ double ingest_atan2(const double y, const double x) {
    const double pi = 3.1415926535897931160E+00, pi_lo = 1.2246467991473531772E-16, pi_2 = 1.5707963267948965580E+00;
    if (x != x || y != y) return x + y;
    const bool ny = __builtin_signbit(y), nx = __builtin_signbit(x);
    if (y == 0.0) return nx ? (ny ? -pi : pi) : y;
    if (x == 0.0) return ny ? -pi_2 : pi_2;
    const double ax = nx ? -x : x, ay = ny ? -y : y;
    double z;
    if (ax > 1.7976931348623157e308 && ay > 1.7976931348623157e308) z = 7.85398163397448278999e-01;  // both infinite
    else z = ingest_atan_pos(ay / ax);
    if (!nx) return ny ? -z : z;
    return ny ? (z - pi_lo) - pi : pi - (z - pi_lo);
}

__host__ __device__ __forceinline__ double ingest_yaw(const float y, const float x) { return (double)(float)ingest_atan2((double)y, (double)x); }

// ---- the per-ring update as a step function ------------------------------------------------------------------------------------
struct IngestStep { float thr, lo, hi; int id; };  // id != 0: the identity (no point of the ring)

__host__ __device__ __forceinline__ float ingest_step_apply(const IngestStep& f, const float v) { return f.id ? v : (v > f.thr ? f.hi : f.lo); }
__host__ __device__ __forceinline__ IngestStep ingest_step_identity() { return IngestStep{0.f, 0.f, 0.f, 1}; }
__host__ __device__ __forceinline__ IngestStep ingest_step_first() { return IngestStep{0.f, 0.f, 0.f, 0}; }  // is_first: time_last = 0
// t' = (t < last) ? t + P : t
__host__ __device__ __forceinline__ IngestStep ingest_step_point(const float t, const float P) { return IngestStep{t, t, t + P, 0}; }
// f first, then g
__host__ __device__ __forceinline__ IngestStep ingest_step_compose(const IngestStep& f, const IngestStep& g) {
    if (f.id) return g;
    if (g.id) return f;
    return IngestStep{f.thr, ingest_step_apply(g, f.lo), ingest_step_apply(g, f.hi), 0};
}
__host__ __device__ __forceinline__ float ingest_period() { return (float)(2.0 * 3.14159265358979323846 / (2.0 * 3.14159265358979323846 * 10.0)); }
// the time before the period test (:540-544)
__host__ __device__ __forceinline__ float ingest_base_time(const double yaw_first, const double yaw) {
    const double omega = 2.0 * 3.14159265358979323846 * 10.0;
    if (yaw <= yaw_first) return (float)((yaw_first - yaw) / omega);
    return (float)((yaw_first - yaw + 2.0 * 3.14159265358979323846) / omega);
}

// ---- loads of any alignment (little-endian) ------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ingest_ld16(const unsigned char* p) {
    if (((size_t)p & 1u) == 0) return *(const unsigned short*)p;
    return (unsigned)p[0] | ((unsigned)p[1] << 8);
}
__device__ __forceinline__ unsigned ingest_ld32(const unsigned char* p) {
    if (((size_t)p & 3u) == 0) return *(const unsigned*)p;
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}
__device__ __forceinline__ float ingest_ldf(const unsigned char* p) { return __uint_as_float(ingest_ld32(p)); }
__device__ __forceinline__ double ingest_ldd(const unsigned char* p) {
    const unsigned long long v = (unsigned long long)ingest_ld32(p) | ((unsigned long long)ingest_ld32(p + 4) << 32);
    return __longlong_as_double((long long)v);
}
__device__ __forceinline__ bool ingest_finite(const float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// LidarModel::RowIndex with FastAtan2 (:485-492): the row as a float (rounded), compared as the reference compares the int
__device__ __forceinline__ bool ingest_none_row(const IngestDev& D, const float x, const float y, const float z, int& row) {
    const float xy = sqrt_rn(x * x + y * y);
    const float r = roundf(div_rn(fast_atan2f_dev(z, xy) + D.lower_angle, D.v_res));
    if (!(r >= 0.f && r < (float)D.vsn)) return false;  // (an int conversion out of range is INT_MIN on x86-64: row < 0)
    row = (int)r;
    return true;
}

__device__ __forceinline__ bool ingest_keep(const IngestDev& D, const unsigned char* q) {
    if (D.sensor == kSensorAvia) {
        const unsigned line = q[D.off_line], tag = q[D.off_tag] & 0x30u;
        return line < 6u && (tag == 0x10u || tag == 0x00u);
    }
    const float x = ingest_ldf(q + D.off_x), y = ingest_ldf(q + D.off_y), z = ingest_ldf(q + D.off_z);
    const bool fin = ingest_finite(x) && ingest_finite(y) && ingest_finite(z);
    if (D.sensor == kSensorNone) {
        int row;
        return fin && ingest_none_row(D, x, y, z, row);
    }
    return fin || !D.drop_nonfinite;
}

// pass 1: the keep rule.  flag[k], blk_cnt[b] = (kept, 0), *first_kept = lowest kept message index
__global__ void __launch_bounds__(kIngestThreads)
ingest_count_kernel(const unsigned char* __restrict__ msg, const IngestDev D, unsigned char* __restrict__ flag, uint2* __restrict__ blk_cnt,
                    unsigned* __restrict__ first_kept) {
    __shared__ unsigned wsum[kIngestThreads / 64];
    __shared__ unsigned wfirst[kIngestThreads / 64];
    const unsigned k = blockIdx.x * kIngestThreads + threadIdx.x;
    bool keep = false;
    if (k < D.n) {
        keep = ingest_keep(D, msg + (size_t)k * D.step);
        flag[k] = keep ? 1 : 0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) {
        wsum[wave] = (unsigned)__popcll(m);
        wfirst[wave] = m ? blockIdx.x * kIngestThreads + wave * 64 + (unsigned)(__ffsll((long long)m) - 1) : kIngestNone;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned a = 0, f = kIngestNone;
        for (int w = 0; w < kIngestThreads / 64; ++w) { a += wsum[w]; f = min(f, wfirst[w]); }
        blk_cnt[blockIdx.x] = make_uint2(a, 0u);
        if (f != kIngestNone) atomicMin(first_kept, f);
    }
}

// pass 3 (pass 2 is deskew_scan_kernel): order-preserving write of the converted rows, their message index and the compact ring array
__global__ void __launch_bounds__(kIngestThreads)
ingest_write_kernel(const unsigned char* __restrict__ msg, const IngestDev D, const unsigned char* __restrict__ flag, const uint2* __restrict__ blk_off,
                    const unsigned* __restrict__ first_kept, uint4* __restrict__ rows, int* __restrict__ msg_index, unsigned char* __restrict__ ring8) {
    __shared__ unsigned wsum[kIngestThreads / 64];
    const unsigned k = blockIdx.x * kIngestThreads + threadIdx.x;
    const unsigned f = k < D.n ? flag[k] : 0u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    if (lane == 0) wsum[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (!f) return;
    unsigned i = blk_off[blockIdx.x].x + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) i += wsum[w];
    const unsigned char* q = msg + (size_t)k * D.step;
    const float x = ingest_ldf(q + D.off_x), y = ingest_ldf(q + D.off_y), z = ingest_ldf(q + D.off_z), it = ingest_ldf(q + D.off_i);
    unsigned ring = 0;
    float t = 0.f;
    switch (D.sensor) {
        case kSensorVelodyne: ring = ingest_ld16(q + D.off_ring); t = (float)((double)ingest_ldf(q + D.off_time) * D.scale); break;
        case kSensorOuster: ring = q[D.off_ring]; t = (float)((double)ingest_ld32(q + D.off_time) * D.scale); break;
        case kSensorAvia: t = (float)((double)ingest_ld32(q + D.off_time) * D.scale); break;
        case kSensorLeiShen: ring = ingest_ld16(q + D.off_ring); t = (float)(ingest_ldd(q + D.off_time) * D.scale); break;
        case kSensorRoboSense:
        case kSensorMid360: {
            const double t0 = ingest_ldd(msg + (size_t)(*first_kept) * D.step + D.off_time);
            if (D.sensor == kSensorRoboSense) ring = ingest_ld16(q + D.off_ring);
            t = (float)((ingest_ldd(q + D.off_time) - t0) * D.scale);
            break;
        }
        default: {  // None
            int row = 0;
            (void)ingest_none_row(D, x, y, z, row);
            ring = (unsigned)row;
            break;
        }
    }
    ring &= 0xFFu;  // static_cast<uint8_t>
    rows[2 * (size_t)i] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0u);
    rows[2 * (size_t)i + 1] = make_uint4(__float_as_uint(it), ring, __float_as_uint(t), 0u);
    msg_index[i] = (int)k;
    ring8[i] = (unsigned char)ring;
}

__device__ __forceinline__ float ingest_row_time(const uint4* __restrict__ rows, const unsigned i) { return __uint_as_float(rows[2 * (size_t)i + 1].z); }
// "Velodyne or None, and the last converted point's time <= 0.0f" (:295, :502): decided by ingest_ring_first_kernel, before any time
// is rewritten, and recorded in *timeless for the two kernels behind it
__device__ __forceinline__ bool ingest_timeless(const IngestDev& D, const unsigned* __restrict__ tot, const uint4* __restrict__ rows) {
    if (D.sensor != kSensorVelodyne && D.sensor != kSensorNone) return false;
    const unsigned n = tot[0];
    return n != 0u && ingest_row_time(rows, n - 1u) <= 0.0f;
}

// time-less 1: first[r] = index of the ring's first point in the converted cloud (kIngestNone: the ring does not occur)
__global__ void __launch_bounds__(kIngestRingThreads)
ingest_ring_first_kernel(const IngestDev D, const unsigned* __restrict__ tot, const uint4* __restrict__ rows, const unsigned char* __restrict__ ring8,
                         unsigned* __restrict__ first, unsigned* __restrict__ timeless) {
    const bool go = ingest_timeless(D, tot, rows);  // (nothing has rewritten a time yet)
    if (blockIdx.x == 0 && threadIdx.x == 0) *timeless = go ? 1u : 0u;
    if (!go) return;
    __shared__ unsigned found;
    const unsigned n = tot[0], r = blockIdx.x;
    if (threadIdx.x == 0) found = kIngestNone;
    __syncthreads();
    for (unsigned base = 0; base < n; base += kIngestRingThreads) {
        const unsigned i = base + threadIdx.x;
        if (i < n && ring8[i] == r) atomicMin(&found, i);  // (LDS; the minimum has no order)
        __syncthreads();
        if (found != kIngestNone) break;  // (uniform: read after the barrier, written only before it)
        __syncthreads();
    }
    if (threadIdx.x == 0) first[r] = found;
}

// time-less 2: the time of every point before the period test, tb[i] (:531-544); the first point of a ring keeps its own time
__global__ void __launch_bounds__(kIngestThreads)
ingest_base_kernel(const IngestDev D, const unsigned* __restrict__ tot, const uint4* __restrict__ rows, const unsigned* __restrict__ first,
                   const unsigned* __restrict__ timeless, float* __restrict__ tb) {
    if (!*timeless) return;
    const unsigned i = blockIdx.x * kIngestThreads + threadIdx.x;
    if (i >= tot[0]) return;
    const unsigned r = rows[2 * (size_t)i + 1].y;
    if (r >= (unsigned)D.vsn) return;
    const unsigned fi = first[r];
    if (fi == i) return;
    const uint4 a = rows[2 * (size_t)i], b = rows[2 * (size_t)fi];
    tb[i] = ingest_base_time(ingest_yaw(__uint_as_float(b.y), __uint_as_float(b.x)), ingest_yaw(__uint_as_float(a.y), __uint_as_float(a.x)));
}

__device__ __forceinline__ IngestStep ingest_step_shfl_up(const IngestStep& f, const int o) {
    return IngestStep{__shfl_up(f.thr, o), __shfl_up(f.lo, o), __shfl_up(f.hi, o), __shfl_up(f.id, o)};
}

// time-less 3: one workgroup per ring walks the converted cloud in chunks of kIngestRingThreads * kIngestRingItems points in stream
// order; inside a chunk the ring's updates are composed per thread, scanned across the workgroup, and applied to the carried `last`
__global__ void __launch_bounds__(kIngestRingThreads)
ingest_ring_scan_kernel(const IngestDev D, const unsigned* __restrict__ tot, uint4* __restrict__ rows, const unsigned char* __restrict__ ring8,
                        const unsigned* __restrict__ first, const unsigned* __restrict__ timeless, const float* __restrict__ tb) {
    if (!*timeless) return;
    constexpr int W = kIngestRingThreads / 64;
    __shared__ IngestStep wtot[W];
    __shared__ float carry;
    const unsigned n = tot[0], r = blockIdx.x, fi = first[r];
    if (fi == kIngestNone) return;
    const float P = ingest_period();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0.f;
    __syncthreads();
    constexpr unsigned chunk = kIngestRingThreads * kIngestRingItems;
    for (unsigned base = (fi / chunk) * chunk; base < n; base += chunk) {
        const unsigned i0 = base + threadIdx.x * kIngestRingItems;
        float t[kIngestRingItems];
        unsigned mem = 0;
        IngestStep F = ingest_step_identity();
#pragma unroll
        for (int j = 0; j < kIngestRingItems; ++j) {
            const unsigned i = i0 + j;
            t[j] = 0.f;
            if (i < n && ring8[i] == r) {
                mem |= 1u << j;
                if (i == fi) F = ingest_step_compose(F, ingest_step_first());
                else { t[j] = tb[i]; F = ingest_step_compose(F, ingest_step_point(t[j], P)); }
            }
        }
        IngestStep S = F;  // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const IngestStep u = ingest_step_shfl_up(S, o);
            if (lane >= o) S = ingest_step_compose(u, S);
        }
        if (lane == 63) wtot[wave] = S;
        IngestStep E = ingest_step_shfl_up(S, 1);  // exclusive
        if (lane == 0) E = ingest_step_identity();
        __syncthreads();
        IngestStep B = ingest_step_identity();
        for (int w = 0; w < wave; ++w) B = ingest_step_compose(B, wtot[w]);
        float last = ingest_step_apply(ingest_step_compose(B, E), carry);
#pragma unroll
        for (int j = 0; j < kIngestRingItems; ++j) {
            if (!(mem & (1u << j))) continue;
            const unsigned i = i0 + j;
            if (i == fi) { last = 0.f; continue; }
            const float v = (t[j] < last) ? t[j] + P : t[j];  // :546-550
            rows[2 * (size_t)i + 1].z = __float_as_uint(v);
            last = v;
        }
        __syncthreads();  // every thread has read `carry` and wtot
        if (threadIdx.x == kIngestRingThreads - 1) carry = last;  // (the last thread's `last` is the chunk's composition applied to the carry)
        __syncthreads();
    }
}

// GetLidarPointMinMaxOffsetTime on the converted cloud: the first point holding the minimum / maximum wins, as in the reference's loop
__device__ __forceinline__ void ingest_mm_merge(IngestMinMax& a, const IngestMinMax& b) {
    if (b.imn != kIngestNone && (a.imn == kIngestNone || b.mn < a.mn || (b.mn == a.mn && b.imn < a.imn))) { a.mn = b.mn; a.imn = b.imn; }
    if (b.imx != kIngestNone && (a.imx == kIngestNone || b.mx > a.mx || (b.mx == a.mx && b.imx < a.imx))) { a.mx = b.mx; a.imx = b.imx; }
}
__device__ __forceinline__ IngestMinMax ingest_mm_block(IngestMinMax v, IngestMinMax* sh) {  // result valid in thread 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const IngestMinMax u{__shfl_down(v.mn, o), __shfl_down(v.mx, o), __shfl_down(v.imn, o), __shfl_down(v.imx, o)};
        ingest_mm_merge(v, u);
    }
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) ingest_mm_merge(v, sh[w]);
    return v;
}

__global__ void __launch_bounds__(kIngestThreads)
ingest_minmax_kernel(const unsigned* __restrict__ tot, const uint4* __restrict__ rows, IngestMinMax* __restrict__ part, unsigned* __restrict__ nonfinite) {
    __shared__ IngestMinMax sh[kIngestThreads / 64];
    const unsigned i = blockIdx.x * kIngestThreads + threadIdx.x;
    IngestMinMax v{0.f, 0.f, kIngestNone, kIngestNone};
    if (i < tot[0]) {
        const float t = ingest_row_time(rows, i);
        if (ingest_finite(t)) v = IngestMinMax{t, t, i, i};
        else *nonfinite = 1u;  // (every writer writes the same value)
    }
    v = ingest_mm_block(v, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ void __launch_bounds__(1024)
ingest_summary_kernel(const IngestDev D, const unsigned char* __restrict__ msg, const unsigned* __restrict__ tot, const uint4* __restrict__ rows,
                      const IngestMinMax* __restrict__ part, const unsigned nb, const unsigned* __restrict__ first_kept, const unsigned* __restrict__ nonfinite,
                      const unsigned* __restrict__ timeless, IngestMail* __restrict__ mail) {
    __shared__ IngestMinMax sh[1024 / 64];
    IngestMinMax v{0.f, 0.f, kIngestNone, kIngestNone};
    for (unsigned b = threadIdx.x; b < nb; b += 1024) ingest_mm_merge(v, part[b]);  // (increasing b per thread; the merge is a total order)
    v = ingest_mm_block(v, sh);
    if (threadIdx.x != 0) return;
    const unsigned n = tot[0];
    IngestMail m{};
    m.n_conv = n;
    m.timeless = *timeless;
    m.nonfinite = *nonfinite;
    m.t_min = v.mn;
    m.t_max = v.mx;
    m.t_last = n ? ingest_row_time(rows, n - 1u) : 0.f;
    m.t0 = (n && (D.sensor == kSensorRoboSense || D.sensor == kSensorMid360)) ? ingest_ldd(msg + (size_t)(*first_kept) * D.step + D.off_time) : 0.0;
    *mail = m;
}

}  // namespace fls
