// ingest_model.cpp -- test model of the driver-cloud front end (include/fls_ingest.h): a sequential restatement of
// PreProcessing::ConvertMessageToCloud and ComputePointOffsetTime (src/slam/preprocessing.cpp:262-552) over message bytes and a field
// descriptor, one point after the other, the way the reference walks its clouds.  Includes no product header.  Built by
// tests/ingest_util.py with g++ -O2 -ffp-contract=off for x86-64 and loaded with ctypes.
//
// yaw: the reference calls libm's atan2f, whose last bit no standard defines; the library defines yaw = (double)(float)A(y, x) with A an
// f64 atan2 of a fixed operation sequence.  im_atan2 restates A (argument reduction at 7/16, 11/16, 19/16, 39/16, odd polynomial of
// degree 23, hi/lo parts of the four reference angles).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

enum Sensor { VELODYNE = 0, OUSTER = 1, LIVOX_AVIA = 2, ROBOSENSE = 3, LEISHEN = 4, LIVOX_MID_360 = 5, NONE = 6 };

struct Row {  // PointXYZIRT, 32 bytes
    float x, y, z, pad0;
    float intensity;
    uint8_t ring, pad1[3];
    float time, pad2;
};
static_assert(sizeof(Row) == 32, "PointXYZIRT");

template <class T>
T rd(const uint8_t* p) {
    T v;
    std::memcpy(&v, p, sizeof(T));
    return v;
}

const double kAtanHi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
const double kAtanLo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
const double kAT[11] = {3.33333333333329318027e-01,  -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
                        9.09088713343650656196e-02,  -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
                        4.97687799461593236017e-02,  -3.65315727442169155270e-02, 1.62858201153657823623e-02};

double atan_nonneg(double x) {
    if (x >= std::ldexp(1.0, 66)) return kAtanHi[3] + kAtanLo[3];
    int id = -1;
    if (x < 0.4375) {
        if (x < std::ldexp(1.0, -29)) return x;
    } else if (x < 0.6875) {
        id = 0;
        x = (2.0 * x - 1.0) / (2.0 + x);
    } else if (x < 1.1875) {
        id = 1;
        x = (x - 1.0) / (x + 1.0);
    } else if (x < 2.4375) {
        id = 2;
        x = (x - 1.5) / (1.0 + 1.5 * x);
    } else {
        id = 3;
        x = -1.0 / x;
    }
    const double z = x * x, w = z * z;
    const double even = z * (kAT[0] + w * (kAT[2] + w * (kAT[4] + w * (kAT[6] + w * (kAT[8] + w * kAT[10])))));
    const double odd = w * (kAT[1] + w * (kAT[3] + w * (kAT[5] + w * (kAT[7] + w * kAT[9]))));
    if (id < 0) return x - x * (even + odd);
    return kAtanHi[id] - ((x * (even + odd) - kAtanLo[id]) - x);
}

double model_atan2(double y, double x) {
    const double pi = 3.1415926535897931160E+00, pi_lo = 1.2246467991473531772E-16;
    if (std::isnan(x) || std::isnan(y)) return x + y;
    const bool ny = std::signbit(y), nx = std::signbit(x);
    if (y == 0.0) return nx ? (ny ? -pi : pi) : y;
    if (x == 0.0) return ny ? -kAtanHi[3] : kAtanHi[3];
    const double z = (std::isinf(x) && std::isinf(y)) ? kAtanHi[1] : atan_nonneg(std::fabs(y) / std::fabs(x));
    if (!nx) return ny ? -z : z;
    return ny ? (z - pi_lo) - pi : pi - (z - pi_lo);
}

// include/common/math_function.h:159-186 with Type = float
float fast_atan2(float y, float x) {
    const float p1 = (float)0.9997878412794807, p3 = (float)-0.3258083974640975, p5 = (float)0.1555786518463281, p7 = (float)-0.04432655554792128;
    const float ax = std::fabs(x), ay = std::fabs(y), eps = 1.1920928955078125e-07f;
    float a;
    if (ax >= ay) {
        const float c = ay / (ax + eps), c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        const float c = ax / (ay + eps), c2 = c * c;
        a = (float)1.57079632679489661923 - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = (float)3.14159265358979323846 - a;
    if (y < 0) a = (float)(2 * 3.14159265358979323846) - a;
    if (a > (float)3.14159265358979323846) a -= (float)(2 * 3.14159265358979323846);
    return a;
}

// static_cast<int>(float) as x86-64 executes it: out of range or NaN -> INT_MIN
int to_int(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : INT32_MIN; }

bool finite3(float x, float y, float z) { return std::isfinite(x) && std::isfinite(y) && std::isfinite(z); }

// ComputePointOffsetTime(cloud, 10.0); branch[i]: 0 skipped ring, 1 first of ring, 2 yaw <= first, 3 yaw > first; bit 2: period added
void offset_time(std::vector<Row>& c, int scan_num, uint8_t* branch) {
    const double rate = 10.0, omega = 2.0 * M_PI * rate;
    std::vector<bool> is_first(scan_num, true);
    std::vector<double> yaw_first(scan_num, 0.0);
    std::vector<float> time_last(scan_num, 0.0f);
    for (size_t i = 0; i < c.size(); ++i) {
        const int ring = c[i].ring;
        if (branch) branch[i] = 0;
        if (ring >= scan_num) continue;
        const double yaw = (double)(float)model_atan2((double)c[i].y, (double)c[i].x);
        if (is_first[ring]) {
            yaw_first[ring] = yaw;
            is_first[ring] = false;
            time_last[ring] = 0.0f;
            if (branch) branch[i] = 1;
            continue;
        }
        if (yaw <= yaw_first[ring]) {
            c[i].time = static_cast<float>((yaw_first[ring] - yaw) / omega);
            if (branch) branch[i] = 2;
        } else {
            c[i].time = static_cast<float>((yaw_first[ring] - yaw + 2.0 * M_PI) / omega);
            if (branch) branch[i] = 3;
        }
        if (c[i].time < time_last[ring]) {
            c[i].time += static_cast<float>(2.0 * M_PI / omega);
            if (branch) branch[i] |= 4;
        }
        time_last[ring] = c[i].time;
    }
}

}  // namespace

extern "C" {

double im_atan2(double y, double x) { return model_atan2(y, x); }
void im_atan2_many(const double* y, const double* x, size_t n, double* out) {
    for (size_t k = 0; k < n; ++k) out[k] = model_atan2(y[k], x[k]);
}
float im_fast_atan2(float y, float x) { return fast_atan2(y, x); }

// the period loop alone on given base times: first[i] != 0 marks the first point of its ring (keeps own[i]); rings >= scan_num skipped
void im_period_loop(const float* base, const uint8_t* ring, const uint8_t* first, size_t n, int scan_num, float* time) {
    std::vector<float> last(scan_num, 0.0f);
    const float P = static_cast<float>(2.0 * M_PI / (2.0 * M_PI * 10.0));
    for (size_t i = 0; i < n; ++i) {
        if (ring[i] >= scan_num) continue;
        if (first[i]) { last[ring[i]] = 0.0f; continue; }
        float t = base[i];
        if (t < last[ring[i]]) t += P;
        time[i] = t;
        last[ring[i]] = t;
    }
}

// off = {x, y, z, intensity, ring, time, tag, line}.  rows: 32 n bytes, index: n.  info = {converted, min, max, last, t0, time-less}.
// branch (may be NULL): per converted point, the branch of ComputePointOffsetTime (see offset_time).  Returns the converted count.
size_t im_convert(const uint8_t* msg, size_t n, int sensor, uint32_t step, int is_dense, const uint32_t* off, double scale, int scan_num,
                  float lower_angle, float v_res, uint64_t stamp, uint8_t* rows, int32_t* index, double* info, uint64_t* stamp_out, uint8_t* branch) {
    std::vector<Row> c;
    std::vector<int32_t> idx;
    // pcl::fromROSMsg + RemoveNaNFromPointCloud / the Livox filter / the None loop: the surviving message points, in order
    std::vector<size_t> keep;
    for (size_t k = 0; k < n; ++k) {
        const uint8_t* q = msg + k * step;
        const float x = rd<float>(q + off[0]), y = rd<float>(q + off[1]), z = rd<float>(q + off[2]);
        if (sensor == LIVOX_AVIA) {
            const uint8_t line = q[off[7]], tag = q[off[6]];
            if (line < 6 && ((tag & 0x30) == 0x10 || (tag & 0x30) == 0x00)) keep.push_back(k);
        } else if (sensor == NONE) {
            if (!finite3(x, y, z)) continue;
            const float xy = std::sqrt(x * x + y * y);
            const int row = to_int(std::round((fast_atan2(z, xy) + lower_angle) / v_res));
            if (row >= scan_num || row < 0) continue;
            keep.push_back(k);
        } else if (is_dense || finite3(x, y, z)) {
            keep.push_back(k);
        }
    }
    double t0 = 0.0;
    *stamp_out = stamp;
    if (!keep.empty() && (sensor == ROBOSENSE || sensor == LIVOX_MID_360)) t0 = rd<double>(msg + keep[0] * step + off[5]);
    if (!keep.empty() && sensor == ROBOSENSE) *stamp_out = static_cast<uint64_t>(t0 * 1.0e6);
    for (size_t k : keep) {
        const uint8_t* q = msg + k * step;
        Row r;
        std::memset(&r, 0, sizeof r);
        r.x = rd<float>(q + off[0]);
        r.y = rd<float>(q + off[1]);
        r.z = rd<float>(q + off[2]);
        r.intensity = rd<float>(q + off[3]);
        switch (sensor) {
            case VELODYNE:
                r.ring = static_cast<uint8_t>(rd<uint16_t>(q + off[4]));
                r.time = static_cast<float>(rd<float>(q + off[5]) * scale);
                break;
            case OUSTER:
                r.ring = rd<uint8_t>(q + off[4]);
                r.time = static_cast<float>(rd<uint32_t>(q + off[5]) * scale);
                break;
            case LEISHEN:
                r.ring = static_cast<uint8_t>(rd<uint16_t>(q + off[4]));
                r.time = static_cast<float>(rd<double>(q + off[5]) * scale);
                break;
            case ROBOSENSE:
                r.ring = static_cast<uint8_t>(rd<uint16_t>(q + off[4]));
                r.time = static_cast<float>((rd<double>(q + off[5]) - t0) * scale);
                break;
            case LIVOX_MID_360:
                r.time = static_cast<float>((rd<double>(q + off[5]) - t0) * scale);
                break;
            case LIVOX_AVIA:
                r.time = static_cast<float>(static_cast<double>(rd<uint32_t>(q + off[5])) * scale);
                break;
            default: {
                const float xy = std::sqrt(r.x * r.x + r.y * r.y);
                r.ring = static_cast<uint8_t>(to_int(std::round((fast_atan2(r.z, xy) + lower_angle) / v_res)));
                break;
            }
        }
        c.push_back(r);
        idx.push_back(static_cast<int32_t>(k));
    }
    bool timeless = false;
    if (branch) std::memset(branch, 0, c.size());
    if (!c.empty() && (sensor == VELODYNE || sensor == NONE) && c.back().time <= 0.0f) {
        timeless = true;
        offset_time(c, scan_num, branch);
    }
    info[0] = static_cast<double>(c.size());
    info[1] = info[2] = info[3] = 0.0;
    info[4] = t0;
    info[5] = timeless ? 1.0 : 0.0;
    if (!c.empty()) {  // GetLidarPointMinMaxOffsetTime
        float mn = c[0].time, mx = c[0].time;
        for (const Row& p : c) {
            if (p.time < mn) mn = p.time;
            if (p.time > mx) mx = p.time;
        }
        info[1] = mn;
        info[2] = mx;
        info[3] = c.back().time;
        std::memcpy(rows, c.data(), c.size() * sizeof(Row));
        std::memcpy(index, idx.data(), idx.size() * sizeof(int32_t));
    }
    return c.size();
}

}  // extern "C"
