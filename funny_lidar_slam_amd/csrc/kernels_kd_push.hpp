// kernels_kd_push.hpp -- a keyframe of the kd-tree kinds pushed into the DeviceCloudRing (kd_map.hpp) without leaving the device:
// the cloud the Match just used lies on the device as x | y | z planes plus an intensity plane, the ring's four planes are its destination.
//   kd_push_kernel  source planes of one or two clouds -> transformed points at the tails of one or two rings, one launch
// The transform is spelled exactly as the host spells it (host_math.hpp), and the library is built with -ffp-contract=off, so the rows are
// bit for bit what the host push stores:
//   kKdPushXformF  xform_cloud_f (IcpOptimized, LoamPointToPlaneKdtree): R, t cast to float, (R0 x + (R3 y + R6 z)) + t0 in float
//   kKdPushXformD  xform_cloud_d (LoamFull): float(((T0 x + T4 y) + T8 z) + T12) in double
//   kKdPushCopy    the points as they are
// Intensity moves as a 32-bit word (NaN payloads survive).  A lane serves one point: four 4-byte loads and four 4-byte stores, consecutive
// lanes on consecutive words, so every access of a wave is one contiguous 256-byte piece.  The ring's tail is any point count and the source
// planes start at any float of their allocation: no access here is wider than the 4 bytes every float is aligned to.
#pragma once
#include <hip/hip_runtime.h>

namespace fls {

constexpr int kKdPushBlock = 256;
constexpr int kKdPushXformF = 0, kKdPushXformD = 1, kKdPushCopy = 2;

// one ring's share of a push launch: n points from the source planes to the ring planes at its tail
struct KdPushMap {
    const float *sx, *sy, *sz;
    const unsigned* si;
    float *dx, *dy, *dz;
    unsigned* di;
    unsigned n;
};
struct KdPushArgs {
    KdPushMap m[2];  // (m[1].n == 0: one ring)
    int mode;
    float R[9], t[3];  // kKdPushXformF: column-major rotation and translation, already cast
    double T[16];      // kKdPushXformD: the column-major pose
};

__global__ void __launch_bounds__(kKdPushBlock) kd_push_kernel(const KdPushArgs a) {
    unsigned g = blockIdx.x * unsigned(kKdPushBlock) + threadIdx.x;
    const bool second = g >= a.m[0].n;
    if (second) g -= a.m[0].n;
    const KdPushMap& m = second ? a.m[1] : a.m[0];
    if (g >= m.n) return;
    const float px = m.sx[g], py = m.sy[g], pz = m.sz[g];
    float ox = px, oy = py, oz = pz;
    if (a.mode == kKdPushXformF) {
        ox = (a.R[0] * px + (a.R[3] * py + a.R[6] * pz)) + a.t[0];
        oy = (a.R[1] * px + (a.R[4] * py + a.R[7] * pz)) + a.t[1];
        oz = (a.R[2] * px + (a.R[5] * py + a.R[8] * pz)) + a.t[2];
    } else if (a.mode == kKdPushXformD) {
        const double x = px, y = py, z = pz;
        ox = float(((a.T[0] * x + a.T[4] * y) + a.T[8] * z) + a.T[12]);
        oy = float(((a.T[1] * x + a.T[5] * y) + a.T[9] * z) + a.T[13]);
        oz = float(((a.T[2] * x + a.T[6] * y) + a.T[10] * z) + a.T[14]);
    }
    m.dx[g] = ox;
    m.dy[g] = oy;
    m.dz[g] = oz;
    m.di[g] = m.si[g];
}

}  // namespace fls
