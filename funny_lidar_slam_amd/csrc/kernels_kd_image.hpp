// kernels_kd_image.hpp -- the rows of the flat image of the kd-tree kinds' local maps (include/fls_map_kd.h, kd_image.hpp) written from and
// read into the four SoA planes of a DeviceCloudRing (kd_map.hpp).
//   kd_image_pack_kernel    planes at head .. tail of one or two rings -> the float4 rows of one image, one launch
//   kd_image_unpack_kernel  the rows of one or two maps -> planes that start at float 0 of a ring of the importer's own
// Pure streaming, no arithmetic on the values (they move as 32-bit words: NaN payloads survive).  A lane serves four consecutive floats of
// every plane -- one 16-byte access per plane -- and the four rows they belong to, 16 bytes each.  The ring's head is any point count, so
// the pack kernel's quads are aligned to the PLANE, not to the head: quad g covers plane floats base + 4 g .. + 3 with base = head & ~3, its
// first and last quad may hold floats outside head .. tail, which are loaded (inside the plane: its capacity is a multiple of 4) and dropped.
#pragma once
#include <hip/hip_runtime.h>

namespace fls {

constexpr int kKdImageBlock = 256;

// one ring's share of a pack launch.  x / y / z / i: the planes at float `base` (16-byte aligned); the points are floats off .. off + n
struct KdPackMap {
    const unsigned *x, *y, *z, *i;
    uint4* rows;         // n rows of the image
    unsigned off, n;     // off = head - base < 4
    unsigned quads;      // (off + n + 3) / 4
};
struct KdPackArgs { KdPackMap m[2]; };  // (m[1].quads == 0: one ring)

__global__ void __launch_bounds__(kKdImageBlock) kd_image_pack_kernel(const KdPackArgs a) {
    unsigned g = blockIdx.x * unsigned(kKdImageBlock) + threadIdx.x;
    const bool second = g >= a.m[0].quads;
    if (second) g -= a.m[0].quads;
    const KdPackMap& m = second ? a.m[1] : a.m[0];
    if (g >= m.quads) return;
    const uint4 vx = reinterpret_cast<const uint4*>(m.x)[g], vy = reinterpret_cast<const uint4*>(m.y)[g], vz = reinterpret_cast<const uint4*>(m.z)[g],
                vi = reinterpret_cast<const uint4*>(m.i)[g];
    const unsigned px[4] = {vx.x, vx.y, vx.z, vx.w}, py[4] = {vy.x, vy.y, vy.z, vy.w}, pz[4] = {vz.x, vz.y, vz.z, vz.w}, pi[4] = {vi.x, vi.y, vi.z, vi.w};
    const long long j0 = (long long)g * 4 - (long long)m.off;  // point of the quad's first float
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long j = j0 + k;
        if (j >= 0 && j < (long long)m.n) m.rows[j] = make_uint4(px[k], py[k], pz[k], pi[k]);
    }
}

// one map's share of an unpack launch.  The planes start at a 16-byte boundary and hold at least 4 * quads floats each
struct KdUnpackMap {
    const uint4* rows;
    unsigned *x, *y, *z, *i;
    unsigned n, quads;  // quads = (n + 3) / 4
};
struct KdUnpackArgs { KdUnpackMap m[2]; };

__global__ void __launch_bounds__(kKdImageBlock) kd_image_unpack_kernel(const KdUnpackArgs a) {
    unsigned g = blockIdx.x * unsigned(kKdImageBlock) + threadIdx.x;
    const bool second = g >= a.m[0].quads;
    if (second) g -= a.m[0].quads;
    const KdUnpackMap& m = second ? a.m[1] : a.m[0];
    if (g >= m.quads) return;
    const unsigned j0 = g * 4u;
    uint4 r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = j0 + k < m.n ? m.rows[j0 + k] : make_uint4(0u, 0u, 0u, 0u);  // (beyond the tail: zeros nobody reads)
    reinterpret_cast<uint4*>(m.x)[g] = make_uint4(r[0].x, r[1].x, r[2].x, r[3].x);
    reinterpret_cast<uint4*>(m.y)[g] = make_uint4(r[0].y, r[1].y, r[2].y, r[3].y);
    reinterpret_cast<uint4*>(m.z)[g] = make_uint4(r[0].z, r[1].z, r[2].z, r[3].z);
    reinterpret_cast<uint4*>(m.i)[g] = make_uint4(r[0].w, r[1].w, r[2].w, r[3].w);
}

}  // namespace fls
