// ivox_blob.hpp -- the host side of the FLSIVOX1 blob (include/fls_map_ivox.h) that needs no device: the header checks of an import and the
// sort key of the closed form of "a blob into an EMPTY map" (DESIGN.md 3).  IvoxMap (ivox_map.hpp) uses both; tests/host/ivox_blob_model_test.cpp
// holds them against HostIvox::assign_layout on the CPU.
#pragma once
#include "host_maps.hpp"
#include "../../include/fls_map_ivox.h"
#include <cmath>
#include <cstring>

namespace fls {

static_assert(sizeof(fls_ivox_blob_header) == 56 && sizeof(fls_ivox_blob_voxel) == 16 && sizeof(Pt4) == 16, "blob records");

// What an import checks before it reads a record.  The header is untrusted (it may come off a broadcast): both counts are bounded by the
// payload BEFORE multiplying (no u64 wrap), the resolution must be this map's.  `head`: at least sizeof(fls_ivox_blob_header) bytes when
// n_bytes says so; n_bytes: the whole blob.
inline fls_status ivox_blob_check_header(const void* head, const size_t n_bytes, const unsigned kind, const float resolution, fls_ivox_blob_header& hd) {
    if (!head || n_bytes < sizeof(fls_ivox_blob_header)) return FLS_ERR_INVALID;
    std::memcpy(&hd, head, sizeof(hd));
    if (std::memcmp(hd.magic, FLS_IVOX_BLOB_MAGIC, 8) != 0 || hd.version != FLS_IVOX_BLOB_VERSION || hd.kind != kind) return FLS_ERR_INVALID;
    const unsigned long long payload = (unsigned long long)(n_bytes - sizeof(fls_ivox_blob_header)) / 16ull;
    if ((n_bytes - sizeof(fls_ivox_blob_header)) % 16u != 0 || hd.n_voxels > payload || hd.n_points > payload || hd.n_voxels + hd.n_points != payload) return FLS_ERR_INVALID;
    if (!(hd.resolution > 0.f) || !std::isfinite(hd.resolution) || hd.resolution != resolution) return FLS_ERR_INVALID;
    if (hd.n_voxels > hd.n_points || hd.next_id < 0 || (unsigned long long)hd.next_id < hd.n_points) return FLS_ERR_INVALID;
    return FLS_OK;
}

// The brick extent of a voxel list and the bits each brick axis needs: the layout order (bz, by, bx, z, y, x) of HostIvox::assign_layout as ONE
// unsigned key, relative to the smallest brick so that the radix sort runs only the passes the extent has bits for (kernels_ivox_build.hpp's
// IvbExtent, computed from brick coordinates here instead of point coordinates).
struct IvoxBrickExtent {
    int bmin[3] = {0, 0, 0};
    int bits[3] = {0, 0, 0};
    int key_bits() const { return bits[0] + bits[1] + bits[2] + 3 * kBrickLog; }  // <= 3 * 18 + 9
};
inline IvoxBrickExtent ivox_brick_extent(const int (&bmin)[3], const int (&bmax)[3]) {
    IvoxBrickExtent e;
    for (int a = 0; a < 3; ++a) {
        e.bmin[a] = bmin[a];
        const unsigned span = unsigned(bmax[a] - bmin[a]);
        while ((1u << e.bits[a]) <= span) ++e.bits[a];
    }
    return e;
}
// a packed voxel key that pack_key wrote for coordinates inside the key range (what every key of a map is)
__host__ __device__ __forceinline__ bool ivox_key_canonical(const unsigned long long key, int& x, int& y, int& z) {
    unpack_key(key, x, y, z);
    const int ax = x < 0 ? -x : x, ay = y < 0 ? -y : y, az = z < 0 ? -z : z;
    return pack_key(x, y, z) == key && ax < kKeyLimit && ay < kKeyLimit && az < kKeyLimit;
}
__host__ __device__ __forceinline__ unsigned long long ivox_brick_major_key(const int x, const int y, const int z, const int bmin_x, const int bmin_y, const int bmin_z,
                                                                            const int bx_bits, const int by_bits) {
    const unsigned long long bx = (unsigned)((x >> kBrickLog) - bmin_x), by = (unsigned)((y >> kBrickLog) - bmin_y), bz = (unsigned)((z >> kBrickLog) - bmin_z);
    const unsigned local = (unsigned)(((z & (kBrickSide - 1)) << (2 * kBrickLog)) | ((y & (kBrickSide - 1)) << kBrickLog) | (x & (kBrickSide - 1)));
    return ((((bz << by_bits) | by) << bx_bits | bx) << (3 * kBrickLog)) | local;
}

}  // namespace fls
