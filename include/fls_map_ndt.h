/* ============================================================================
 * fls_map_ndt.h -- the flat image of the voxel map of an FLS_INCREMENTAL_NDT handle: what fls_map_export / fls_map_import and
 * fls_map_image_export / fls_map_image_import (fls_reg.h) move for that kind, and what a replica set copies (same shared library;
 * FLS_ABI_REVISION stays 9, this header has a revision of its own, like the other additive headers).
 *
 * Layout: header | arrays.  Little-endian PODs, every array starts on a 16-byte boundary, every padding and unused byte is zero.  One
 * entry per alive voxel, in LRU order, OLDEST first (entry r is the r-th least recently touched voxel):
 *
 *      key         uint64[n]      packed voxel key (21 bits per axis, csrc/device_common.hpp::pack_key)
 *      num_points  int32[n]
 *      vid         int32[n]       voxel id (creation order: the correspondence id)
 *      estimated   uint8[n]       0 / 1
 *      pending     uint8[n]       points waiting for the next estimate (at most `carry`)
 *      points      double[n][8][3] the pending points in arrival order, zero beyond `pending`
 *      mu          double[n][3]
 *      sigma       double[n][9]   column-major
 *      info        double[n][9]   column-major
 *
 * A voxel beyond ndt_max_points_in_voxel (estimated, num_points > max) never reads its list again: it is written with pending = 0 and
 * zero points -- the normalisation fls_debug_ndt_voxels applies.  Not in the image: the hash table (rebuilt by the importer, whose slack
 * decides its size), LRU stamps (implied by the order), the state of the last Match, the fitness grid of a localization handle (rebuilt
 * by the importer's next fls_add_cloud_to_local_map; fls_get_fitness_score answers FLS_ERR_STATE until then).
 *
 * The image is a function of the map's logical state alone: a handle that keeps its map on the device and one that keeps it on the host
 * write the same bytes after the same calls.  A handle with ndt_min_points_in_voxel > 8 exports nothing (size 0 / FLS_ERR_STATE): its
 * voxels may hold more pending points than an entry carries.  A handle that never received a cloud exports the header alone.
 *
 * Import validates everything before the handle changes (a refused import leaves the handle as it was): FLS_ERR_INVALID for a wrong
 * magic, revision, size, count, parameter set (voxel size, min / max points, capacity must equal the importer's), a key that is reserved,
 * out of range or present twice, estimated not 0 / 1, pending > 8 or > 0 in a voxel beyond max, num_points < 0, vid outside
 * [0, next_vid), a non-finite mu / info of an estimated voxel.
 * ==========================================================================*/
#ifndef FLS_MAP_NDT_H
#define FLS_MAP_NDT_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_NDT_IMAGE_REVISION 1
#define FLS_NDT_IMAGE_MAGIC "FLSNDT01"
#define FLS_NDT_IMAGE_CARRY 8

typedef struct fls_ndt_image_header {
    char magic[8];             /* FLS_NDT_IMAGE_MAGIC, no terminator */
    uint32_t revision;         /* FLS_NDT_IMAGE_REVISION */
    uint32_t carry;            /* FLS_NDT_IMAGE_CARRY: pending points an entry carries */
    uint64_t total_bytes;      /* header + arrays + padding */
    uint64_t n_voxels;
    int32_t next_vid;          /* id the next created voxel gets */
    uint32_t flag_first_scan;  /* 0 / 1 (a localization handle keeps 1) */
    uint64_t ndt_voxel_size_bits; /* the bits of the double */
    int32_t ndt_min_points_in_voxel;
    int32_t ndt_max_points_in_voxel;
    int32_t ndt_capacity;
    uint32_t reserved;         /* zero */
} fls_ndt_image_header;        /* 64 bytes */

int fls_ndt_image_revision(void);

#ifdef __cplusplus
}
#endif
#endif
