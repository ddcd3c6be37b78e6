/* ============================================================================
 * fls_map_ivox.h -- the FLSIVOX1 blob of the iVox map of an FLS_P2PLANE_IVOX handle, written and read at device speed (same shared
 * library; FLS_ABI_REVISION stays 9, this header has a revision of its own, like the other additive headers).
 *
 * The bytes are exactly what fls_map_export (fls_reg.h) writes for that kind; nothing about the format is new.  A blob from either export
 * call goes into either import call, and the importer is an ORDINARY handle: it matches, updates its map and exports like the exporter
 * (fls_map_image_import, by contrast, leaves a read-only replica).
 *
 * Layout: header | voxel records | points.  Little-endian PODs, no padding between the sections:
 *
 *      fls_ivox_blob_header   56 bytes
 *      fls_ivox_blob_voxel    [n_voxels]   one per alive voxel in LRU order, OLDEST first; count >= 1; pad = 0
 *      {float x, y, z; int32 id} [n_points] the points of the voxels in that order, inside a voxel in insertion (id) order
 *
 * The header is 56 bytes, so the two sections start 8 bytes off a 16-byte boundary of the blob (offsets 56 and 56 + 16 n_voxels): they are
 * 8-byte aligned, not 16.  The library packs and unpacks them in a staging buffer of its own that is shifted by 8 bytes, where every record
 * is 16-byte aligned, and moves the blob to or from caller memory with one copy; caller memory needs no alignment.
 *
 * Not in the blob: the slot layout of the device image (the importer lays the voxels out as a first build does: brick-major order, regions
 * of cap_for(count) slots back to back), LRU stamps (implied by the order: the k-th record gets stamp k + 1), the state of the last Match,
 * the fitness grid of a localization handle.
 *
 * `dst` / `src` is memory of the handle's device when the flag is non-zero, host memory otherwise (the convention of fls_map_image_*).
 *
 * fls_ivox_map_bytes   size of the blob now; 0 for a handle of another kind, a batch lane, a read-only replica.  Answered from counts the
 *                      host already holds: nothing is built or downloaded.
 * fls_ivox_map_export  FLS_ERR_STATE for a lane or a replica, FLS_ERR_RANGE when cap_bytes is too small.  A handle whose device image is
 *                      the map packs the blob on the device and stays in its state (no host mirror is built: fls_map_size slot 147 and
 *                      every other counter but 168 stay); a handle whose map is held by the host writes it as fls_map_export does.
 * fls_ivox_map_import  FLS_ERR_INVALID for a lane and for a blob that fails a check; a refused blob leaves the handle as it was.  Checked on
 *                      the host: magic, version, kind, sizes (bounded by the payload before multiplying), resolution equal to the
 *                      handle's, n_voxels <= n_points <= next_id.  Checked on the device before anything of the handle changes: every
 *                      count >= 1, the counts sum to n_points, no key twice.  The map is then built on the device from the voxels given.
 *                      The build declines to the host path (fls_map_import's: a device source is downloaded first), counted by reason.
 *
 * FLS_IVOX_DEVICE_IMAGE=0 (read when the handle is created) sends both calls through the host path.
 *
 * fls_map_size slots:  168  exports packed on the device          169  exports written by the host
 *                      170  imports built on the device           171  imports declined to the host path, of which
 *                      172  size: FLS_IVOX_DEVICE_IMAGE=0 is counted in 171 alone; here an empty blob, n_voxels >= the LRU capacity, or more
 *                           voxels or points than the device sort takes (4,194,304)
 *                      173  a key outside the key range or with reserved bits (an extent the sort key cannot hold)
 *                      174  a brick pool over its byte budget
 *                      175  the hash-table form (FLS_IVOX_DENSE=0, or the budget exceeded earlier)
 * ==========================================================================*/
#ifndef FLS_MAP_IVOX_H
#define FLS_MAP_IVOX_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_IVOX_BLOB_REVISION 1
#define FLS_IVOX_BLOB_MAGIC "FLSIVOX1"
#define FLS_IVOX_BLOB_VERSION 1

typedef struct fls_ivox_blob_header {
    char magic[8];       /* FLS_IVOX_BLOB_MAGIC, no terminator */
    uint32_t version;    /* FLS_IVOX_BLOB_VERSION */
    uint32_t kind;       /* FLS_P2PLANE_IVOX */
    float resolution;    /* voxel edge; must equal the importer's */
    uint32_t is_first;   /* 0 / 1: the map has not received its first cloud yet */
    uint64_t capacity;   /* the exporter's LRU capacity (informative: the importer keeps its own) */
    uint64_t n_voxels;
    uint64_t n_points;
    int64_t next_id;     /* id the next inserted point gets; >= n_points */
} fls_ivox_blob_header;  /* 56 bytes */

typedef struct fls_ivox_blob_voxel {
    uint64_t key;        /* packed voxel key (21 bits per axis, csrc/device_common.hpp::pack_key) */
    uint32_t count;      /* points of this voxel, >= 1 */
    uint32_t pad;        /* zero */
} fls_ivox_blob_voxel;   /* 16 bytes */

unsigned fls_ivox_blob_revision(void);
size_t fls_ivox_map_bytes(fls_handle h);
fls_status fls_ivox_map_export(fls_handle h, void* dst, size_t cap_bytes, int dst_on_device);
fls_status fls_ivox_map_import(fls_handle h, const void* src, size_t n_bytes, int src_on_device);

#ifdef __cplusplus
}
#endif
#endif
