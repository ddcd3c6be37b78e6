/* ============================================================================
 * fls_map_kd.h -- the flat image of the local map of the three kd-tree kinds (FLS_ICP_OPTIMIZED, FLS_LOAM_FULL, FLS_P2PLANE_KDTREE): what
 * fls_map_export / fls_map_import and fls_map_image_export / fls_map_image_import (fls_reg.h) move for those kinds, what a replica set
 * copies, and the fused batch over a replica set (same shared library; FLS_ABI_REVISION stays 9, this header has a revision of its own,
 * like the other additive headers).
 *
 * The local map of these kinds is a pure function of the deque of keyframe clouds and the handle's parameters ([VoxelGrid of] the
 * concatenated deque, then the search grid), so the image carries the deque and the keyframe gate, and the importer rebuilds filter and
 * grid with the launches a keyframe update uses.
 *
 * Layout: header | map 0 | [map 1].  Little-endian PODs, every array starts on a 16-byte boundary, every padding and unused byte is zero.
 * One map for ICP and P2PlaneKd; two for LoamFull, planar first, then corner.  The header holds n_clouds and n_points of every map
 * (n_points == the sum of the map's sizes); per map:
 *
 *      sizes       uint32[n_clouds]   points per cloud, OLDEST cloud first; empty clouds are legal and are kept
 *      rows        float[n_points][4] x, y, z, intensity, copied as bits (NaN payloads survive), the clouds back to back in deque order
 *
 * Not in the image: the filtered map cloud and the search grid (rebuilt by the importer), the resident scan, the final pose of the last
 * Match (fls_get_fitness_score answers FLS_ERR_STATE until the importer's next Match, as after fls_scan_upload_raw), counters.
 *
 * The image is a function of the map's logical state alone: a handle that keeps its deque on the device and one that keeps it on the host
 * (FLS_DEVICE_VOXELGRID=0) write the same bytes after the same calls, and fls_map_export, fls_map_image_export to host memory and to
 * device memory write the same bytes.  A handle that never received a cloud exports the header alone (n_clouds 0).  A batch lane exports
 * nothing.
 *
 * Import validates everything before the handle changes (a refused import leaves the handle as it was): FLS_ERR_INVALID for a wrong
 * magic, revision, kind, map count or total_bytes, a size that is too small or overflows, sizes that do not sum to n_points, a parameter
 * or a localization mode that differs from the importer's, more clouds than the kind's deque may hold (1 for a localization handle of
 * ICP / P2PlaneKd), a gate with init not 0 / 1, a non-finite last_T while init is 1 or a non-zero one while it is 0, non-zero padding.
 * Point VALUES are not checked: whatever fls_add_cloud_to_local_map accepted, import accepts, so import(export(h)) never refuses.
 * The importer is an ordinary handle: it maps on bit for bit like the exporter.
 * ==========================================================================*/
#ifndef FLS_MAP_KD_H
#define FLS_MAP_KD_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_KD_IMAGE_REVISION 1
#define FLS_KD_IMAGE_MAGIC "FLSKDM01"

typedef struct fls_kd_image_header {
    char magic[8];                 /* FLS_KD_IMAGE_MAGIC, no terminator */
    uint32_t revision;             /* FLS_KD_IMAGE_REVISION */
    uint32_t kind;                 /* fls_kind of the exporter */
    uint64_t total_bytes;          /* header + maps + padding */
    uint32_t n_maps;               /* 1; 2 for FLS_LOAM_FULL */
    uint32_t is_localization_mode; /* 0 / 1 */
    uint32_t filter_size_bits[2];  /* the bits of the float: map_cloud_filter_size, 0 | planar_voxel_filter_size, corner_voxel_filter_size */
    uint32_t local_size[2];        /* local_map_size, 0 | local_planar_size, local_corner_size */
    uint64_t point_search_thres_bits; /* the bits of the double (ICP, LoamFull); 0 for P2PlaneKd, whose search has no gate */
    uint32_t gate_init;            /* keyframe gate: 0 / 1 */
    uint32_t reserved;             /* zero */
    double gate_last_T[16];        /* column-major, as bits; all zero while gate_init is 0 */
    uint64_t n_clouds[2];          /* per map; zero for a map the kind does not have */
    uint64_t n_points[2];
} fls_kd_image_header;             /* 224 bytes */

int fls_kd_image_revision(void);

/* fls_replicas_match_batch with fls_match_batch_fused per entry: the same block partition of the jobs over the set's entries, one host
 * thread per entry.  A kind without a fused form runs as fls_match_batch, exactly as fls_match_batch_fused does. */
fls_status fls_replicas_match_batch_fused(fls_replicas_handle r, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                          const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int slots);

#ifdef __cplusplus
}
#endif
#endif
