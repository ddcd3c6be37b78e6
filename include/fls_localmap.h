/* ============================================================================
 * fls_localmap.h -- C ABI of the device local-map source (same shared library as fls_reg.h and fls_keyframes.h; FLS_ABI_REVISION stays 9,
 * this header has a revision of its own): a localization run's global map and its tiles stay in the memory of an MI355X (gfx950), the
 * local map a reload needs is cut or stitched there, and it goes into a matcher without leaving the device.
 *
 *   Localization::Run, LoadGlobalMap + VoxelGridCloud(global, 0.3)   src/slam/localization.cpp:176-182   -> fls_localmap_set_global, once
 *   Localization::LoadLocalMap, crop-box branch                      src/slam/localization.cpp:366-409   -> fls_localmap_crop
 *   SplitMap::Split                                                  src/slam/split_map.cpp:22-55        -> fls_localmap_split
 *   LoadTileMap (tiles from files)                                   src/slam/localization.cpp:412-      -> fls_localmap_add_tile, once per tile
 *   Localization::LoadLocalMap, tile branch                          src/slam/localization.cpp:309-365   -> fls_localmap_load_tiles
 *   matcher_->AddCloudToLocalMap({*local_map})                       src/slam/localization.cpp:135, :222 -> fls_add_localmap_to_local_map
 *
 * Bit for bit:
 *   filter   fls_voxel_grid_cloud's contract (fls_reg.h): the device filter, and the exact host filter for whatever the device declines
 *   crop     the store keeps edge[6], empty after create, set_global and reset.  A call does the work when edge is empty, or force != 0, or
 *            some axis i in 0..2 fails fabs(t_i - edge[i]) > 50.0 && fabs(t_i - edge[i + 3]) > 50.0 (double; t = the pose's translation).
 *            Then edge = t -+ 100.0 in double, the box corners are those doubles cast to float, and a point is kept iff
 *            !(x < min.x || y < min.y || z < min.z || x > max.x || y > max.y || z > max.z) in float: a point on a face is kept.  The kept
 *            points keep the stored cloud's order and their intensities.  Otherwise *updated = 0 and nothing changes.
 *   split    per point gx = int(floor((double(x) - grid_size / 2) / grid_size)), gy likewise; tiles in (gx, gy) order (LessGridIndex), the
 *            points of a tile in the global cloud's order
 *   tiles    current tile c from the pose's x and y by the same formula; the 3 x 3 neighbours, x outer and y inner: one that exists as a
 *            tile and is not resident enters (its VoxelGridCloud(tile, leaf) computed, or taken from the cache); then a resident tile with
 *            dx * dx + dy * dy > 4 leaves (the reference's float norm() > 2).  When either happened -- or `leaf` differs from the one the
 *            local map was last stitched with -- the local map becomes the filtered forms of the resident tiles, concatenated in (gx, gy)
 *            order, and *updated = 1.  Every tile holds up to two filtered forms; a third replaces the older one.
 *   add      fls_add_localmap_to_local_map(m, h) equals fls_add_cloud_to_local_map(m, rows, n, NULL, 0, 4) on the rows
 *            fls_localmap_get_local returns: status, map, the following Match, fls_get_fitness_score.  LoamPointToPlaneIVOX and
 *            IncrementalNDT handles take the cloud device to device (their device builds read the store's planes; the iVox bounds come from
 *            a device reduction); where a build declines -- its own counters say why -- and for every other kind the local map is
 *            downloaded once and goes through the host entry point.
 *
 * A stated departure: a cloud stored with leaf == 0, and every tile, must hold finite coordinates only (FLS_ERR_RANGE otherwise).  The
 * pipeline's own map.pcd never holds another, and pcl::CropBox would keep such a point of a dense cloud.
 *
 * Plain C; no exception crosses the boundary; a handle is not thread-safe.  No CPU fallback for the store itself.  Every call returns with
 * the store's stream drained.  Arguments are validated before the device is looked at.  Statuses:
 *   FLS_ERR_INVALID  NULL handle or pointer; stride_floats < 3; a negative or non-finite leaf or grid_size; grid_size <= 0; a grid_size other
 *                    than the one in force (set by fls_localmap_split, or by the first fls_localmap_add_tile); an unknown tile; a cap too
 *                    small (*n_out / *n_tiles is still set); a non-finite pose translation; handles on different devices; more than
 *                    4,000,000,000 points; a split of more than 4,194,304 points (a larger map comes in tile by tile, fls_localmap_add_tile)
 *   FLS_ERR_STATE    no stored global cloud (crop, split); no tiles (load_tiles); an empty local map handed to a matcher
 *   FLS_ERR_RANGE    a non-finite coordinate (above); a tile index that does not fit int32; a split whose tile bounding box has more than
 *                    2^32 - 1 cells
 *   FLS_ERR_NOMEM    an allocation failed;  FLS_ERR_DEVICE  no gfx950 device, a HIP error
 * After any error the store is what it was before the call.
 * ==========================================================================*/
#ifndef FLS_LOCALMAP_H
#define FLS_LOCALMAP_H
#include "fls_reg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_LOCALMAP_REVISION 1

typedef struct fls_localmap* fls_localmap_handle;

int fls_localmap_revision(void);
fls_status fls_localmap_create(int device_id, fls_localmap_handle* out);
void fls_localmap_destroy(fls_localmap_handle h);

/* LoadGlobalMap + (leaf > 0 ? VoxelGridCloud(cloud, leaf) : cloud): replaces the stored global cloud; the edges, the tiles, the resident set
 * and the local map are cleared.  Rows of stride_floats floats: x y z [intensity] (3: intensity 0; 4..7: the fourth float; >= 8:
 * pcl::PointXYZI, the fifth).  n == 0 stores an empty cloud.  n_stored may be NULL. */
fls_status fls_localmap_set_global(fls_localmap_handle h, const float* pts, size_t n, int stride_floats, float leaf, size_t* n_stored);

/* LoadLocalMap, crop-box branch.  pose_colmajor: Mat4d::data().  *updated = 1: the local map is the new cut (*n_local points; an empty cut is
 * valid); 0: the hysteresis skipped the call, *n_local is the local map's size as it stays. */
fls_status fls_localmap_crop(fls_localmap_handle h, const double pose_colmajor[16], int force, int* updated, size_t* n_local);

/* SplitMap::Split of the stored global cloud: replaces all tiles, their caches and the resident set, and puts grid_size in force. */
fls_status fls_localmap_split(fls_localmap_handle h, double grid_size, size_t* n_tiles);

/* One tile from a file, uploaded once.  A tile that exists is replaced (its cached forms go, and it leaves the resident set). */
fls_status fls_localmap_add_tile(fls_localmap_handle h, double grid_size, int32_t gx, int32_t gy, const float* pts, size_t n, int stride_floats);

/* tile_map_indices.txt: (gx, gy) pairs and point counts in LessGridIndex order.  *n_tiles is set even when cap_tiles is too small. */
fls_status fls_localmap_tiles(fls_localmap_handle h, int32_t* gxgy, uint32_t* counts, size_t cap_tiles, size_t* n_tiles);

/* A tile's rows (x y z intensity): leaf == 0 as split / added, leaf > 0 VoxelGridCloud(tile, leaf), cached. */
fls_status fls_localmap_get_tile(fls_localmap_handle h, int32_t gx, int32_t gy, float leaf, float* out_xyzi, size_t cap_points, size_t* n_out);

/* LoadLocalMap, tile branch.  leaf == 0: the tiles as they are. */
fls_status fls_localmap_load_tiles(fls_localmap_handle h, const double pose_colmajor[16], float leaf, int* updated, size_t* n_local);

/* Forget the crop edges and the resident tile set (a new Localization, or `first || !has_init_`): the next crop or load_tiles does the work.
 * The stored clouds, the caches and the local map stay. */
fls_status fls_localmap_reset(fls_localmap_handle h);

/* The current local map as x y z intensity rows (UpdateLocalMapCloud). */
fls_status fls_localmap_get_local(fls_localmap_handle h, float* out_xyzi, size_t cap_points, size_t* n_out);

/* matcher_->AddCloudToLocalMap({*local_map}), device to device.  The matcher's stream waits for the store's work by an event; the call
 * returns with both streams drained. */
fls_status fls_add_localmap_to_local_map(fls_handle m, fls_localmap_handle h);

/* introspection: 0 stored global points, 1 tiles, 2 tile points, 3 crops run, 4 crops skipped by the hysteresis, 5 tile filters run, 6 tile
 * filter cache hits, 7 filters the device declined (the exact host filter ran), 8 stitches, 9 device-to-device hand-overs, 10 hand-overs that
 * went through the host entry point, 11 bytes resident, 12 device nanoseconds of the last crop or stitch (hipEvents; 0 before the first).
 * Other slots and a NULL handle: 0. */
size_t fls_localmap_stat(fls_localmap_handle h, int slot);

#ifdef __cplusplus
}
#endif
#endif
