/* ============================================================================
 * fls_keyframes.h -- C ABI of the device keyframe store (same shared library as fls_reg.h, fls_preprocess.h and fls_ingest.h;
 * FLS_ABI_REVISION stays 9, this header has a revision of its own): the ordered clouds of the keyframes stay in the memory of an
 * MI355X (gfx950), their VoxelGrid-filtered forms are computed once per keyframe and leaf size, and a sub-map of any selection
 * of keyframes under any poses is ONE launch.
 *
 *   KeyFrame::LoadOrderedCloud                 the PCD load per keyframe and sub-map         -> fls_keyframes_add / _add_preprocessed, once
 *   LoopClosure::GetSubMap                     src/slam/loop_closure.cpp:179-231             -> fls_keyframes_merge(ids, poses, 0.2, 0)
 *   System::SaveMap, the global-map publisher  src/slam/system.cpp:310-316, :884-892         -> fls_keyframes_merge(ids, poses, 0.3, 0.3 | 0)
 *   GetSubMap x 2 + LoopClosure::Match         src/slam/loop_closure.cpp:233-267             -> fls_keyframes_loop_match
 *
 * A keyframe's cloud never changes after it is stored; only its pose does (pose-graph optimisation).  So the poses come in with every
 * call: the library stores none and composes none.  ref_pose.inverse() * pose (loop_closure.cpp:211-214) and the range clipping of
 * :194-200 are the caller's (include/fls_hip_keyframes.h has the real Eigen, funny_lidar_slam_amd/keyframes.py numpy); the library's
 * only arithmetic on a pose is the cast to float.
 *
 * Bit for bit:
 *   transform  TransformPointCloud(cloud, Mat4d) (include/common/pointcloud_utility.h:141-158): R and t cast to float, then
 *              (r0*x + (r1*y + r2*z)) + t per row in float without contraction; the intensity is copied
 *   filter     fls_voxel_grid_cloud's contract (fls_reg.h): the device filter, and the exact host filter for whatever the device declines
 *              (empty cloud, no finite point, a non-finite point, "leaf size too small", more than 4,194,304 points, the heap-sort case)
 *   order      keyframes in the order of `ids`, the points of a keyframe in cloud order, as operator+= leaves them
 *
 * Every keyframe holds up to four filtered forms (leaf sizes); a fifth replaces the oldest.
 *
 * Plain C; no exception crosses the boundary; a handle is not thread-safe.  No CPU fallback for the store itself.
 * Statuses: FLS_ERR_INVALID: NULL handle or pointer, stride_floats < 3, an id outside [0, count), a negative or non-finite leaf,
 * cap_points too small (*n_out is set), more than 4,000,000,000 merged points; FLS_ERR_NOMEM: an allocation failed, the store is
 * unchanged; FLS_ERR_DEVICE: no gfx950 device, a HIP error.  Arguments are validated before the device is looked at.
 * ==========================================================================*/
#ifndef FLS_KEYFRAMES_H
#define FLS_KEYFRAMES_H
#include "fls_preprocess.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_KEYFRAMES_REVISION 1

typedef struct fls_keyframes* fls_keyframes_handle;

int fls_keyframes_revision(void);
fls_status fls_keyframes_create(int device_id, fls_keyframes_handle* out);
void fls_keyframes_destroy(fls_keyframes_handle h);

/* LoadOrderedCloud's replacement: the keyframe's cloud goes to the device once.  Rows of stride_floats floats: x y z [intensity]
 * (3: intensity 0; 4..7: the fourth float; >= 8: pcl::PointXYZI, the fifth).  *id = 0, 1, 2, ... (KeyFrame::ID).  n == 0 is a valid,
 * empty keyframe. */
fls_status fls_keyframes_add(fls_keyframes_handle h, const float* pts, size_t n, int stride_floats, int32_t* id);

/* The same, device to device, from the last scan of `pre` (what = FLS_PRE_ORDERED / FLS_PRE_PLANAR / FLS_PRE_PLANAR_FILTERED): the
 * copy is queued behind the scan and `pre`'s next scan behind the copy (hipEvents, as in fls_scan_attach_preprocessed).
 * FLS_ERR_STATE: no completed scan on `pre`, or its last scan was DROP / WAIT; FLS_ERR_INVALID: NULL, unknown `what`, handles on
 * different devices.  On an error the store is unchanged. */
fls_status fls_keyframes_add_preprocessed(fls_keyframes_handle h, fls_preprocess_handle pre, int what, int32_t* id);

size_t fls_keyframes_count(fls_keyframes_handle h);

/* Rows (x y z intensity) of keyframe `id`: leaf == 0 the stored cloud, leaf > 0 VoxelGridCloud(cloud, leaf), computed and cached on
 * the first request.  *n_out is set even when out_xyzi is too small (-> FLS_ERR_INVALID); out_xyzi may be NULL when cap_points is 0. */
fls_status fls_keyframes_get(fls_keyframes_handle h, int32_t id, float leaf, float* out_xyzi, size_t cap_points, size_t* n_out);

/* for k in 0..n_ids: out += TransformPointCloud(leaf_each > 0 ? VoxelGridCloud(cloud[ids[k]], leaf_each) : cloud[ids[k]], poses[k]);
 * then, if leaf_final > 0: out = VoxelGridCloud(out, leaf_final).
 * poses: n_ids x 16 doubles, column-major (Mat4d::data()).  GetSubMap = (0.2, 0); SaveMap = (0.3, 0.3).  An id may repeat.
 * n_ids == 0: FLS_OK, *n_out = 0.  *n_out is set even when out_xyzi is too small (-> FLS_ERR_INVALID). */
fls_status fls_keyframes_merge(fls_keyframes_handle h, const int32_t* ids, const double* poses, size_t n_ids, float leaf_each, float leaf_final,
                               float* out_xyzi, size_t cap_points, size_t* n_out);

/* GetSubMap twice (leaf 0.2, no final filter) + LoopClosure::Match: the result equals fls_loop_match on the two clouds
 * fls_keyframes_merge returns.  T_colmajor is the initial guess on entry, as in fls_loop_match; stats may be NULL.
 * Both sub-maps are assembled on the device and downloaded once each; the matcher is fls_loop_match's own (one per device, calls on a
 * device serialised).  Here that matcher starts from host clouds: its first filters are the exact host ones.  The same Match started
 * from the device sub-maps, without the two downloads, is fls_keyframes_loop_match_device (include/fls_loop_device.h). */
fls_status fls_keyframes_loop_match(fls_keyframes_handle h, const int32_t* src_ids, const double* src_poses, size_t n_src, const int32_t* tgt_ids,
                                    const double* tgt_poses, size_t n_tgt, double T_colmajor[16], float* fitness, fls_loop_stats* stats);

/* introspection, like the slots of fls_map_size: 0 stored points, 1 cached filtered clouds, 2 filters run (cache misses), 3 cache hits,
 * 4 filters the device declined, per keyframe or on the merged cloud (the exact host filter ran), 5 merge launches, 6 bytes resident
 * (keyframes and cached clouds), 7 device time of the last merge launch in nanoseconds (hipEvents; 0 before the first).  Other slots and a NULL
 * handle: 0. */
size_t fls_keyframes_stat(fls_keyframes_handle h, int slot);

#ifdef __cplusplus
}
#endif
#endif
