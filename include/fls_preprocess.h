/* ============================================================================
 * fls_preprocess.h -- C ABI of the per-scan preprocessing that feeds Match (same shared library as fls_reg.h, revisions 8 and 9):
 * IMU de-skew of a raw driver cloud, the range gate, the point-jump subsample and the planar VoxelGrid, on MI355X (gfx950).
 *
 *   PreProcessing::Run() per-scan loop            src/slam/preprocessing.cpp:86-223
 *     time [min, max] of the points, the IMU segment (IMUDataSearcher::GetDataSegment, include/imu/imu_data_searcher.h:17-114,
 *     slerp on the host with the C library's acos / sin), SetRefTime(header stamp)                      -> host, once per scan
 *     range gate, LidarDistortionCorrector::ProcessPoint (src/lidar/lidar_distortion_corrector.cpp:19-63),
 *     ordered_cloud_ / planar_cloud_ (raw index % lidar_point_jump_span == 0)                           -> device, one lane per point
 *     planer_voxel_filter_ on planar_cloud_                                                              -> device VoxelGrid (host
 *                                                                                                           exact filter where it declines)
 *   LoamFull_KdTree: PointcloudProjector::Project with the corrector (src/loam/pointcloud_projector.cpp:58-112)
 *     -> fls_features_project_deskew (fls_features.h handle; then fls_features_extract as usual)
 *
 * The library reports what Run() would do with the scan (imu_status) and does not act on it: no queue, no thread.  The f64 order of
 * the rotation arithmetic is written down in funny_lidar_slam_amd/csrc/kernels_deskew.hpp.  Translation is not de-skewed (the
 * reference's TODO).  Plain C; no exception crosses the boundary; a handle is not thread-safe.  No CPU fallback.
 * ==========================================================================*/
#ifndef FLS_PREPROCESS_H
#define FLS_PREPROCESS_H
#include "fls_features.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct fls_preprocess* fls_preprocess_handle;

/* byte layout of one raw driver point with its time: PointXYZIRT (lidar_point_type.h:121-136, uint8 ring) = {32, 0, 16, 20, 1, 24};
 * VelodynePointXYZIRT (uint16 ring) = {32, 0, 16, 20, 2, 24}.  ring_bytes 0: no ring (fls_preprocess_scan only). */
typedef struct fls_raw_layout {
    uint32_t stride_bytes, xyz_offset /* 3 floats */, intensity_offset /* float */, ring_offset, ring_bytes /* 0, 1 or 2 */,
        time_offset /* float, seconds relative to the header stamp */;
} fls_raw_layout;

typedef struct fls_preprocess_params {
    uint32_t struct_size;             /* = sizeof(fls_preprocess_params) */
    int32_t lidar_point_jump_span;    /* >= 1                                                    */
    float min_distance, max_distance; /* lidar_use_min_dist_ / lidar_use_max_dist_               */
    float planar_voxel_filter_size;   /* 0 = no filtered cloud                                   */
    float reserved;
    double T_lidar_to_imu[16];        /* column-major, like every pose of this library           */
} fls_preprocess_params;

/* what PreProcessing::Run() does with the scan (preprocessing.cpp:115-146) */
enum {
    FLS_IMU_OK = 0,            /* segment built, clouds computed                                            */
    FLS_IMU_DROP = 1,          /* oldest IMU sample later than the cloud start: the reference drops the cloud */
    FLS_IMU_WAIT = 2,          /* newest IMU sample earlier than the cloud end: the reference waits for IMU   */
    FLS_IMU_EMPTY_SEGMENT = 3, /* start >= end: empty segment, every ProcessPoint fails, clouds empty         */
    FLS_IMU_EMPTY_CLOUD = 4    /* n == 0 (the reference does not accept an empty cloud here)                */
};

typedef struct fls_preprocess_result {
    uint32_t struct_size;      /* = sizeof(fls_preprocess_result), set by the caller */
    int32_t imu_status;        /* FLS_IMU_*                                          */
    uint64_t cloud_start_us, cloud_end_us; /* after widening to the header stamp     */
    uint64_t n_raw, n_ordered, n_planar, n_planar_filtered, n_segment;
    int32_t filter_on_device;  /* 1: the planar VoxelGrid ran on the device; 0: the host exact filter (or none) */
    int32_t reserved;
} fls_preprocess_result;

/* arrays fls_preprocess_get returns */
enum {
    FLS_PRE_ORDERED = 0,         /* xyzi (4 floats)   ordered_cloud_                                  */
    FLS_PRE_ORDERED_INDEX = 1,   /* int32             raw index of every ordered point                */
    FLS_PRE_PLANAR = 2,          /* xyzi              planar_cloud_ before the VoxelGrid              */
    FLS_PRE_PLANAR_FILTERED = 3, /* xyzi              VoxelGrid(planar_cloud_, planar_voxel_filter_size) */
    FLS_PRE_SEGMENT_T = 4,       /* uint64            IMU segment timestamps [us]                     */
    FLS_PRE_SEGMENT_Q = 5        /* 4 doubles, xyzw   IMU segment orientations                        */
};

/* Invalid parameters (span < 1, negative leaf, struct_size mismatch) -> FLS_ERR_INVALID */
fls_status fls_preprocess_create(const fls_preprocess_params* params, int device_id, fls_preprocess_handle* out);
void fls_preprocess_destroy(fls_preprocess_handle h);
/* One scan.  raw_points + layout: the driver cloud as received; stamp_us: its header stamp.  IMU: t_us[n_imu] strictly increasing,
 * q_xyzw[4 n_imu] = Quaterniond::coeffs() (used as given, not normalised); any superset of the samples covering the scan.
 * FLS_ERR_INVALID: bad layout, n_imu < 2, timestamps not strictly increasing, a non-finite point time, a segment of more than 1024
 * samples.  FLS_ERR_STATE with empty outputs: imu_status DROP or WAIT.  FLS_OK otherwise (EMPTY_SEGMENT / EMPTY_CLOUD: empty clouds). */
fls_status fls_preprocess_scan(fls_preprocess_handle h, const void* raw_points, size_t n, const fls_raw_layout* layout, uint64_t stamp_us,
                               const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, fls_preprocess_result* result);
/* copy a result array of the last scan into `out` (NULL: only the size); returns its element count */
size_t fls_preprocess_get(fls_preprocess_handle h, int what, void* out, size_t cap_elems);
/* Revision 9: fls_preprocess_scan with the clouds left in device memory.  Same arguments, validation, status codes, result struct and
 * bits in every cloud; the host learns the counts only.  fls_preprocess_get after such a scan downloads the requested array on its
 * first request (cached until the next scan) and returns what it returns after fls_preprocess_scan.  Where the device VoxelGrid
 * declines (filter_on_device = 0) the planar cloud is downloaded for the exact host filter, as in fls_preprocess_scan. */
fls_status fls_preprocess_scan_device(fls_preprocess_handle h, const void* raw_points, size_t n, const fls_raw_layout* layout, uint64_t stamp_us,
                                      const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, fls_preprocess_result* result);
/* Revision 9: make a cloud of `pre`'s last scan (what = FLS_PRE_ORDERED, FLS_PRE_PLANAR or FLS_PRE_PLANAR_FILTERED; after either scan
 * function) the resident scan of `m`, device to device.  Afterwards `m` is in the state fls_scan_upload_raw(m, rows, n, NULL, 0, 4) leaves
 * it in, rows = what fls_preprocess_get(pre, what, ...) returns: fls_match_resident runs the in-Match VoxelGrid of IcpOptimized /
 * IncrementalNDT on the attached cloud, and for either value of update_map the result, the map and every later call equal the host
 * path's.  The copy is queued on `m`'s stream behind the scan, and `pre`'s next scan is queued behind the copy (hipEvents; the host
 * does not wait): `pre` may scan again at once, before `m` has matched.  `m` fetches host copies of the scan only when a map update or
 * a declined device filter needs them; a Match with update_map == 0 downloads nothing of it.
 * Kinds: FLS_P2PLANE_IVOX, FLS_P2PLANE_KDTREE, FLS_ICP_OPTIMIZED, FLS_INCREMENTAL_NDT.  FLS_ERR_STATE: no completed scan on `pre`, its
 * last scan was DROP / WAIT (or invalid), or `m` is FLS_LOAM_FULL (its clouds come from fls_features_*).  FLS_ERR_INVALID: NULL handle,
 * unknown `what`, handles on different devices.  On an error `m` keeps its resident scan.  An EMPTY_SEGMENT / EMPTY_CLOUD scan
 * attaches an empty cloud.  A read-only replica accepts the call as it accepts fls_scan_upload. */
fls_status fls_scan_attach_preprocessed(fls_handle m, fls_preprocess_handle pre, int what);
/* introspection: bytes of result arrays and counts copied device -> host on behalf of the last scan so far (lazy downloads included) */
fls_status fls_preprocess_get_host_bytes(fls_preprocess_handle h, uint64_t* d2h_bytes);
/* device time of the last scan [ms] (hipEvents on the handle's stream): deskew_ms = the upload of the raw cloud + the de-skew and
 * compaction kernels, filter_ms = the planar VoxelGrid */
fls_status fls_preprocess_get_time(fls_preprocess_handle h, double* deskew_ms, double* filter_ms);

/* PointcloudProjector::Project with IMU de-skew: as fls_features_project, but a point claims its range-image cell only when its
 * ProcessPoint succeeds, and the ordered cloud stores the corrected xyz (depth, column and row from the raw xyz).  layout must have a
 * ring (ring_bytes 1 or 2).  *imu_status as above; DROP / WAIT -> FLS_ERR_STATE and no projection (fls_features_extract then fails). */
fls_status fls_features_project_deskew(fls_features_handle h, const void* raw_points, size_t n, const fls_raw_layout* layout, uint64_t stamp_us,
                                       const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, const double T_lidar_to_imu[16],
                                       size_t* n_ordered, int* imu_status);

#ifdef __cplusplus
}
#endif
#endif
