/* ============================================================================
 * fls_ingest.h -- C ABI of the driver-cloud front end of the per-scan preprocessing (same shared library as fls_reg.h and
 * fls_preprocess.h; FLS_ABI_REVISION stays 9, this header has a revision of its own): the conversion of a lidar driver's message
 * into the unified PointXYZIRT cloud on MI355X (gfx950), followed by what fls_preprocess_scan / fls_preprocess_scan_device /
 * fls_features_project_deskew do with that cloud.
 *
 *   PreProcessing::ConvertMessageToCloud       src/slam/preprocessing.cpp:262-511   keep rule, order-preserving compaction, ring and
 *                                                                                  time per sensor, RoboSense header stamp
 *   PreProcessing::ComputePointOffsetTime      src/slam/preprocessing.cpp:513-552   clouds without point times (Velodyne / None whose
 *                                                                                  last converted point has time <= 0): a per-ring
 *                                                                                  scan in stream order
 *
 * The message bytes go to the device once; no loop over the points runs on the host.  The index every later step uses
 * (lidar_point_jump_span, FLS_PRE_ORDERED_INDEX, the range image's raw index) is the index in the CONVERTED cloud, as in the
 * reference.  Little-endian messages only.  Field types are fixed by the sensor (include/lidar/lidar_point_type.h; pcl::fromROSMsg
 * maps fields by name), the byte offsets are the caller's: offsets and point_step need not be aligned.
 *
 * yaw.  ComputePointOffsetTime takes std::atan2(float, float), libm's atan2f, which is not correctly rounded: its last bit is not
 * defined by any standard.  This library defines yaw = (double)(float)A(y, x), A an f64 atan2 written out as a fixed operation
 * sequence (funny_lidar_slam_amd/csrc/kernels_ingest.hpp) with an error below 1e-12 rad: A is this library's model of atan2f.
 *
 * Plain C; no exception crosses the boundary; a handle is not thread-safe.  No CPU fallback.
 * ==========================================================================*/
#ifndef FLS_INGEST_H
#define FLS_INGEST_H
#include "fls_preprocess.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_INGEST_REVISION 1

/* LidarModel::LidarSensorType (include/lidar/lidar_model.h:24-26), same order */
enum {
    FLS_SENSOR_VELODYNE = 0,      /* uint16 ring, float time                                                   */
    FLS_SENSOR_OUSTER = 1,        /* uint8 ring, uint32 time ("t")                                             */
    FLS_SENSOR_LIVOX_AVIA = 2,    /* uint32 time, uint8 line, uint8 tag; ring 0                                */
    FLS_SENSOR_ROBOSENSE = 3,     /* uint16 ring, double absolute time ("timestamp")                           */
    FLS_SENSOR_LEISHEN = 4,       /* uint16 ring, double time ("timestamp")                                    */
    FLS_SENSOR_LIVOX_MID_360 = 5, /* double absolute time ("timestamp"); ring 0                                */
    FLS_SENSOR_NONE = 6           /* x y z intensity only; ring from the elevation, time 0                     */
};

/* the message as it arrived: sensor_msgs::PointCloud2 point_step, is_dense and the byte offset of each field the sensor's branch
 * reads (x, y, z, intensity: float; the others as listed above; offsets of fields the branch does not read are ignored) */
typedef struct fls_driver_cloud {
    uint32_t struct_size; /* = sizeof(fls_driver_cloud) */
    int32_t sensor;       /* FLS_SENSOR_*               */
    uint32_t point_step;
    int32_t is_dense;     /* 0: the five ring sensors and Mid-360 drop points with a non-finite x, y or z */
    uint32_t x_offset, y_offset, z_offset, intensity_offset, ring_offset, time_offset, tag_offset, line_offset;
} fls_driver_cloud;

typedef struct fls_ingest_params {
    uint32_t struct_size;          /* = sizeof(fls_ingest_params)                                                   */
    int32_t vertical_scan_num;     /* LidarModel::vertical_scan_num_, 1..255 (Velodyne and None; ignored otherwise) */
    double lidar_point_time_scale; /* ConfigParameters::lidar_point_time_scale_                                     */
    float lower_angle, v_res;      /* LidarModel::lower_angle_ / v_res_ [rad] (None only)                           */
} fls_ingest_params;

/* what the conversion found (the summary the device sends back before the IMU segment is built) */
typedef struct fls_ingest_info {
    uint32_t struct_size;  /* = sizeof(fls_ingest_info), set by the caller                                        */
    int32_t timeless;      /* 1: ComputePointOffsetTime ran                                                        */
    uint64_t n_message;    /* points in the message                                                                */
    uint64_t n_converted;  /* points in the converted cloud (= fls_preprocess_result.n_raw)                        */
    float time_min, time_max, time_last; /* of the converted cloud, after ComputePointOffsetTime                  */
    int32_t reserved;
    double t0;             /* RoboSense / Mid-360: the absolute stamp of the first kept point; 0 otherwise         */
} fls_ingest_info;

/* two more `what` codes of fls_preprocess_get, valid after fls_preprocess_scan_driver */
enum {
    FLS_PRE_CONVERTED = 16,      /* 32-byte PointXYZIRT rows, fls_raw_layout {32, 0, 16, 20, 1, 24}; padding bytes are 0 */
    FLS_PRE_CONVERTED_INDEX = 17 /* int32: message index of every converted point                                        */
};

int fls_ingest_revision(void);
/* the reference's own PCL struct of the sensor (lidar_point_type.h; pcl::PointXYZI for None), is_dense = 1.  The packed Livox Avia
 * message of system.cpp:476-529 is {x 0, y 4, z 8, intensity 12, time 16, line 20, tag 21}, point_step 22: set it by hand.
 * FLS_ERR_INVALID: unknown sensor, NULL. */
fls_status fls_ingest_default_layout(int sensor, fls_driver_cloud* out);

/* ConvertMessageToCloud on the device, then exactly fls_preprocess_scan (keep_on_device = 0) or fls_preprocess_scan_device
 * (keep_on_device = 1) on the converted cloud with the header stamp the reference goes on with (*stamp_out_us: the input stamp, for
 * RoboSense uint64(t0 * 1e6)).  Afterwards fls_preprocess_get, fls_scan_attach_preprocessed, fls_preprocess_get_host_bytes and
 * fls_preprocess_get_time work as after those functions; result->n_raw is the converted count.  result, stamp_out_us and info may be
 * NULL.
 * FLS_ERR_INVALID: NULL handle / descriptor / parameters, a struct_size mismatch, unknown sensor, a field the branch reads running
 * past point_step, vertical_scan_num outside 1..255 (Velodyne, None), a non-finite lidar_point_time_scale, and everything
 * fls_preprocess_scan rejects (a non-finite converted time among them).  FLS_ERR_STATE: imu_status DROP or WAIT.
 * A cloud that is empty after the conversion gives FLS_OK with imu_status FLS_IMU_EMPTY_CLOUD and empty clouds (the reference
 * reads points.back() and [0] of the empty cloud there, which is undefined). */
fls_status fls_preprocess_scan_driver(fls_preprocess_handle h, const void* msg_points, size_t n, const fls_driver_cloud* cloud,
                                      const fls_ingest_params* ingest, uint64_t stamp_us, const uint64_t* imu_t_us, const double* imu_q_xyzw,
                                      size_t n_imu, int keep_on_device, fls_preprocess_result* result, uint64_t* stamp_out_us,
                                      fls_ingest_info* info);

/* The same front end for fls_features_project_deskew (LoamFull_KdTree): ring and corrected xyz come from the converted cloud, the raw
 * index of the range image is the index in the converted cloud.  Same errors; an empty converted cloud projects nothing. */
fls_status fls_features_project_driver(fls_features_handle h, const void* msg_points, size_t n, const fls_driver_cloud* cloud,
                                       const fls_ingest_params* ingest, uint64_t stamp_us, const uint64_t* imu_t_us, const double* imu_q_xyzw,
                                       size_t n_imu, const double T_lidar_to_imu[16], size_t* n_ordered, int* imu_status,
                                       uint64_t* stamp_out_us, fls_ingest_info* info);

#ifdef __cplusplus
}
#endif
#endif
