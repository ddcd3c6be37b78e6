"""ctypes binding of libfls_reg.so (the product's C ABI, include/fls_reg.h).

No fallback of any kind: if the shared library is missing, or no gfx950 device
is usable, the calls fail loudly (RuntimeError / FlsError).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLS_REG_LIB") or os.path.join(_HERE, "libfls_reg.so")  # FLS_REG_LIB: diagnosis builds only (csrc/Makefile `timing`)
CSRC_DIR = os.path.join(_HERE, "csrc")

# every symbol include/fls_reg.h declares (tests check they are all exported)
EXPORTED_SYMBOLS = [
    "fls_create", "fls_destroy", "fls_add_cloud_to_local_map", "fls_match", "fls_get_fitness_score",
    "fls_scan_upload", "fls_scan_upload_raw", "fls_match_resident", "fls_match_batch", "fls_map_export", "fls_map_import", "fls_map_image_bytes", "fls_map_image_export", "fls_map_image_import", "fls_get_iteration_log", "fls_get_correspondences", "fls_map_size",
    "fls_set_profiling", "fls_get_kernel_time", "fls_get_traffic_counters", "fls_get_debug_stamps", "fls_debug_fullpiv_qr6", "fls_debug_ldlt6", "fls_debug_voxel_grid", "fls_debug_voxel_grid_timed", "fls_debug_exact_sort", "fls_debug_exact_sort_marks", "fls_voxel_grid_cloud", "fls_loop_match", "fls_status_string", "fls_abi_version", "fls_abi_revision",
    "fls_device_count",
    "fls_replicas_create", "fls_replicas_refresh", "fls_replicas_match_batch", "fls_replicas_import_ms", "fls_replicas_destroy",
    # include/fls_features.h
    "fls_features_create", "fls_features_destroy", "fls_features_project", "fls_features_extract", "fls_features_get", "fls_features_get_time",
]
# every symbol include/fls_preprocess.h declares (revision 8; revision 9 = HANDOFF_SYMBOLS)
HANDOFF_SYMBOLS = ["fls_preprocess_scan_device", "fls_scan_attach_preprocessed", "fls_preprocess_get_host_bytes"]
PREPROCESS_SYMBOLS = [
    "fls_preprocess_create", "fls_preprocess_destroy", "fls_preprocess_scan", "fls_preprocess_get", "fls_preprocess_get_time",
    "fls_features_project_deskew",
] + HANDOFF_SYMBOLS

# every symbol include/fls_features_device.h declares (FLS_FEATURES_DEVICE_REVISION 1): the feature clouds kept on the device, LoamFull attach
FEATURES_DEVICE_SYMBOLS = ["fls_features_device_revision", "fls_features_keep_on_device", "fls_features_get_host_bytes", "fls_features_stat",
                           "fls_scan_attach_features"]
FEAT_STAT_DEVICE_GATHERS, FEAT_STAT_DEVICE_FILTERS, FEAT_STAT_FILTER_DECLINES, FEAT_STAT_LAZY_DOWNLOADS = range(4)

# every symbol include/fls_ingest.h declares (FLS_INGEST_REVISION 1)
INGEST_SYMBOLS = ["fls_ingest_revision", "fls_ingest_default_layout", "fls_preprocess_scan_driver", "fls_features_project_driver"]

# every symbol include/fls_keyframes.h declares (FLS_KEYFRAMES_REVISION 1)
KEYFRAMES_SYMBOLS = ["fls_keyframes_revision", "fls_keyframes_create", "fls_keyframes_destroy", "fls_keyframes_add", "fls_keyframes_add_preprocessed",
                     "fls_keyframes_count", "fls_keyframes_get", "fls_keyframes_merge", "fls_keyframes_loop_match", "fls_keyframes_stat"]

# every symbol include/fls_localmap.h declares (FLS_LOCALMAP_REVISION 1)
LOCALMAP_SYMBOLS = ["fls_localmap_revision", "fls_localmap_create", "fls_localmap_destroy", "fls_localmap_set_global", "fls_localmap_crop",
                    "fls_localmap_split", "fls_localmap_add_tile", "fls_localmap_tiles", "fls_localmap_get_tile", "fls_localmap_load_tiles",
                    "fls_localmap_reset", "fls_localmap_get_local", "fls_add_localmap_to_local_map", "fls_localmap_stat"]

# every symbol include/fls_batch.h declares (FLS_BATCH_REVISION 1)
BATCH_SYMBOLS = ["fls_batch_revision", "fls_match_batch_fused", "fls_batch_stat"]

# every symbol include/fls_batch_ivox.h declares (FLS_BATCH_IVOX_REVISION 1)
BATCH_IVOX_SYMBOLS = ["fls_batch_ivox_revision", "fls_match_batch_shared_ivox", "fls_batch_ivox_stat"]

# every symbol include/fls_debug_linalg.h declares (FLS_DEBUG_LINALG_REVISION 1): test hooks of csrc/linalg_dev.hpp / wave_solve.hpp
DEBUG_LINALG_SYMBOLS = ["fls_debug_linalg_revision", "fls_debug_plane_fit_5x3", "fls_debug_svd3", "fls_debug_lu6", "fls_debug_so3", "fls_debug_wave_sum"]

# every symbol include/fls_debug_fit.h declares (FLS_DEBUG_FIT_REVISION 1): test hooks of the stages of the fit launch
DEBUG_FIT_SYMBOLS = ["fls_debug_fit_revision", "fls_debug_plane_residual", "fls_debug_line_residual", "fls_debug_icp_point_rows", "fls_debug_rank1_mfma",
                     "fls_debug_rank1_dpp", "fls_debug_rank1x3_mfma", "fls_debug_reduce_partials", "fls_debug_fanin", "fls_debug_last_system"]
DEBUG_TICKET_WORDS = 320  # FLS_DEBUG_TICKET_WORDS

# every symbol include/fls_debug_ndt.h declares (FLS_DEBUG_NDT_REVISION 1): test read-out of the NDT voxel map
DEBUG_NDT_SYMBOLS = ["fls_debug_ndt_revision", "fls_debug_ndt_voxels"]

# every symbol include/fls_debug_loop.h declares (FLS_DEBUG_LOOP_REVISION 1): test hooks of the stages of the loop-closure matcher
DEBUG_LOOP_SYMBOLS = ["fls_debug_loop_revision", "fls_debug_loop_ndt", "fls_debug_loop_gicp_cov", "fls_debug_loop_gicp_corr", "fls_debug_loop_gicp_fdf",
                      "fls_debug_loop_fitness"]

# every symbol include/fls_loop_device.h declares (FLS_LOOP_DEVICE_REVISION 1): the loop-closure Match from clouds on the device
LOOP_DEVICE_SYMBOLS = ["fls_loop_device_revision", "fls_loop_match_device", "fls_keyframes_loop_match_device", "fls_loop_device_stat"]
LOOP_DEVICE_STAT_SLOTS = ("matches", "filters_device", "filters_host", "leaves_device", "leaves_host", "input_bytes_downloaded",
                          "filtered_bytes_downloaded")

# every symbol include/fls_debug_loop_leaves.h declares (FLS_DEBUG_LOOP_LEAVES_REVISION 1): test hooks of the device leaf-Gaussian build
DEBUG_LOOP_LEAVES_SYMBOLS = ["fls_debug_loop_leaves_revision", "fls_debug_loop_leaves", "fls_debug_loop_ndt_device"]

# every symbol include/fls_debug_knn.h declares (FLS_DEBUG_KNN_REVISION 1): test hooks of the cooperative grid k-NN kernels of the kd-tree kinds
DEBUG_KNN_SYMBOLS = ["fls_debug_knn_revision", "fls_debug_grid_knn5", "fls_debug_grid_knn5_dual", "fls_debug_icp_knn1"]

# every symbol include/fls_debug_ivox_knn.h declares (FLS_DEBUG_IVOX_KNN_REVISION 1): the limits of the iVox kNN kernel's shared-run gate
DEBUG_IVOX_KNN_SYMBOLS = ["fls_debug_ivox_knn_revision", "fls_debug_ivox_knn_limits"]

# every symbol include/fls_debug_ivox_update.h declares (FLS_DEBUG_IVOX_UPDATE_REVISION 1): one decided batch through the iVox map update
DEBUG_IVOX_UPDATE_SYMBOLS = ["fls_debug_ivox_update_revision", "fls_debug_ivox_add_points"]

# every symbol include/fls_debug_ivox_decide.h declares (FLS_DEBUG_IVOX_DECIDE_REVISION 1): the iVox map-update decision launch, the list
# materialization and the host rule on caller-supplied arrays
DEBUG_IVOX_DECIDE_SYMBOLS = ["fls_debug_ivox_decide_revision", "fls_debug_ivox_decide", "fls_debug_ivox_nn_materialize", "fls_debug_ivox_decide_host"]
DEBUG_IVOX_DECIDE_FILL, DEBUG_IVOX_DECIDE_MAP_PAD = 0xA5, 64  # FLS_DEBUG_IVOX_DECIDE_FILL, FLS_DEBUG_IVOX_DECIDE_MAP_PAD

# every symbol include/fls_debug_tail.h declares (FLS_DEBUG_TAIL_REVISION 1): one launch of a Gauss-Newton tail on caller-supplied rows and state
DEBUG_TAIL_SYMBOLS = ["fls_debug_tail_revision", "fls_debug_loam_tail", "fls_debug_lu_tail"]
DEBUG_TAIL_MAX_ITER, DEBUG_TAIL_MAX_ROWS = 64, 2048  # FLS_DEBUG_TAIL_MAX_ITER, FLS_DEBUG_TAIL_MAX_ROWS


class DebugGnState(C.Structure):
    """fls_debug_gn_state (include/fls_debug_tail.h): GnState of csrc/device_common.hpp."""

    _fields_ = [("T", C.c_double * 16), ("last_rot", C.c_double), ("last_pos", C.c_double), ("sum_res", C.c_double), ("sum_res2", C.c_double),
                ("last_dx", C.c_double * 6), ("H", C.c_double * 36), ("g", C.c_double * 6), ("iter", C.c_int32), ("done", C.c_int32),
                ("converged", C.c_int32), ("n_valid", C.c_int32), ("n_valid2", C.c_int32), ("pad", C.c_int32), ("dbg", C.c_int64 * 16),
                ("log_T", C.c_double * (16 * DEBUG_TAIL_MAX_ITER)), ("log_res", C.c_double * DEBUG_TAIL_MAX_ITER), ("log_nv", C.c_int32 * DEBUG_TAIL_MAX_ITER)]


class DebugMailbox(C.Structure):
    """fls_debug_mailbox (include/fls_debug_tail.h): Mailbox of csrc/device_common.hpp."""

    _fields_ = [("T", C.c_double * 16), ("sum_res", C.c_double), ("sum_res2", C.c_double), ("last_dx", C.c_double * 6), ("iter", C.c_int32),
                ("done", C.c_int32), ("converged", C.c_int32), ("n_valid", C.c_int32), ("n_valid2", C.c_int32), ("seq", C.c_uint32)]


class DebugIvoxGate(C.Structure):
    """fls_debug_ivox_gate (include/fls_debug_ivox_decide.h)."""

    _fields_ = [("done", C.c_int32), ("iter", C.c_int32), ("n_valid", C.c_int32), ("max_iterations", C.c_int32), ("T", C.c_double * 16)]


# every symbol include/fls_map_ndt.h declares (FLS_NDT_IMAGE_REVISION 1): the flat image of the NDT voxel map, moved by fls_map_export / _import,
# fls_map_image_* and the replica sets of fls_reg.h
NDT_IMAGE_SYMBOLS = ["fls_ndt_image_revision"]
NDT_IMAGE_MAGIC, NDT_IMAGE_HEADER_BYTES, NDT_IMAGE_CARRY = b"FLSNDT01", 64, 8


class NdtImageHeader(C.Structure):
    """fls_ndt_image_header (include/fls_map_ndt.h)."""

    _fields_ = [("magic", C.c_char * 8), ("revision", C.c_uint32), ("carry", C.c_uint32), ("total_bytes", C.c_uint64), ("n_voxels", C.c_uint64),
                ("next_vid", C.c_int32), ("flag_first_scan", C.c_uint32), ("ndt_voxel_size_bits", C.c_uint64), ("ndt_min_points_in_voxel", C.c_int32),
                ("ndt_max_points_in_voxel", C.c_int32), ("ndt_capacity", C.c_int32), ("reserved", C.c_uint32)]


def ndt_image_layout(n: int) -> dict:
    """byte offsets of the arrays of an image of n voxels (csrc/ndt_image.hpp::ndt_image_layout): every array starts on a 16-byte boundary"""
    out, o = {}, NDT_IMAGE_HEADER_BYTES
    for name, width in (("key", 8), ("num_points", 4), ("vid", 4), ("estimated", 1), ("pending", 1), ("points", NDT_IMAGE_CARRY * 24), ("mu", 24),
                        ("sigma", 72), ("info", 72)):
        out[name] = o
        o = (o + n * width + 15) & ~15
    out["total"] = o
    return out

# every symbol include/fls_map_kd.h declares (FLS_KD_IMAGE_REVISION 1): the flat image of the kd-tree kinds' local maps (ICP, LoamFull, P2PlaneKd),
# moved by fls_map_export / _import, fls_map_image_* and the replica sets of fls_reg.h, and the fused batch over a replica set
KD_IMAGE_SYMBOLS = ["fls_kd_image_revision", "fls_replicas_match_batch_fused"]
KD_IMAGE_MAGIC, KD_IMAGE_HEADER_BYTES = b"FLSKDM01", 224


class KdImageHeader(C.Structure):
    """fls_kd_image_header (include/fls_map_kd.h)."""

    _fields_ = [("magic", C.c_char * 8), ("revision", C.c_uint32), ("kind", C.c_uint32), ("total_bytes", C.c_uint64), ("n_maps", C.c_uint32),
                ("is_localization_mode", C.c_uint32), ("filter_size_bits", C.c_uint32 * 2), ("local_size", C.c_uint32 * 2),
                ("point_search_thres_bits", C.c_uint64), ("gate_init", C.c_uint32), ("reserved", C.c_uint32), ("gate_last_T", C.c_double * 16),
                ("n_clouds", C.c_uint64 * 2), ("n_points", C.c_uint64 * 2)]


def kd_image_layout(n_clouds, n_points) -> dict:
    """byte offsets of the arrays of an image (csrc/kd_image.hpp::kd_image_layout): n_clouds / n_points per map (one entry, or two for LoamFull:
    planar, corner); every array starts on a 16-byte boundary.  Returns {"sizes": [...], "rows": [...], "total": n}."""
    out, o = {"sizes": [], "rows": []}, KD_IMAGE_HEADER_BYTES
    for nc, npts in zip(n_clouds, n_points):
        out["sizes"].append(o)
        o = (o + 4 * int(nc) + 15) & ~15
        out["rows"].append(o)
        o = (o + 16 * int(npts) + 15) & ~15
    out["total"] = o
    return out


# every symbol include/fls_map_ivox.h declares (FLS_IVOX_BLOB_REVISION 1): the FLSIVOX1 blob of fls_map_export / fls_map_import for the iVox kind,
# packed from and built into the device image without the host mirror
IVOX_BLOB_SYMBOLS = ["fls_ivox_blob_revision", "fls_ivox_map_bytes", "fls_ivox_map_export", "fls_ivox_map_import"]
IVOX_BLOB_MAGIC, IVOX_BLOB_VERSION, IVOX_BLOB_HEADER_BYTES, IVOX_BLOB_VOXEL_BYTES, IVOX_BLOB_POINT_BYTES = b"FLSIVOX1", 1, 56, 16, 16


class IvoxBlobHeader(C.Structure):
    """fls_ivox_blob_header (include/fls_map_ivox.h)."""

    _fields_ = [("magic", C.c_char * 8), ("version", C.c_uint32), ("kind", C.c_uint32), ("resolution", C.c_float), ("is_first", C.c_uint32),
                ("capacity", C.c_uint64), ("n_voxels", C.c_uint64), ("n_points", C.c_uint64), ("next_id", C.c_int64)]


class IvoxBlobVoxel(C.Structure):
    """fls_ivox_blob_voxel (include/fls_map_ivox.h)."""

    _fields_ = [("key", C.c_uint64), ("count", C.c_uint32), ("pad", C.c_uint32)]


# every symbol include/fls_knn_order.h declares (FLS_KNN_ORDER_REVISION 1): the neighbour order of the iVox point-to-plane kind
KNN_ORDER_SYMBOLS = ["fls_knn_order_revision", "fls_set_knn_order", "fls_get_knn_order", "fls_knn_order_limits"]
KNN_ORDER_DEFAULT, KNN_ORDER_REFERENCE = 0, 1

FLS_OK, FLS_NOT_CONVERGED, FLS_SKIPPED = 0, 1, 2
FLS_ERR_INVALID, FLS_ERR_DEVICE, FLS_ERR_RANGE, FLS_ERR_NOMEM, FLS_ERR_STATE = -1, -2, -3, -4, -5

ICP_OPTIMIZED, P2PLANE_IVOX, INCREMENTAL_NDT, LOAM_FULL, P2PLANE_KDTREE = range(5)


class FlsError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        super().__init__(f"{where}: {status_string(status)} ({status})")


class Params(C.Structure):
    """fls_params (include/fls_reg.h)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_iterations", C.c_uint32),
        ("is_localization_mode", C.c_int32),
        ("local_map_size", C.c_uint32),
        ("local_corner_size", C.c_uint32),
        ("local_planar_size", C.c_uint32),
        ("ndt_min_points_in_voxel", C.c_int32),
        ("ndt_max_points_in_voxel", C.c_int32),
        ("ndt_min_effective_pts", C.c_int32),
        ("ndt_capacity", C.c_int32),
        ("map_cloud_filter_size", C.c_float),
        ("source_cloud_filter_size", C.c_float),
        ("corner_voxel_filter_size", C.c_float),
        ("planar_voxel_filter_size", C.c_float),
        ("point_to_planar_thres", C.c_double),
        ("point_search_thres", C.c_double),
        ("line_ratio_thres", C.c_double),
        ("position_converge_thres", C.c_double),
        ("rotation_converge_thres", C.c_double),
        ("rot_thre_add_cloud", C.c_double),
        ("dist_thre_add_cloud", C.c_double),
        ("ndt_voxel_size", C.c_double),
        ("ndt_res_outlier_threshold", C.c_double),
    ]

    def __init__(self, **kw):
        super().__init__()
        self.struct_size = C.sizeof(Params)
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


class Stats(C.Structure):
    """fls_stats (include/fls_reg.h)."""

    _fields_ = [
        ("iterations", C.c_int32),
        ("converged", C.c_int32),
        ("n_valid", C.c_int32),
        ("n_valid_corner", C.c_int32),
        ("n_source", C.c_int32),
        ("n_source_corner", C.c_int32),
        ("map_updated", C.c_int32),
        ("reserved", C.c_int32),
        ("sum_res", C.c_double),
        ("sum_res_corner", C.c_double),
        ("last_dx", C.c_double * 6),
    ]


class FeatureParams(C.Structure):
    """fls_feature_params (include/fls_features.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("lidar_vertical_scan", C.c_int32), ("lidar_horizontal_scan", C.c_int32),
                ("lidar_horizontal_resolution", C.c_float), ("min_distance", C.c_float), ("max_distance", C.c_float),
                ("corner_thres", C.c_float), ("planar_thres", C.c_float), ("corner_voxel_filter_size", C.c_float),
                ("planar_voxel_filter_size", C.c_float)]


class PointLayout(C.Structure):
    """fls_point_layout (include/fls_features.h)."""

    _fields_ = [("stride_bytes", C.c_uint32), ("xyz_offset", C.c_uint32), ("intensity_offset", C.c_uint32), ("ring_offset", C.c_uint32)]


class RawLayout(C.Structure):
    """fls_raw_layout (include/fls_preprocess.h)."""

    _fields_ = [("stride_bytes", C.c_uint32), ("xyz_offset", C.c_uint32), ("intensity_offset", C.c_uint32), ("ring_offset", C.c_uint32),
                ("ring_bytes", C.c_uint32), ("time_offset", C.c_uint32)]


class PreprocessParams(C.Structure):
    """fls_preprocess_params (include/fls_preprocess.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("lidar_point_jump_span", C.c_int32), ("min_distance", C.c_float), ("max_distance", C.c_float),
                ("planar_voxel_filter_size", C.c_float), ("reserved", C.c_float), ("T_lidar_to_imu", C.c_double * 16)]


class PreprocessResult(C.Structure):
    """fls_preprocess_result (include/fls_preprocess.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("imu_status", C.c_int32), ("cloud_start_us", C.c_uint64), ("cloud_end_us", C.c_uint64),
                ("n_raw", C.c_uint64), ("n_ordered", C.c_uint64), ("n_planar", C.c_uint64), ("n_planar_filtered", C.c_uint64),
                ("n_segment", C.c_uint64), ("filter_on_device", C.c_int32), ("reserved", C.c_int32)]


FLS_IMU_OK, FLS_IMU_DROP, FLS_IMU_WAIT, FLS_IMU_EMPTY_SEGMENT, FLS_IMU_EMPTY_CLOUD = range(5)


class DriverCloud(C.Structure):
    """fls_driver_cloud (include/fls_ingest.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("sensor", C.c_int32), ("point_step", C.c_uint32), ("is_dense", C.c_int32),
                ("x_offset", C.c_uint32), ("y_offset", C.c_uint32), ("z_offset", C.c_uint32), ("intensity_offset", C.c_uint32),
                ("ring_offset", C.c_uint32), ("time_offset", C.c_uint32), ("tag_offset", C.c_uint32), ("line_offset", C.c_uint32)]


class IngestParams(C.Structure):
    """fls_ingest_params (include/fls_ingest.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("vertical_scan_num", C.c_int32), ("lidar_point_time_scale", C.c_double),
                ("lower_angle", C.c_float), ("v_res", C.c_float)]


class IngestInfo(C.Structure):
    """fls_ingest_info (include/fls_ingest.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("timeless", C.c_int32), ("n_message", C.c_uint64), ("n_converted", C.c_uint64),
                ("time_min", C.c_float), ("time_max", C.c_float), ("time_last", C.c_float), ("reserved", C.c_int32), ("t0", C.c_double)]


# LidarModel::LidarSensorType, same order (FLS_SENSOR_*)
SENSOR_VELODYNE, SENSOR_OUSTER, SENSOR_LIVOX_AVIA, SENSOR_ROBOSENSE, SENSOR_LEISHEN, SENSOR_LIVOX_MID_360, SENSOR_NONE = range(7)
FLS_PRE_CONVERTED, FLS_PRE_CONVERTED_INDEX = 16, 17


def build(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of libfls_reg.so (cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC_DIR, "-s"] + (["-B"] if force else []))
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the registration hot path)")
        L = C.CDLL(LIB_PATH)
        fp = C.POINTER(C.c_float)
        dp = C.POINTER(C.c_double)
        ip = C.POINTER(C.c_int32)
        bp = C.POINTER(C.c_uint8)
        hp = C.c_void_p
        L.fls_create.restype = C.c_int
        L.fls_create.argtypes = [C.c_int, C.POINTER(Params), C.c_int, C.POINTER(hp)]
        L.fls_destroy.restype = None
        L.fls_destroy.argtypes = [hp]
        L.fls_add_cloud_to_local_map.restype = C.c_int
        L.fls_add_cloud_to_local_map.argtypes = [hp, fp, C.c_size_t, fp, C.c_size_t, C.c_int]
        L.fls_match.restype = C.c_int
        L.fls_match.argtypes = [hp, fp, C.c_size_t, fp, C.c_size_t, C.c_int, dp, C.c_int, C.POINTER(Stats)]
        L.fls_get_fitness_score.restype = C.c_int
        L.fls_get_fitness_score.argtypes = [hp, C.c_float, fp]
        L.fls_scan_upload.restype = C.c_int
        L.fls_scan_upload.argtypes = [hp, fp, C.c_size_t, fp, C.c_size_t, C.c_int]
        L.fls_map_image_bytes.restype = C.c_size_t
        L.fls_map_image_bytes.argtypes = [hp]
        L.fls_map_image_export.restype = C.c_int
        L.fls_map_image_export.argtypes = [hp, C.c_void_p, C.c_size_t, C.c_int]
        L.fls_map_image_import.restype = C.c_int
        L.fls_map_image_import.argtypes = [hp, C.c_void_p, C.c_size_t, C.c_int]
        L.fls_scan_upload_raw.restype = C.c_int
        L.fls_scan_upload_raw.argtypes = [hp, fp, C.c_size_t, fp, C.c_size_t, C.c_int]
        L.fls_match_resident.restype = C.c_int
        L.fls_match_resident.argtypes = [hp, dp, C.c_int, C.POINTER(Stats)]
        L.fls_match_batch.restype = C.c_int
        L.fls_match_batch.argtypes = [hp, C.c_size_t, C.POINTER(fp), C.POINTER(C.c_size_t), C.POINTER(fp), C.POINTER(C.c_size_t), C.c_int,
                                      dp, C.POINTER(Stats), ip, C.c_int]
        L.fls_replicas_create.restype = C.c_int
        L.fls_replicas_create.argtypes = [hp, ip, C.c_int, C.POINTER(C.c_void_p)]
        L.fls_replicas_refresh.restype = C.c_int
        L.fls_replicas_refresh.argtypes = [C.c_void_p]
        L.fls_replicas_match_batch.restype = C.c_int
        L.fls_replicas_match_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(fp), C.POINTER(C.c_size_t), C.POINTER(fp), C.POINTER(C.c_size_t), C.c_int,
                                               dp, C.POINTER(Stats), ip, C.c_int]
        L.fls_replicas_import_ms.restype = C.c_int
        L.fls_replicas_import_ms.argtypes = [C.c_void_p, dp, C.c_int]
        L.fls_replicas_destroy.restype = None
        L.fls_replicas_destroy.argtypes = [C.c_void_p]
        L.fls_get_iteration_log.restype = C.c_int
        L.fls_get_iteration_log.argtypes = [hp, dp, ip, dp, C.c_int]
        L.fls_get_correspondences.restype = C.c_int
        L.fls_get_correspondences.argtypes = [hp, C.c_int, ip, bp, bp, C.c_size_t]
        L.fls_map_size.restype = C.c_size_t
        L.fls_map_size.argtypes = [hp, C.c_int]
        L.fls_set_profiling.restype = C.c_int
        L.fls_set_profiling.argtypes = [hp, C.c_int]
        L.fls_get_kernel_time.restype = C.c_int
        L.fls_get_kernel_time.argtypes = [hp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        L.fls_get_traffic_counters.restype = C.c_int
        L.fls_get_traffic_counters.argtypes = [hp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.fls_map_export.restype = C.c_size_t
        L.fls_map_export.argtypes = [hp, C.c_void_p, C.c_size_t]
        L.fls_map_import.restype = C.c_int
        L.fls_map_import.argtypes = [hp, C.c_void_p, C.c_size_t]
        L.fls_ivox_blob_revision.restype = C.c_uint
        L.fls_ivox_blob_revision.argtypes = []
        L.fls_ivox_map_bytes.restype = C.c_size_t
        L.fls_ivox_map_bytes.argtypes = [hp]
        L.fls_ivox_map_export.restype = C.c_int
        L.fls_ivox_map_export.argtypes = [hp, C.c_void_p, C.c_size_t, C.c_int]
        L.fls_ivox_map_import.restype = C.c_int
        L.fls_ivox_map_import.argtypes = [hp, C.c_void_p, C.c_size_t, C.c_int]
        L.fls_loop_match.restype = C.c_int
        L.fls_loop_match.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_float),
                                     C.c_void_p]
        L.fls_voxel_grid_cloud.restype = C.c_int
        L.fls_voxel_grid_cloud.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_float, C.POINTER(C.c_float), C.c_size_t,
                                           C.POINTER(C.c_size_t)]
        L.fls_debug_voxel_grid.restype = C.c_int
        L.fls_debug_voxel_grid.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_float, C.POINTER(C.c_float), C.c_size_t,
                                           C.POINTER(C.c_size_t)]
        L.fls_debug_voxel_grid_timed.restype = C.c_int
        L.fls_debug_voxel_grid_timed.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_size_t)]
        L.fls_debug_exact_sort.restype = C.c_int
        L.fls_debug_exact_sort.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t, C.c_int]
        L.fls_debug_fullpiv_qr6.restype = C.c_int
        L.fls_debug_fullpiv_qr6.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
        L.fls_debug_ldlt6.restype = C.c_int
        L.fls_debug_ldlt6.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        L.fls_get_debug_stamps.restype = C.c_int
        L.fls_get_debug_stamps.argtypes = [hp, C.POINTER(C.c_int64)]
        L.fls_features_create.restype = C.c_int
        L.fls_features_create.argtypes = [C.POINTER(FeatureParams), C.c_int, C.POINTER(hp)]
        L.fls_features_destroy.restype = None
        L.fls_features_destroy.argtypes = [hp]
        L.fls_features_project.restype = C.c_int
        L.fls_features_project.argtypes = [hp, C.c_void_p, C.c_size_t, C.POINTER(PointLayout), C.POINTER(C.c_size_t)]
        L.fls_features_extract.restype = C.c_int
        L.fls_features_extract.argtypes = [hp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.fls_features_get.restype = C.c_size_t
        L.fls_features_get.argtypes = [hp, C.c_int, C.c_void_p, C.c_size_t]
        L.fls_features_get_time.restype = C.c_int
        L.fls_features_get_time.argtypes = [hp, dp, dp]
        u64p = C.POINTER(C.c_uint64)
        L.fls_preprocess_create.restype = C.c_int
        L.fls_preprocess_create.argtypes = [C.POINTER(PreprocessParams), C.c_int, C.POINTER(hp)]
        L.fls_preprocess_destroy.restype = None
        L.fls_preprocess_destroy.argtypes = [hp]
        L.fls_preprocess_scan.restype = C.c_int
        L.fls_preprocess_scan.argtypes = [hp, C.c_void_p, C.c_size_t, C.POINTER(RawLayout), C.c_uint64, u64p, dp, C.c_size_t, C.POINTER(PreprocessResult)]
        L.fls_preprocess_scan_device.restype = C.c_int
        L.fls_preprocess_scan_device.argtypes = L.fls_preprocess_scan.argtypes
        L.fls_scan_attach_preprocessed.restype = C.c_int
        L.fls_scan_attach_preprocessed.argtypes = [hp, hp, C.c_int]
        L.fls_preprocess_get_host_bytes.restype = C.c_int
        L.fls_preprocess_get_host_bytes.argtypes = [hp, u64p]
        L.fls_preprocess_get.restype = C.c_size_t
        L.fls_preprocess_get.argtypes = [hp, C.c_int, C.c_void_p, C.c_size_t]
        L.fls_preprocess_get_time.restype = C.c_int
        L.fls_preprocess_get_time.argtypes = [hp, dp, dp]
        L.fls_features_project_deskew.restype = C.c_int
        L.fls_features_project_deskew.argtypes = [hp, C.c_void_p, C.c_size_t, C.POINTER(RawLayout), C.c_uint64, u64p, dp, C.c_size_t, dp,
                                                  C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        if hasattr(L, "fls_features_device_revision"):  # (as fls_batch_ivox_revision below)
            L.fls_features_device_revision.restype = C.c_int
            L.fls_features_device_revision.argtypes = []
            L.fls_features_keep_on_device.restype = C.c_int
            L.fls_features_keep_on_device.argtypes = [hp, C.c_int]
            L.fls_features_get_host_bytes.restype = C.c_int
            L.fls_features_get_host_bytes.argtypes = [hp, u64p]
            L.fls_features_stat.restype = C.c_size_t
            L.fls_features_stat.argtypes = [hp, C.c_int]
            L.fls_scan_attach_features.restype = C.c_int
            L.fls_scan_attach_features.argtypes = [hp, hp, C.c_int]
        L.fls_ingest_revision.restype = C.c_int
        L.fls_ingest_revision.argtypes = []
        L.fls_ingest_default_layout.restype = C.c_int
        L.fls_ingest_default_layout.argtypes = [C.c_int, C.POINTER(DriverCloud)]
        L.fls_preprocess_scan_driver.restype = C.c_int
        L.fls_preprocess_scan_driver.argtypes = [hp, C.c_void_p, C.c_size_t, C.POINTER(DriverCloud), C.POINTER(IngestParams), C.c_uint64, u64p, dp,
                                                 C.c_size_t, C.c_int, C.POINTER(PreprocessResult), u64p, C.POINTER(IngestInfo)]
        L.fls_features_project_driver.restype = C.c_int
        L.fls_features_project_driver.argtypes = [hp, C.c_void_p, C.c_size_t, C.POINTER(DriverCloud), C.POINTER(IngestParams), C.c_uint64, u64p, dp,
                                                  C.c_size_t, dp, C.POINTER(C.c_size_t), C.POINTER(C.c_int), u64p, C.POINTER(IngestInfo)]
        szp = C.POINTER(C.c_size_t)
        L.fls_keyframes_revision.restype = C.c_int
        L.fls_keyframes_revision.argtypes = []
        L.fls_keyframes_create.restype = C.c_int
        L.fls_keyframes_create.argtypes = [C.c_int, C.POINTER(hp)]
        L.fls_keyframes_destroy.restype = None
        L.fls_keyframes_destroy.argtypes = [hp]
        L.fls_keyframes_add.restype = C.c_int
        L.fls_keyframes_add.argtypes = [hp, fp, C.c_size_t, C.c_int, ip]
        L.fls_keyframes_add_preprocessed.restype = C.c_int
        L.fls_keyframes_add_preprocessed.argtypes = [hp, hp, C.c_int, ip]
        L.fls_keyframes_count.restype = C.c_size_t
        L.fls_keyframes_count.argtypes = [hp]
        L.fls_keyframes_get.restype = C.c_int
        L.fls_keyframes_get.argtypes = [hp, C.c_int32, C.c_float, fp, C.c_size_t, szp]
        L.fls_keyframes_merge.restype = C.c_int
        L.fls_keyframes_merge.argtypes = [hp, ip, dp, C.c_size_t, C.c_float, C.c_float, fp, C.c_size_t, szp]
        L.fls_keyframes_loop_match.restype = C.c_int
        L.fls_keyframes_loop_match.argtypes = [hp, ip, dp, C.c_size_t, ip, dp, C.c_size_t, dp, fp, C.c_void_p]
        L.fls_keyframes_stat.restype = C.c_size_t
        L.fls_keyframes_stat.argtypes = [hp, C.c_int]
        if hasattr(L, "fls_localmap_revision"):  # (as fls_batch_ivox_revision below)
            L.fls_localmap_revision.restype = C.c_int
            L.fls_localmap_revision.argtypes = []
            L.fls_localmap_create.restype = C.c_int
            L.fls_localmap_create.argtypes = [C.c_int, C.POINTER(hp)]
            L.fls_localmap_destroy.restype = None
            L.fls_localmap_destroy.argtypes = [hp]
            L.fls_localmap_set_global.restype = C.c_int
            L.fls_localmap_set_global.argtypes = [hp, fp, C.c_size_t, C.c_int, C.c_float, szp]
            L.fls_localmap_crop.restype = C.c_int
            L.fls_localmap_crop.argtypes = [hp, dp, C.c_int, C.POINTER(C.c_int), szp]
            L.fls_localmap_split.restype = C.c_int
            L.fls_localmap_split.argtypes = [hp, C.c_double, szp]
            L.fls_localmap_add_tile.restype = C.c_int
            L.fls_localmap_add_tile.argtypes = [hp, C.c_double, C.c_int32, C.c_int32, fp, C.c_size_t, C.c_int]
            L.fls_localmap_tiles.restype = C.c_int
            L.fls_localmap_tiles.argtypes = [hp, ip, C.POINTER(C.c_uint32), C.c_size_t, szp]
            L.fls_localmap_get_tile.restype = C.c_int
            L.fls_localmap_get_tile.argtypes = [hp, C.c_int32, C.c_int32, C.c_float, fp, C.c_size_t, szp]
            L.fls_localmap_load_tiles.restype = C.c_int
            L.fls_localmap_load_tiles.argtypes = [hp, dp, C.c_float, C.POINTER(C.c_int), szp]
            L.fls_localmap_reset.restype = C.c_int
            L.fls_localmap_reset.argtypes = [hp]
            L.fls_localmap_get_local.restype = C.c_int
            L.fls_localmap_get_local.argtypes = [hp, fp, C.c_size_t, szp]
            L.fls_add_localmap_to_local_map.restype = C.c_int
            L.fls_add_localmap_to_local_map.argtypes = [hp, hp]
            L.fls_localmap_stat.restype = C.c_size_t
            L.fls_localmap_stat.argtypes = [hp, C.c_int]
        L.fls_batch_revision.restype = C.c_int
        L.fls_batch_revision.argtypes = []
        L.fls_match_batch_fused.restype = C.c_int
        L.fls_match_batch_fused.argtypes = L.fls_match_batch.argtypes
        L.fls_batch_stat.restype = C.c_size_t
        L.fls_batch_stat.argtypes = [hp, C.c_int]
        if hasattr(L, "fls_batch_ivox_revision"):  # (FLS_REG_LIB may name the parent commit's build in an A/B: calling what it lacks still raises)
            L.fls_batch_ivox_revision.restype = C.c_int
            L.fls_batch_ivox_revision.argtypes = []
            L.fls_match_batch_shared_ivox.restype = C.c_int
            L.fls_match_batch_shared_ivox.argtypes = L.fls_match_batch.argtypes
            L.fls_batch_ivox_stat.restype = C.c_size_t
            L.fls_batch_ivox_stat.argtypes = [hp, C.c_int]
        L.fls_debug_linalg_revision.restype = C.c_int
        L.fls_debug_linalg_revision.argtypes = []
        L.fls_debug_plane_fit_5x3.restype = C.c_int
        L.fls_debug_plane_fit_5x3.argtypes = [C.c_int, dp, C.c_int, dp]
        L.fls_debug_svd3.restype = C.c_int
        L.fls_debug_svd3.argtypes = [C.c_int, dp, C.c_int, dp, dp]
        L.fls_debug_lu6.restype = C.c_int
        L.fls_debug_lu6.argtypes = [C.c_int, dp, dp, C.c_int, dp, dp, dp]
        L.fls_debug_so3.restype = C.c_int
        L.fls_debug_so3.argtypes = [C.c_int, dp, dp, C.c_int, dp, dp, dp]
        L.fls_debug_wave_sum.restype = C.c_int
        L.fls_debug_wave_sum.argtypes = [C.c_int, dp, C.c_int, dp]
        if hasattr(L, "fls_debug_fit_revision"):  # (as fls_batch_ivox_revision above)
            u32p = C.POINTER(C.c_uint32)
            L.fls_debug_fit_revision.restype = C.c_int
            L.fls_debug_fit_revision.argtypes = []
            for f in (L.fls_debug_plane_residual, L.fls_debug_line_residual):
                f.restype = C.c_int
                f.argtypes = [C.c_int, dp, dp, dp, dp, dp, C.c_int, dp, dp, dp]
            L.fls_debug_icp_point_rows.restype = C.c_int
            L.fls_debug_icp_point_rows.argtypes = [C.c_int, dp, dp, dp, C.c_int, dp, dp, dp]
            for f in (L.fls_debug_rank1_mfma, L.fls_debug_rank1_dpp, L.fls_debug_rank1x3_mfma):
                f.restype = C.c_int
                f.argtypes = [C.c_int, dp, dp, dp, C.c_int, dp]
            L.fls_debug_reduce_partials.restype = C.c_int
            L.fls_debug_reduce_partials.argtypes = [C.c_int, C.c_int, dp, C.c_int, dp]
            L.fls_debug_fanin.restype = C.c_int
            L.fls_debug_fanin.argtypes = [C.c_int, C.c_int, C.c_int, dp, u32p, u32p]
            L.fls_debug_last_system.restype = C.c_int
            L.fls_debug_last_system.argtypes = [hp, dp, dp]
        if hasattr(L, "fls_debug_ndt_revision"):  # (as fls_batch_ivox_revision above)
            L.fls_debug_ndt_revision.restype = C.c_int
            L.fls_debug_ndt_revision.argtypes = []
            L.fls_debug_ndt_voxels.restype = C.c_int
            L.fls_debug_ndt_voxels.argtypes = [hp, C.c_size_t, ip, ip, ip, bp, bp, dp, dp, dp, C.POINTER(C.c_size_t)]
        if hasattr(L, "fls_debug_loop_revision"):  # (as fls_batch_ivox_revision above)
            i64p = C.POINTER(C.c_int64)
            L.fls_debug_loop_revision.restype = C.c_int
            L.fls_debug_loop_revision.argtypes = []
            L.fls_debug_loop_ndt.restype = C.c_int
            L.fls_debug_loop_ndt.argtypes = [C.c_int, fp, C.c_int, fp, C.c_int, C.c_int, C.c_float, dp, C.c_int, dp, dp, dp, i64p, ip, ip]
            L.fls_debug_loop_gicp_cov.restype = C.c_int
            L.fls_debug_loop_gicp_cov.argtypes = [C.c_int, fp, C.c_int, C.c_int, C.c_float, C.c_double, C.c_int, dp]
            L.fls_debug_loop_gicp_corr.restype = C.c_int
            L.fls_debug_loop_gicp_corr.argtypes = [C.c_int, fp, C.c_int, fp, C.c_int, C.c_int, fp, dp, dp, dp, C.c_double, C.c_int, ip, dp]
            L.fls_debug_loop_gicp_fdf.restype = C.c_int
            L.fls_debug_loop_gicp_fdf.argtypes = [C.c_int, fp, C.c_int, fp, C.c_int, C.c_int, dp, ip, dp, C.c_int, dp]
            L.fls_debug_loop_fitness.restype = C.c_int
            L.fls_debug_loop_fitness.argtypes = [C.c_int, fp, C.c_int, fp, C.c_int, C.c_int, fp, C.c_int, dp, i64p]
        if hasattr(L, "fls_loop_device_revision"):  # (as fls_batch_ivox_revision above)
            i64p = C.POINTER(C.c_int64)
            vp = C.c_void_p  # device pointers
            L.fls_loop_device_revision.restype = C.c_int
            L.fls_loop_device_revision.argtypes = []
            L.fls_loop_match_device.restype = C.c_int
            L.fls_loop_match_device.argtypes = [C.c_int, vp, vp, vp, vp, C.c_size_t, vp, vp, vp, vp, C.c_size_t, dp, fp, C.c_void_p]
            L.fls_keyframes_loop_match_device.restype = C.c_int
            L.fls_keyframes_loop_match_device.argtypes = L.fls_keyframes_loop_match.argtypes
            L.fls_loop_device_stat.restype = C.c_size_t
            L.fls_loop_device_stat.argtypes = [C.c_int, C.c_int]
            L.fls_debug_loop_leaves_revision.restype = C.c_int
            L.fls_debug_loop_leaves_revision.argtypes = []
            L.fls_debug_loop_leaves.restype = C.c_int
            L.fls_debug_loop_leaves.argtypes = [C.c_int, fp, C.c_int, C.c_int, C.c_float, C.c_int, ip, ip, dp, dp, fp, C.c_int, ip, ip]
            L.fls_debug_loop_ndt_device.restype = C.c_int
            L.fls_debug_loop_ndt_device.argtypes = [C.c_int, fp, C.c_int, fp, C.c_int, C.c_int, C.c_float, dp, C.c_int, dp, dp, dp, i64p, ip, ip]
        if hasattr(L, "fls_debug_knn_revision"):  # (as fls_batch_ivox_revision above)
            L.fls_debug_knn_revision.restype = C.c_int
            L.fls_debug_knn_revision.argtypes = []
            L.fls_debug_grid_knn5.restype = C.c_int
            L.fls_debug_grid_knn5.argtypes = [C.c_int, fp, C.c_int, fp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, dp, C.c_int, fp, bp, fp, ip]
            L.fls_debug_grid_knn5_dual.restype = C.c_int
            L.fls_debug_grid_knn5_dual.argtypes = [C.c_int, fp, C.c_int, fp, C.c_int, C.c_float, C.c_int, C.c_float, fp, C.c_int, fp, C.c_int, C.c_float, C.c_int,
                                                   C.c_float, C.c_int, dp, C.c_int, fp, bp, fp, ip, fp, bp, fp, ip]
            L.fls_debug_icp_knn1.restype = C.c_int
            L.fls_debug_icp_knn1.argtypes = [C.c_int, fp, C.c_int, fp, C.c_int, C.c_int, C.c_float, C.c_double, dp, C.c_int, ip, bp, ip]
        if hasattr(L, "fls_debug_ivox_knn_revision"):  # (as fls_batch_ivox_revision above)
            L.fls_debug_ivox_knn_revision.restype = C.c_int
            L.fls_debug_ivox_knn_revision.argtypes = []
            L.fls_debug_ivox_knn_limits.restype = C.c_int
            L.fls_debug_ivox_knn_limits.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        if hasattr(L, "fls_debug_ivox_update_revision"):  # (as fls_batch_ivox_revision above)
            L.fls_debug_ivox_update_revision.restype = C.c_int
            L.fls_debug_ivox_update_revision.argtypes = []
            L.fls_debug_ivox_add_points.restype = C.c_int
            L.fls_debug_ivox_add_points.argtypes = [hp, fp, bp, C.c_size_t, C.POINTER(C.c_uint32)]
        if hasattr(L, "fls_debug_ivox_decide_revision"):  # (as fls_batch_ivox_revision above)
            u32p = C.POINTER(C.c_uint32)
            L.fls_debug_ivox_decide_revision.restype = C.c_int
            L.fls_debug_ivox_decide_revision.argtypes = []
            L.fls_debug_ivox_decide.restype = C.c_int
            L.fls_debug_ivox_decide.argtypes = [C.c_int, fp, C.c_int, dp, C.c_double, fp, bp, C.c_int, u32p, fp, C.c_int, fp, C.c_int, C.c_int,
                                                C.POINTER(DebugIvoxGate), bp, fp, u32p, u32p, u32p]
            L.fls_debug_ivox_nn_materialize.restype = C.c_int
            L.fls_debug_ivox_nn_materialize.argtypes = [C.c_int, u32p, bp, C.c_int, fp, C.c_int, fp, fp]
            L.fls_debug_ivox_decide_host.restype = C.c_int
            L.fls_debug_ivox_decide_host.argtypes = [fp, dp, C.c_double, fp, bp, C.c_int, bp, fp]
        if hasattr(L, "fls_debug_tail_revision"):  # (as fls_batch_ivox_revision above)
            L.fls_debug_tail_revision.restype = C.c_int
            L.fls_debug_tail_revision.argtypes = []
            L.fls_debug_loam_tail.restype = C.c_int
            L.fls_debug_loam_tail.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_void_p, dp, C.c_int, dp, C.c_int, C.c_double, C.c_double, C.c_uint32, C.c_void_p]
            L.fls_debug_lu_tail.restype = C.c_int
            L.fls_debug_lu_tail.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_void_p, dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_uint32, C.c_void_p]
        if hasattr(L, "fls_ndt_image_revision"):  # (as fls_batch_ivox_revision above)
            L.fls_ndt_image_revision.restype = C.c_int
            L.fls_ndt_image_revision.argtypes = []
        if hasattr(L, "fls_kd_image_revision"):  # (as fls_batch_ivox_revision above)
            L.fls_kd_image_revision.restype = C.c_int
            L.fls_kd_image_revision.argtypes = []
            L.fls_replicas_match_batch_fused.restype = C.c_int
            L.fls_replicas_match_batch_fused.argtypes = L.fls_replicas_match_batch.argtypes
        if hasattr(L, "fls_knn_order_revision"):  # (as fls_batch_ivox_revision above)
            L.fls_knn_order_revision.restype = C.c_int
            L.fls_knn_order_revision.argtypes = []
            L.fls_set_knn_order.restype = C.c_int
            L.fls_set_knn_order.argtypes = [hp, C.c_int]
            L.fls_get_knn_order.restype = C.c_int
            L.fls_get_knn_order.argtypes = [hp, C.POINTER(C.c_int)]
            L.fls_knn_order_limits.restype = C.c_int
            L.fls_knn_order_limits.argtypes = [C.POINTER(C.c_int)]
        L.fls_status_string.restype = C.c_char_p
        L.fls_status_string.argtypes = [C.c_int]
        L.fls_abi_version.restype = C.c_int
        L.fls_abi_revision.restype = C.c_int
        L.fls_device_count.restype = C.c_int
        _lib = L
    return _lib


def status_string(s: int) -> str:
    return lib().fls_status_string(int(s)).decode()


def knn_order_limit() -> int:
    """fls_knn_order_limits: W, the records of one query's work array in the reference neighbour order (include/fls_knn_order.h)."""
    w = C.c_int(0)
    rc = lib().fls_knn_order_limits(C.byref(w))
    if rc != FLS_OK:
        raise FlsError(rc, "fls_knn_order_limits")
    return int(w.value)


def device_count() -> int:
    return int(lib().fls_device_count())
