"""Per-scan preprocessing on the GPU (include/fls_preprocess.h): the loop PreProcessing::Run() runs on every raw cloud before Match
(src/slam/preprocessing.cpp:86-223) -- the IMU segment of the sweep, IMU de-skew of every point, the range gate, the point-jump
subsample and the planar VoxelGrid.  The result is what the reference puts into a PointcloudCluster's ordered_cloud_ / planar_cloud_.

What Run() would do with the scan (drop it, wait for IMU, ...) is reported in `imu_status`, not acted on.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import DriverCloud, FlsError, IngestInfo, IngestParams, PreprocessParams, PreprocessResult, RawLayout

IMU_STATUS = {_lib.FLS_IMU_OK: "ok", _lib.FLS_IMU_DROP: "drop", _lib.FLS_IMU_WAIT: "wait", _lib.FLS_IMU_EMPTY_SEGMENT: "empty_segment",
              _lib.FLS_IMU_EMPTY_CLOUD: "empty_cloud"}
ARRAYS = {"ordered": (0, np.float32, 4), "ordered_index": (1, np.int32, 1), "planar": (2, np.float32, 4), "planar_filtered": (3, np.float32, 4),
          "segment_t": (4, np.uint64, 1), "segment_q": (5, np.float64, 4), "converted_index": (_lib.FLS_PRE_CONVERTED_INDEX, np.int32, 1)}


def raw_layout(dtype: np.dtype, need_ring: bool = False) -> RawLayout:
    """fls_raw_layout of a structured point dtype with x, y, z (consecutive floats), intensity and time (floats), ring (uint8 / uint16)."""
    f = dtype.fields
    if f is None or not all(k in f for k in ("x", "y", "z", "intensity", "time")):
        raise ValueError("raw cloud must be a structured array with x, y, z, intensity, time")
    if f["y"][1] != f["x"][1] + 4 or f["z"][1] != f["x"][1] + 8 or any(dtype[k] != np.float32 for k in ("x", "y", "z", "intensity", "time")):
        raise ValueError("x, y, z, intensity, time must be float32, x, y, z consecutive")
    ring_off, ring_bytes = 0, 0
    if "ring" in f:
        if dtype["ring"] not in (np.uint8, np.uint16):
            raise ValueError("ring must be uint8 or uint16")
        ring_off, ring_bytes = f["ring"][1], dtype["ring"].itemsize
    elif need_ring:
        raise ValueError("the projection needs a ring field")
    return RawLayout(dtype.itemsize, f["x"][1], f["intensity"][1], ring_off, ring_bytes, f["time"][1])


# the converted cloud fls_preprocess_get(FLS_PRE_CONVERTED) returns: PointXYZIRT, fls_raw_layout {32, 0, 16, 20, 1, 24}
CONVERTED_DTYPE = np.dtype({"names": ["x", "y", "z", "intensity", "ring", "time"], "formats": ["<f4", "<f4", "<f4", "<f4", "u1", "<f4"],
                            "offsets": [0, 4, 8, 16, 20, 24], "itemsize": 32})
_TIME_NAMES = ("time", "t", "timestamp")


def driver_cloud(dtype: np.dtype, sensor: int, is_dense: bool = True) -> DriverCloud:
    """fls_driver_cloud of a structured message dtype: x, y, z, intensity by name, the time field as `time`, `t` or `timestamp`, and
    ring / tag / line where the sensor has them.  Offsets and itemsize need not be aligned (the packed Livox message)."""
    f = dtype.fields
    if f is None or not all(k in f for k in ("x", "y", "z", "intensity")):
        raise ValueError("a driver message must be a structured array with x, y, z, intensity")
    off = {k: (f[k][1] if k in f else 0) for k in ("x", "y", "z", "intensity", "ring", "tag", "line")}
    t = next((f[k][1] for k in _TIME_NAMES if k in f), 0)
    return DriverCloud(C.sizeof(DriverCloud), int(sensor), dtype.itemsize, 1 if is_dense else 0, off["x"], off["y"], off["z"], off["intensity"],
                       off["ring"], t, off["tag"], off["line"])


def ingest_params(time_scale: float = 1.0, vertical_scan_num: int = 0, lower_angle: float = 0.0, v_res: float = 0.0) -> IngestParams:
    return IngestParams(C.sizeof(IngestParams), int(vertical_scan_num), float(time_scale), float(lower_angle), float(v_res))


def imu_arrays(t_us, q_xyzw):
    t = np.ascontiguousarray(t_us, dtype=np.uint64).reshape(-1)
    q = np.ascontiguousarray(q_xyzw, dtype=np.float64).reshape(-1, 4)
    if q.shape[0] != t.shape[0]:
        raise ValueError("one xyzw quaternion per IMU timestamp")
    return t, q


@dataclass
class PreprocessOutput:
    status: int              # fls_status of the call (FLS_OK / FLS_ERR_STATE)
    imu_status: str          # "ok", "drop", "wait", "empty_segment", "empty_cloud"
    cloud_start_us: int
    cloud_end_us: int
    ordered: np.ndarray      # (N, 4) xyzi, ordered_cloud_
    ordered_index: np.ndarray
    planar: np.ndarray       # (M, 4) planar_cloud_ before the VoxelGrid
    planar_filtered: np.ndarray
    filter_on_device: bool


class ScanPreprocessor:
    """One fls_preprocess handle.  Arguments = the configuration the reference's PreProcessing reads (lidar_use_min_dist_,
    lidar_use_max_dist_, lidar_point_jump_span_, planar_voxel_filter_size_, the lidar-to-IMU extrinsic)."""

    def __init__(self, min_distance, max_distance, lidar_point_jump_span=1, planar_voxel_filter_size=0.0, T_lidar_to_imu=None, device_id=0):
        T = np.eye(4) if T_lidar_to_imu is None else np.asarray(T_lidar_to_imu, dtype=np.float64)
        self.params = PreprocessParams(C.sizeof(PreprocessParams), int(lidar_point_jump_span), min_distance, max_distance, planar_voxel_filter_size, 0.0,
                                       (C.c_double * 16)(*T.reshape(4, 4).T.reshape(-1)))  # column-major
        self._h = C.c_void_p()
        rc = _lib.lib().fls_preprocess_create(C.byref(self.params), device_id, C.byref(self._h))
        if rc != _lib.FLS_OK:
            self._h = C.c_void_p()
            raise FlsError(rc, "fls_preprocess_create")

    def scan(self, raw: np.ndarray, stamp_us: int, imu_t_us, imu_q_xyzw) -> PreprocessOutput:
        """De-skew + preprocess one raw cloud.  Raises FlsError on invalid input; drop / wait come back as imu_status with empty clouds."""
        raw = np.ascontiguousarray(raw)
        lay = raw_layout(raw.dtype)
        t, q = imu_arrays(imu_t_us, imu_q_xyzw)
        res = PreprocessResult()
        res.struct_size = C.sizeof(PreprocessResult)
        rc = _lib.lib().fls_preprocess_scan(self._h, raw.ctypes.data, raw.shape[0], C.byref(lay), int(stamp_us),
                                            t.ctypes.data_as(C.POINTER(C.c_uint64)), q.ctypes.data_as(C.POINTER(C.c_double)), t.shape[0], C.byref(res))
        if rc not in (_lib.FLS_OK, _lib.FLS_ERR_STATE):
            raise FlsError(rc, "fls_preprocess_scan")
        self.last = res
        return self.output(rc)

    def scan_device(self, raw: np.ndarray, stamp_us: int, imu_t_us, imu_q_xyzw) -> PreprocessResult:
        """scan() with the clouds left in device memory (fls_preprocess_scan_device): returns the result struct (status in `.status`,
        counts, imu_status, filter_on_device); get() downloads an array on its first request; a matcher takes a cloud over with
        RegistrationInterface.attach_preprocessed(self, which)."""
        raw = np.ascontiguousarray(raw)
        lay = raw_layout(raw.dtype)
        t, q = imu_arrays(imu_t_us, imu_q_xyzw)
        res = PreprocessResult()
        res.struct_size = C.sizeof(PreprocessResult)
        rc = _lib.lib().fls_preprocess_scan_device(self._h, raw.ctypes.data, raw.shape[0], C.byref(lay), int(stamp_us),
                                                   t.ctypes.data_as(C.POINTER(C.c_uint64)), q.ctypes.data_as(C.POINTER(C.c_double)), t.shape[0], C.byref(res))
        if rc not in (_lib.FLS_OK, _lib.FLS_ERR_STATE):
            raise FlsError(rc, "fls_preprocess_scan_device")
        self.last = res
        res.status = rc
        return res

    def scan_driver(self, msg: np.ndarray, sensor: int, stamp_us: int, imu_t_us, imu_q_xyzw, ingest: IngestParams, keep_on_device: bool = False,
                    is_dense: bool = True, cloud: DriverCloud | None = None) -> PreprocessResult:
        """ConvertMessageToCloud on the device, then scan() / scan_device() on the converted cloud (fls_preprocess_scan_driver).  `msg`:
        the driver message as a structured array (see driver_cloud()).  Returns the result struct with `.status`; `self.stamp_out` is
        the header stamp the reference goes on with, `self.ingest_info` the conversion's summary; get("converted") /
        get("converted_index") return the converted cloud and the message index of each of its points."""
        msg = np.ascontiguousarray(msg)
        dc = driver_cloud(msg.dtype, sensor, is_dense) if cloud is None else cloud
        t, q = imu_arrays(imu_t_us, imu_q_xyzw)
        res = PreprocessResult()
        res.struct_size = C.sizeof(PreprocessResult)
        info = IngestInfo()
        info.struct_size = C.sizeof(IngestInfo)
        stamp_out = C.c_uint64()
        rc = _lib.lib().fls_preprocess_scan_driver(self._h, msg.ctypes.data, msg.shape[0], C.byref(dc), C.byref(ingest), int(stamp_us),
                                                   t.ctypes.data_as(C.POINTER(C.c_uint64)), q.ctypes.data_as(C.POINTER(C.c_double)), t.shape[0],
                                                   1 if keep_on_device else 0, C.byref(res), C.byref(stamp_out), C.byref(info))
        if rc not in (_lib.FLS_OK, _lib.FLS_ERR_STATE):
            raise FlsError(rc, "fls_preprocess_scan_driver")
        self.last, self.stamp_out, self.ingest_info = res, int(stamp_out.value), info
        res.status = rc
        return res

    def output(self, status: int | None = None) -> PreprocessOutput:
        """The PreprocessOutput of the last scan (after scan_device: downloads the four clouds)."""
        res = self.last
        rc = getattr(res, "status", _lib.FLS_OK) if status is None else status
        return PreprocessOutput(rc, IMU_STATUS[res.imu_status], int(res.cloud_start_us), int(res.cloud_end_us), self.get("ordered"),
                                self.get("ordered_index"), self.get("planar"), self.get("planar_filtered"), bool(res.filter_on_device))

    def host_bytes(self) -> int:
        """Bytes copied device -> host on behalf of the last scan so far (fls_preprocess_get_host_bytes), lazy downloads included."""
        n = C.c_uint64()
        rc = _lib.lib().fls_preprocess_get_host_bytes(self._h, C.byref(n))
        if rc != _lib.FLS_OK:
            raise FlsError(rc, "fls_preprocess_get_host_bytes")
        return int(n.value)

    def get(self, name: str) -> np.ndarray:
        if name == "converted":
            n = _lib.lib().fls_preprocess_get(self._h, _lib.FLS_PRE_CONVERTED, None, 0)
            rows = np.zeros(max(n, 1), dtype=CONVERTED_DTYPE)
            _lib.lib().fls_preprocess_get(self._h, _lib.FLS_PRE_CONVERTED, rows.ctypes.data, n)
            return rows[:n]
        what, dt, cols = ARRAYS[name]
        n = _lib.lib().fls_preprocess_get(self._h, what, None, 0)
        out = np.zeros((max(n, 1), cols), dtype=dt)
        _lib.lib().fls_preprocess_get(self._h, what, out.ctypes.data, n)
        out = out[:n]
        return out if cols > 1 else out.reshape(-1)

    def times_ms(self):
        """(upload + de-skew + compaction, planar VoxelGrid) device time of the last scan [ms]."""
        a, b = C.c_double(), C.c_double()
        _lib.lib().fls_preprocess_get_time(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def fill_cluster(self, cluster, raw: np.ndarray, stamp_us: int, imu_t_us, imu_q_xyzw) -> PreprocessOutput:
        """The non-LOAM branch of Run(): ordered_cloud_ and planar_cloud_ (filtered when a leaf size is set) of a PointcloudCluster."""
        out = self.scan(raw, stamp_us, imu_t_us, imu_q_xyzw)
        cluster.ordered_cloud_ = out.ordered
        cluster.planar_cloud_ = out.planar_filtered if self.params.planar_voxel_filter_size > 0 else out.planar
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().fls_preprocess_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
