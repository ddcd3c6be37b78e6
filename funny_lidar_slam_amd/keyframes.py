"""Device keyframe store (include/fls_keyframes.h): the keyframes' ordered clouds stay on the GPU, their VoxelGrid-filtered forms
are computed once per keyframe and leaf size, and a sub-map -- LoopClosure::GetSubMap (src/slam/loop_closure.cpp:179-231), the loops
of System::SaveMap and of the global-map publisher (src/slam/system.cpp:310-316, :884-892) -- is one launch.

The store keeps no poses: they change with every pose-graph optimisation and come in with every call.  `submap` composes
inv(ref) @ pose with numpy (np.linalg.inv and a float64 matmul): that rounding is numpy's, not Eigen's Matrix4d::inverse() and
product; the C++ adapter (include/fls_hip_keyframes.h) uses the real Eigen.  Everything after the composition -- the cast of R and t to
float, the transform, the filters, the order of the points -- is the reference's bit for bit.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FlsError

_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int32)
STAT_SLOTS = ("stored_points", "cached_clouds", "filters_run", "cache_hits", "filters_declined", "merge_launches", "bytes_resident",
              "last_merge_ns")


def _ids_poses(ids, poses):
    """(int32 ids, column-major float64 poses (n, 16)) from ids and (n, 4, 4) row-major matrices"""
    i = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if p.shape[0] != i.shape[0]:
        raise ValueError("one 4x4 pose per id")
    return i, np.ascontiguousarray(p.transpose(0, 2, 1)).reshape(-1, 16)


class KeyframeStore:
    """One fls_keyframes handle.  Not thread-safe."""

    def __init__(self, device_id: int = 0):
        self._h = C.c_void_p()
        rc = _lib.lib().fls_keyframes_create(device_id, C.byref(self._h))
        if rc != _lib.FLS_OK:
            self._h = C.c_void_p()
            raise FlsError(rc, "fls_keyframes_create")
        self._n = []  # points of every keyframe (sizes the result arrays)

    def __len__(self) -> int:
        return int(_lib.lib().fls_keyframes_count(self._h))

    def add(self, cloud: np.ndarray) -> int:
        """Store a keyframe's cloud, (n, 3 | 4 | 8) float32 rows; returns its id (0, 1, 2, ...)."""
        a = np.ascontiguousarray(cloud, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("cloud must be (n, >=3) float32")
        kid = C.c_int32(-1)
        rc = _lib.lib().fls_keyframes_add(self._h, a.ctypes.data_as(_FP), a.shape[0], a.shape[1], C.byref(kid))
        if rc != _lib.FLS_OK:
            raise FlsError(rc, "fls_keyframes_add")
        self._n.append(a.shape[0])
        return int(kid.value)

    def add_preprocessed(self, pre, which: str = "ordered") -> int:
        """Store a cloud of the last scan of a preprocess.ScanPreprocessor ("ordered", "planar" or "planar_filtered"), device to device."""
        what = {"ordered": 0, "planar": 2, "planar_filtered": 3}[which]
        kid = C.c_int32(-1)
        rc = _lib.lib().fls_keyframes_add_preprocessed(self._h, pre._h, what, C.byref(kid))
        if rc != _lib.FLS_OK:
            raise FlsError(rc, "fls_keyframes_add_preprocessed")
        n = C.c_size_t(0)
        _lib.lib().fls_keyframes_get(self._h, kid.value, np.float32(0), None, 0, C.byref(n))  # (too small on purpose: the count)
        self._n.append(int(n.value))
        return int(kid.value)

    def _stored(self, ids) -> int:
        """points stored under the ids: no result of get / merge is longer (a VoxelGrid never adds points); unknown ids count 0"""
        return sum(self._n[int(i)] for i in ids if 0 <= int(i) < len(self._n))

    def get(self, keyframe_id: int, leaf: float = 0.0) -> np.ndarray:
        """(n, 4) xyzi rows of a keyframe: the stored cloud (leaf 0) or VoxelGridCloud(cloud, leaf), cached on the device."""
        out = np.zeros((max(self._stored([keyframe_id]), 1), 4), np.float32)
        n = C.c_size_t(0)
        rc = _lib.lib().fls_keyframes_get(self._h, int(keyframe_id), np.float32(leaf), out.ctypes.data_as(_FP), out.shape[0], C.byref(n))
        if rc != _lib.FLS_OK:
            raise FlsError(rc, "fls_keyframes_get")
        return out[: n.value]

    def merge(self, ids, poses, leaf_each: float = 0.2, leaf_final: float = 0.0, capacity: int | None = None) -> np.ndarray:
        """concat_k TransformPointCloud(VoxelGridCloud(cloud[ids[k]], leaf_each), poses[k]), then VoxelGridCloud(.., leaf_final); a leaf
        of 0 skips that filter.  poses: (n, 4, 4).  (n_out, 4) xyzi rows.  capacity: rows to allocate (default: the points stored
        under the ids, which no result exceeds)."""
        i, p = _ids_poses(ids, poses)
        out = np.zeros((max(self._stored(i) if capacity is None else int(capacity), 1), 4), np.float32)
        n = C.c_size_t(0)
        rc = _lib.lib().fls_keyframes_merge(self._h, i.ctypes.data_as(_IP), p.ctypes.data_as(_DP), i.shape[0], np.float32(leaf_each),
                                            np.float32(leaf_final), out.ctypes.data_as(_FP), out.shape[0], C.byref(n))
        if rc != _lib.FLS_OK:
            raise FlsError(rc, "fls_keyframes_merge")
        return out[: n.value]

    @staticmethod
    def submap_selection(keyframe_id: int, left: int, right: int, use_local_pose: bool, poses):
        """The ids and poses LoopClosure::GetSubMap merges (loop_closure.cpp:186-215): keyframe_id - left .. keyframe_id + right clipped to
        the keyframes there are, each pose replaced by inv(poses[keyframe_id]) @ pose when use_local_pose (numpy's rounding)."""
        P = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        ids = [keyframe_id + i for i in range(-left, right + 1) if 0 <= keyframe_id + i < P.shape[0]]
        sel = P[ids]
        if use_local_pose:
            sel = np.linalg.inv(P[keyframe_id]) @ sel
        return np.asarray(ids, np.int32), sel

    def submap(self, keyframe_id: int, left: int, right: int, use_local_pose: bool, poses) -> np.ndarray:
        """LoopClosure::GetSubMap(keyframe_id, left, right, use_local_pose); poses: the pose of every keyframe, (count, 4, 4)."""
        ids, sel = self.submap_selection(keyframe_id, left, right, use_local_pose, poses)
        return self.merge(ids, sel, 0.2, 0.0)

    def loop_match(self, src_ids, src_poses, tgt_ids, tgt_poses, pose: np.ndarray, on_device: bool = False):
        """GetSubMap twice + LoopClosure::Match on the selections; `pose` (4, 4) is in/out like the reference's Mat4d&.  Returns
        (fitness, LoopStats), equal to registration.LoopClosureMatch on the two merge() results.  on_device: the sub-maps stay on the
        device and the Match starts from them there (fls_keyframes_loop_match_device): the same results, bit for bit."""
        from .registration import LoopStats
        si, sp = _ids_poses(src_ids, src_poses)
        ti, tp = _ids_poses(tgt_ids, tgt_poses)
        Tf = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(4, 4).T).reshape(-1).copy()
        fit = C.c_float()
        st = LoopStats()
        call = _lib.lib().fls_keyframes_loop_match_device if on_device else _lib.lib().fls_keyframes_loop_match
        rc = call(self._h, si.ctypes.data_as(_IP), sp.ctypes.data_as(_DP), si.shape[0], ti.ctypes.data_as(_IP), tp.ctypes.data_as(_DP), ti.shape[0],
                  Tf.ctypes.data_as(_DP), C.byref(fit), C.byref(st))
        if rc != _lib.FLS_OK:
            raise FlsError(rc, "fls_keyframes_loop_match_device" if on_device else "fls_keyframes_loop_match")
        pose[...] = Tf.reshape(4, 4).T
        return float(fit.value), st

    def stats(self) -> dict:
        L = _lib.lib()
        return {name: int(L.fls_keyframes_stat(self._h, k)) for k, name in enumerate(STAT_SLOTS)}

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().fls_keyframes_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
