"""Device local-map source (include/fls_localmap.h): the global map of a localization run and its tiles stay on the GPU, the local map of
a reload -- Localization::LoadLocalMap (src/slam/localization.cpp:306-410), crop-box branch or tile branch -- is cut or stitched there, and
`AddTo(matcher)` is matcher_->AddCloudToLocalMap({*local_map}) without a host round trip for the kinds whose maps are built on the device.

Poses are (4, 4) row-major matrices, as everywhere in this package; only the translation is read.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FlsError

_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int32)
STAT_SLOTS = ("global_points", "tiles", "tile_points", "crops_run", "crops_skipped", "tile_filters_run", "tile_filter_hits", "filters_declined",
              "stitches", "handovers_device", "handovers_host", "bytes_resident", "last_crop_or_stitch_ns")


def _rows(cloud) -> np.ndarray:
    a = np.ascontiguousarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("cloud must be (n, >=3) float32")
    return a


def _pose(pose) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(4, 4).T).reshape(-1)


class LocalMapSource:
    """One fls_localmap handle.  Not thread-safe."""

    def __init__(self, device_id: int = 0):
        self._h = C.c_void_p()
        rc = _lib.lib().fls_localmap_create(device_id, C.byref(self._h))
        if rc != _lib.FLS_OK:
            self._h = C.c_void_p()
            raise FlsError(rc, "fls_localmap_create")

    def _check(self, rc: int, where: str) -> None:
        if rc != _lib.FLS_OK:
            raise FlsError(rc, where)

    def SetGlobal(self, cloud, leaf: float = 0.0) -> int:
        """LoadGlobalMap + VoxelGridCloud(cloud, leaf) (leaf 0: the cloud as it is); returns the points stored."""
        a = _rows(cloud)
        n = C.c_size_t(0)
        self._check(_lib.lib().fls_localmap_set_global(self._h, a.ctypes.data_as(_FP), a.shape[0], a.shape[1], np.float32(leaf), C.byref(n)),
                    "fls_localmap_set_global")
        return int(n.value)

    def Crop(self, pose, force: bool = False):
        """LoadLocalMap's crop-box branch: (updated, points of the local map)."""
        T = _pose(pose)
        upd, n = C.c_int(0), C.c_size_t(0)
        self._check(_lib.lib().fls_localmap_crop(self._h, T.ctypes.data_as(_DP), 1 if force else 0, C.byref(upd), C.byref(n)), "fls_localmap_crop")
        return bool(upd.value), int(n.value)

    def Split(self, grid_size: float) -> int:
        """SplitMap::Split of the stored global cloud; returns the number of tiles."""
        n = C.c_size_t(0)
        self._check(_lib.lib().fls_localmap_split(self._h, float(grid_size), C.byref(n)), "fls_localmap_split")
        return int(n.value)

    def AddTile(self, grid_size: float, gx: int, gy: int, cloud) -> None:
        a = _rows(cloud)
        self._check(_lib.lib().fls_localmap_add_tile(self._h, float(grid_size), int(gx), int(gy), a.ctypes.data_as(_FP), a.shape[0], a.shape[1]),
                    "fls_localmap_add_tile")

    def Tiles(self):
        """((n, 2) int32 tile indices in LessGridIndex order, (n,) uint32 point counts)"""
        n = C.c_size_t(0)
        _lib.lib().fls_localmap_tiles(self._h, None, None, 0, C.byref(n))  # (too small on purpose: the count)
        idx = np.zeros((max(int(n.value), 1), 2), np.int32)
        cnt = np.zeros(max(int(n.value), 1), np.uint32)
        self._check(_lib.lib().fls_localmap_tiles(self._h, idx.ctypes.data_as(_IP), cnt.ctypes.data_as(C.POINTER(C.c_uint32)), idx.shape[0], C.byref(n)),
                    "fls_localmap_tiles")
        return idx[: n.value], cnt[: n.value]

    def GetTile(self, gx: int, gy: int, leaf: float = 0.0) -> np.ndarray:
        """(n, 4) xyzi rows of a tile: as split / added (leaf 0) or VoxelGridCloud(tile, leaf), cached on the device."""
        idx, cnt = self.Tiles()
        hit = np.flatnonzero((idx[:, 0] == int(gx)) & (idx[:, 1] == int(gy)))
        if hit.size == 0:
            raise FlsError(_lib.FLS_ERR_INVALID, "fls_localmap_get_tile")
        out = np.zeros((max(int(cnt[hit[0]]), 1), 4), np.float32)  # (a VoxelGrid never adds points)
        n = C.c_size_t(0)
        self._check(_lib.lib().fls_localmap_get_tile(self._h, int(gx), int(gy), np.float32(leaf), out.ctypes.data_as(_FP), out.shape[0], C.byref(n)),
                    "fls_localmap_get_tile")
        return out[: n.value]

    def LoadTiles(self, pose, leaf: float):
        """LoadLocalMap's tile branch: (updated, points of the local map)."""
        T = _pose(pose)
        upd, n = C.c_int(0), C.c_size_t(0)
        self._check(_lib.lib().fls_localmap_load_tiles(self._h, T.ctypes.data_as(_DP), np.float32(leaf), C.byref(upd), C.byref(n)), "fls_localmap_load_tiles")
        return bool(upd.value), int(n.value)

    def Reset(self) -> None:
        self._check(_lib.lib().fls_localmap_reset(self._h), "fls_localmap_reset")

    def Local(self) -> np.ndarray:
        """(n, 4) xyzi rows of the current local map"""
        L = _lib.lib()
        n = C.c_size_t(0)
        L.fls_localmap_get_local(self._h, None, 0, C.byref(n))  # (too small on purpose: the count)
        out = np.zeros((max(int(n.value), 1), 4), np.float32)
        self._check(L.fls_localmap_get_local(self._h, out.ctypes.data_as(_FP), out.shape[0], C.byref(n)), "fls_localmap_get_local")
        return out[: n.value]

    def AddTo(self, matcher) -> None:
        """matcher.AddCloudToLocalMap([self.Local()]), device to device where the matcher's map is built on the device"""
        self._check(_lib.lib().fls_add_localmap_to_local_map(matcher._h, self._h), "fls_add_localmap_to_local_map")

    def Stat(self, slot: int) -> int:
        return int(_lib.lib().fls_localmap_stat(self._h, int(slot)))

    def stats(self) -> dict:
        return {name: self.Stat(k) for k, name in enumerate(STAT_SLOTS)}

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().fls_localmap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
