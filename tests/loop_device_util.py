"""Shared by tests/test_gpu_loop_device.py and its child processes: clouds as x | y | z | intensity planes in device memory (hipMalloc through
ctypes, as tests/test_gpu_kd_image.py does), the two forms of the loop-closure Match on them, and the counters."""
import ctypes as C
import functools

import numpy as np

from funny_lidar_slam_amd import _lib, registration as reg


@functools.lru_cache(maxsize=None)
def hip():
    h = C.CDLL("libamdhip64.so")  # the runtime libfls_reg.so itself is linked against
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


class DevPlanes:
    """the columns of an (n, 3 | 4) float32 cloud as planes on the device, each in an allocation of its own, `skew` bytes into it (hipMalloc
    aligns to 256 bytes: skew 4 puts every plane 4 bytes off a 16-byte boundary); intensity=False: no fourth plane (NULL)"""

    def __init__(self, cloud, skew=0, intensity=True):
        c = np.ascontiguousarray(cloud, np.float32)
        self.n, self.bases, self.addr = c.shape[0], [], []
        for a in range(4 if intensity and c.shape[1] >= 4 else 3):
            col = np.ascontiguousarray(c[:, a])
            base = C.c_void_p()
            assert hip().hipMalloc(C.byref(base), col.nbytes + 64) == 0
            self.bases.append(base)
            self.addr.append(base.value + skew)
            if self.n:
                assert hip().hipMemcpy(base.value + skew, col.ctypes.data, col.nbytes, 1) == 0  # hipMemcpyHostToDevice (synchronous: complete on return)
        while len(self.addr) < 4:
            self.addr.append(None)

    def free(self):
        for b in self.bases:
            hip().hipFree(b)
        self.bases = []


def result(T, fitness, st):
    """what must be equal between the two forms: T as uint64 bits, the fitness as uint32 bits, the stats as bytes"""
    return T.view(np.uint64).tolist(), int(np.float32(fitness).view(np.uint32)), bytes(st).hex()


def match_rows(src, tgt, T0=None):
    T = np.eye(4) if T0 is None else np.array(T0, np.float64)
    f, st = reg.LoopClosureMatch(src, tgt, T)
    return T, f, st


def match_device(src, tgt, T0=None, skew=0, intensity=True):
    a, b = DevPlanes(src, skew, intensity), DevPlanes(tgt, skew, intensity)
    try:
        T = np.eye(4) if T0 is None else np.array(T0, np.float64)
        f, st = reg.LoopClosureMatchDevice(a.addr, a.n, b.addr, b.n, T)
    finally:
        a.free()
        b.free()
    return T, f, st


def stats():
    L = _lib.lib()
    return [int(L.fls_loop_device_stat(0, k)) for k in range(7)]


def delta(before):
    return [a - b for a, b in zip(stats(), before)]
