"""include/fls_localmap.h without a GPU: every declared symbol is exported by both libraries and listed, the lists do not overlap, the
header's own revision is 1 while the ABI revision and the existing symbol lists stay what they were, invalid arguments are refused before
the device is looked at, the C++ adapter builds with -Wall -Werror against the stand-in headers, and the kernels compile for gfx950
without scratch or spills."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
KERNELS = ("lm_crop_count_kernel", "lm_scan_counts_kernel", "lm_crop_scatter_kernel", "lm_bounds_kernel", "lm_tile_minmax_kernel", "lm_tile_keys_kernel",
           "lm_tile_heads_kernel", "lm_gather4_kernel", "lm_stitch_kernel")


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_localmap_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    declared = _declared("fls_localmap.h")
    assert len(declared) == 14 and declared == set(_lib.LOCALMAP_SYMBOLS) and len(_lib.LOCALMAP_SYMBOLS) == 14
    for s in declared:
        assert hasattr(L, s) and hasattr(dpp, s), s
    assert L.fls_localmap_revision() == 1 and dpp.fls_localmap_revision() == 1
    assert "#define FLS_LOCALMAP_REVISION 1" in open(os.path.join(ROOT, "include", "fls_localmap.h")).read()


def test_existing_abi_is_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1 and L.fls_keyframes_revision() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    assert set(_lib.EXPORTED_SYMBOLS) == _declared("fls_reg.h") | _declared("fls_features.h") and len(_lib.EXPORTED_SYMBOLS) == 44
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS +
              _lib.BATCH_SYMBOLS + _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS + _lib.NDT_IMAGE_SYMBOLS + _lib.KD_IMAGE_SYMBOLS)
    assert not set(_lib.LOCALMAP_SYMBOLS) & set(others)
    assert (len(_lib.PREPROCESS_SYMBOLS), len(_lib.INGEST_SYMBOLS), len(_lib.KEYFRAMES_SYMBOLS), len(_lib.BATCH_SYMBOLS), len(_lib.BATCH_IVOX_SYMBOLS),
            len(_lib.KD_IMAGE_SYMBOLS)) == (9, 4, 10, 3, 3, 2)


def test_localmap_invalid_arguments_need_no_device(built):
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    pts = np.zeros((4, 4), np.float32)
    p = pts.ctypes.data_as(FP)
    n, upd = C.c_size_t(99), C.c_int(7)
    T = np.eye(4).reshape(-1).copy()
    Tp = T.ctypes.data_as(DP)
    bad_T = T.copy(); bad_T[13] = np.inf
    nan_T = T.copy(); nan_T[12] = np.nan
    idx, cnt = np.zeros(2, np.int32), np.zeros(1, np.uint32)
    fake = C.c_void_p(1)  # never dereferenced: the argument checks below come first
    f32 = np.float32
    assert L.fls_localmap_create(0, None) == inv
    assert L.fls_localmap_set_global(None, p, 4, 4, f32(0), C.byref(n)) == inv and n.value == 99
    assert L.fls_localmap_set_global(fake, p, 4, 2, f32(0), C.byref(n)) == inv  # stride_floats < 3
    assert L.fls_localmap_set_global(fake, None, 4, 4, f32(0), C.byref(n)) == inv
    assert L.fls_localmap_set_global(fake, p, 4, 4, f32(-0.3), C.byref(n)) == inv
    assert L.fls_localmap_set_global(fake, p, 4, 4, f32(np.nan), C.byref(n)) == inv and n.value == 99
    assert L.fls_localmap_crop(None, Tp, 0, C.byref(upd), C.byref(n)) == inv
    assert L.fls_localmap_crop(fake, None, 0, C.byref(upd), C.byref(n)) == inv
    assert L.fls_localmap_crop(fake, Tp, 0, None, C.byref(n)) == inv and L.fls_localmap_crop(fake, Tp, 0, C.byref(upd), None) == inv
    assert L.fls_localmap_crop(fake, bad_T.ctypes.data_as(DP), 0, C.byref(upd), C.byref(n)) == inv
    assert L.fls_localmap_crop(fake, nan_T.ctypes.data_as(DP), 1, C.byref(upd), C.byref(n)) == inv and (upd.value, n.value) == (7, 99)
    assert L.fls_localmap_split(None, 100.0, C.byref(n)) == inv and L.fls_localmap_split(fake, 100.0, None) == inv
    for g in (0.0, -100.0, float("nan"), float("inf")):
        assert L.fls_localmap_split(fake, g, C.byref(n)) == inv, g
        assert L.fls_localmap_add_tile(fake, g, 0, 0, p, 4, 4) == inv, g
    assert L.fls_localmap_add_tile(None, 100.0, 0, 0, p, 4, 4) == inv
    assert L.fls_localmap_add_tile(fake, 100.0, 0, 0, None, 4, 4) == inv and L.fls_localmap_add_tile(fake, 100.0, 0, 0, p, 4, 2) == inv
    assert L.fls_localmap_tiles(None, idx.ctypes.data_as(IP), cnt.ctypes.data_as(C.POINTER(C.c_uint32)), 1, C.byref(n)) == inv
    assert L.fls_localmap_tiles(fake, idx.ctypes.data_as(IP), cnt.ctypes.data_as(C.POINTER(C.c_uint32)), 1, None) == inv
    assert L.fls_localmap_tiles(fake, None, None, 1, C.byref(n)) == inv
    assert L.fls_localmap_get_tile(None, 0, 0, f32(0), p, 4, C.byref(n)) == inv and L.fls_localmap_get_tile(fake, 0, 0, f32(0), p, 4, None) == inv
    assert L.fls_localmap_get_tile(fake, 0, 0, f32(0), None, 4, C.byref(n)) == inv and L.fls_localmap_get_tile(fake, 0, 0, f32(-1), p, 4, C.byref(n)) == inv
    assert L.fls_localmap_load_tiles(None, Tp, f32(0.5), C.byref(upd), C.byref(n)) == inv
    assert L.fls_localmap_load_tiles(fake, None, f32(0.5), C.byref(upd), C.byref(n)) == inv
    assert L.fls_localmap_load_tiles(fake, Tp, f32(-0.5), C.byref(upd), C.byref(n)) == inv
    assert L.fls_localmap_load_tiles(fake, Tp, f32(np.inf), C.byref(upd), C.byref(n)) == inv
    assert L.fls_localmap_load_tiles(fake, bad_T.ctypes.data_as(DP), f32(0.5), C.byref(upd), C.byref(n)) == inv
    assert L.fls_localmap_load_tiles(fake, Tp, f32(0.5), None, C.byref(n)) == inv and L.fls_localmap_load_tiles(fake, Tp, f32(0.5), C.byref(upd), None) == inv
    assert L.fls_localmap_reset(None) == inv
    assert L.fls_localmap_get_local(None, p, 4, C.byref(n)) == inv and L.fls_localmap_get_local(fake, p, 4, None) == inv
    assert L.fls_localmap_get_local(fake, None, 4, C.byref(n)) == inv
    assert L.fls_add_localmap_to_local_map(None, fake) == inv and L.fls_add_localmap_to_local_map(fake, None) == inv
    assert (upd.value, n.value) == (7, 99)
    assert L.fls_localmap_stat(None, 0) == 0
    L.fls_localmap_destroy(None)


def test_localmap_create_needs_a_device(built):
    L = _lib.lib()
    h = C.c_void_p(123)
    if _lib.device_count() == 0:
        assert L.fls_localmap_create(0, C.byref(h)) == _lib.FLS_ERR_DEVICE and not h.value
    else:
        assert L.fls_localmap_create(10_000, C.byref(h)) == _lib.FLS_ERR_DEVICE and not h.value


def _build_smoke(tmp_path):
    exe = os.path.join(str(tmp_path), "localmap_smoke")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-invalid-offsetof", "-I" + os.path.join(ROOT, "tests", "stubs"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stubs", "localmap_smoke.cpp"), "-o", exe, "-L" + libdir,
                           "-lfls_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_localmap_adapter_compiles_and_links(built, tmp_path):
    out = subprocess.run([_build_smoke(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "localmap adapter compiled" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_localmap_adapter_runs_on_gpu(built, tmp_path):
    """Both branches of LoadLocalMap through HipLocalMapSource: the cut equals the box test bit for bit, both local maps go into a matcher."""
    out = subprocess.run([_build_smoke(tmp_path), "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok=1 same=1" in out.stdout, out.stdout + out.stderr


def test_localmap_kernels_use_no_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 on csrc/kernels_localmap.hpp: every kernel without scratch memory or spills, LDS within a few KiB."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the local-map kernels cannot be checked")
    src = tmp_path / "localmap_tu.hip"
    src.write_text('#include "kernels_localmap.hpp"\n' + "".join(f"void* use_{k} = (void*)&fls::{k};\n" for k in KERNELS))
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + _lib.CSRC_DIR,
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "localmap_tu.o")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    seen = {}
    for b in re.split(r"Function Name: ", out.stderr)[1:]:
        get = lambda key: int(re.search(key + r":\s*(\d+)", b).group(1))
        seen[b.split()[0]] = dict(scratch=get(r"ScratchSize \[bytes/lane\]"), vspill=get("VGPRs Spill"), sspill=get("SGPRs Spill"), lds=get(r"LDS Size \[bytes/block\]"))
    mine = {k: v for k, v in seen.items() if any(name in k for name in KERNELS)}
    print(mine)
    assert len(mine) == len(KERNELS), list(seen)
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["vspill"] == 0 and v["sspill"] == 0 and v["lds"] <= 8192, (k, v)
