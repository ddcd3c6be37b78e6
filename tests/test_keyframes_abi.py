"""include/fls_keyframes.h without a GPU: every declared symbol is exported and listed, the header's own revision is 1 while the ABI
revision and the symbol list of fls_reg.h / fls_features.h stay what they were, invalid arguments are refused before the device is
looked at, the C++ adapter builds with -Wall -Werror against the stand-in headers, and the merge kernel compiles for gfx950 without
scratch or spills."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_keyframe_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    declared = _declared("fls_keyframes.h")
    assert len(declared) == 10 and declared == set(_lib.KEYFRAMES_SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s
    assert L.fls_keyframes_revision() == 1
    assert "#define FLS_KEYFRAMES_REVISION 1" in open(os.path.join(ROOT, "include", "fls_keyframes.h")).read()


def test_existing_abi_is_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1 and L.fls_ingest_revision() == 1
    assert set(_lib.EXPORTED_SYMBOLS) == _declared("fls_reg.h") | _declared("fls_features.h")
    assert not any(s.startswith("fls_keyframes") for s in _lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS)
    assert len(_lib.EXPORTED_SYMBOLS) == 44


def test_keyframe_invalid_arguments_need_no_device(built):
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    pts = np.zeros((4, 4), np.float32)
    kid, n, fit = C.c_int32(-7), C.c_size_t(99), C.c_float(0)
    T = np.eye(4).reshape(-1).copy()
    fake = C.c_void_p(1)  # never dereferenced: the argument checks below come first
    assert L.fls_keyframes_create(0, None) == inv
    assert L.fls_keyframes_add(None, pts.ctypes.data_as(FP), 4, 4, C.byref(kid)) == inv and kid.value == -7
    assert L.fls_keyframes_add(fake, pts.ctypes.data_as(FP), 4, 2, C.byref(kid)) == inv  # stride_floats < 3
    assert L.fls_keyframes_add(fake, None, 4, 4, C.byref(kid)) == inv
    assert L.fls_keyframes_add(fake, pts.ctypes.data_as(FP), 4, 4, None) == inv and kid.value == -7
    assert L.fls_keyframes_add_preprocessed(None, None, 0, C.byref(kid)) == inv
    assert L.fls_keyframes_get(None, 0, np.float32(0), pts.ctypes.data_as(FP), 4, C.byref(n)) == inv and n.value == 99
    assert L.fls_keyframes_get(fake, 0, np.float32(0), pts.ctypes.data_as(FP), 4, None) == inv
    assert L.fls_keyframes_merge(None, None, None, 0, np.float32(0.2), np.float32(0), None, 0, C.byref(n)) == inv
    assert L.fls_keyframes_merge(fake, None, None, 0, np.float32(0.2), np.float32(0), None, 0, None) == inv
    assert L.fls_keyframes_merge(fake, None, None, 0, np.float32(-1), np.float32(0), None, 0, C.byref(n)) == inv
    assert L.fls_keyframes_merge(fake, None, None, 0, np.float32(0.2), np.float32(np.nan), None, 0, C.byref(n)) == inv
    assert L.fls_keyframes_merge(fake, None, None, 1, np.float32(0.2), np.float32(0), None, 0, C.byref(n)) == inv and n.value == 99
    assert L.fls_keyframes_loop_match(None, None, None, 0, None, None, 0, T.ctypes.data_as(DP), C.byref(fit), None) == inv
    assert L.fls_keyframes_loop_match(fake, None, None, 0, None, None, 0, None, C.byref(fit), None) == inv
    assert L.fls_keyframes_count(None) == 0 and L.fls_keyframes_stat(None, 0) == 0
    L.fls_keyframes_destroy(None)


def test_keyframes_create_needs_a_device(built):
    L = _lib.lib()
    h = C.c_void_p(123)
    if _lib.device_count() == 0:
        assert L.fls_keyframes_create(0, C.byref(h)) == _lib.FLS_ERR_DEVICE and not h.value
    else:
        assert L.fls_keyframes_create(10_000, C.byref(h)) == _lib.FLS_ERR_DEVICE and not h.value


def _build_smoke(tmp_path):
    exe = os.path.join(str(tmp_path), "keyframes_smoke")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-invalid-offsetof", "-I" + os.path.join(ROOT, "tests", "stubs"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stubs", "keyframes_smoke.cpp"), "-o", exe, "-L" + libdir,
                           "-lfls_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_keyframe_adapter_compiles_and_links(built, tmp_path):
    out = subprocess.run([_build_smoke(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "keyframe adapter compiled" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_keyframe_adapter_runs_on_gpu(built, tmp_path):
    """GetSubMap through HipKeyframeStore equals the exact filter + the float transform, bit for bit; MergeMap runs."""
    out = subprocess.run([_build_smoke(tmp_path), "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok=1 same=1" in out.stdout, out.stdout + out.stderr


def test_merge_kernel_uses_no_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 on csrc/kernels_keyframes.hpp: both forms of the merge kernel without scratch memory or spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the merge kernel cannot be checked")
    args = "(const fls::KfSegment*, unsigned, const unsigned*, unsigned, float4*, float*, float*, float*, float*);\n"
    src = tmp_path / "keyframes_tu.hip"
    src.write_text('#include "kernels_keyframes.hpp"\n' + "".join(f"template __global__ void fls::kf_merge_kernel<{b}>{args}" for b in ("true", "false")))
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + _lib.CSRC_DIR, "-Rpass-analysis=kernel-resource-usage",
                          "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "keyframes_tu.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    seen = {}
    for b in re.split(r"Function Name: ", out.stderr)[1:]:
        get = lambda key: int(re.search(key + r":\s*(\d+)", b).group(1))
        seen[b.split()[0]] = dict(scratch=get(r"ScratchSize \[bytes/lane\]"), vspill=get("VGPRs Spill"), sspill=get("SGPRs Spill"), lds=get(r"LDS Size \[bytes/block\]"))
    merge = {k: v for k, v in seen.items() if "kf_merge_kernel" in k}
    print(merge)
    assert len(merge) == 2, list(seen)
    for k, v in merge.items():
        assert v["scratch"] == 0 and v["vspill"] == 0 and v["sspill"] == 0 and 0 < v["lds"] <= 8192, (k, v)
