"""include/fls_features_device.h without a GPU: every declared symbol is exported by both libraries and listed in FEATURES_DEVICE_SYMBOLS, the
header's revision is 1 while FLS_ABI_REVISION stays 9, NULL handles are refused, the C++ adapters' new members (HipFeatureFrontEnd::RunOnDevice /
FillCluster, HipRegistration::MatchFeatures) build with -Wall -Werror against the stand-in headers, and the gather kernel compiles for gfx950
without scratch or spills."""
import ctypes as C
import os
import re
import subprocess

import pytest

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = ["fls_features_device_revision", "fls_features_keep_on_device", "fls_features_get_host_bytes", "fls_features_stat", "fls_scan_attach_features"]


def test_symbols_exported_by_both_libraries_declared_and_listed(built):
    L = _lib.lib()
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    text = open(os.path.join(ROOT, "include", "fls_features_device.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))
    assert declared == set(DECLARED)
    assert sorted(_lib.FEATURES_DEVICE_SYMBOLS) == sorted(DECLARED)
    for s in DECLARED:
        assert hasattr(L, s) and hasattr(dpp, s), s
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.LOCALMAP_SYMBOLS + _lib.BATCH_SYMBOLS +
              _lib.BATCH_IVOX_SYMBOLS)
    assert not set(DECLARED) & set(others)
    assert "#define FLS_FEATURES_DEVICE_REVISION 1" in text
    assert L.fls_features_device_revision() == 1 and dpp.fls_features_device_revision() == 1
    assert L.fls_abi_revision() == 9
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()


def test_null_handles_are_invalid(built):
    L = _lib.lib()
    n = C.c_uint64(7)
    assert L.fls_features_keep_on_device(None, 1) == _lib.FLS_ERR_INVALID
    assert L.fls_features_get_host_bytes(None, C.byref(n)) == _lib.FLS_ERR_INVALID and n.value == 7
    assert L.fls_features_stat(None, 0) == 0
    assert L.fls_scan_attach_features(None, None, 1) == _lib.FLS_ERR_INVALID


def test_adapters_compile_and_link(built, tmp_path):
    exe = os.path.join(str(tmp_path), "features_device_smoke")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-invalid-offsetof", "-I" + os.path.join(ROOT, "tests", "stubs"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stubs", "features_device_smoke.cpp"), "-o", exe, "-L" + libdir,
                           "-lfls_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "features device adapters compiled; revision 1" in out.stdout, out.stdout + out.stderr


def test_gather_kernel_uses_no_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 on csrc/kernels_features_gather.hpp: no scratch memory, no register spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the gather kernel cannot be checked")
    src = tmp_path / "gather_tu.hip"
    src.write_text('#include "kernels_features_gather.hpp"\n')
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + _lib.CSRC_DIR, "-Rpass-analysis=kernel-resource-usage",
                          "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "gather_tu.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    blocks = [b for b in re.split(r"Function Name: ", out.stderr)[1:] if "feat_gather_kernel" in b.split()[0]]
    assert len(blocks) == 1, out.stderr
    get = lambda key: int(re.search(key + r":\s*(\d+)", blocks[0]).group(1))
    usage = dict(vgpr=get("VGPRs"), sgpr=get("SGPRs"), scratch=get(r"ScratchSize \[bytes/lane\]"), vspill=get("VGPRs Spill"), sspill=get("SGPRs Spill"))
    print(usage)
    assert usage["scratch"] == 0 and usage["vspill"] == 0 and usage["sspill"] == 0, usage
