"""The host side of the flat NDT map image (include/fls_map_ndt.h, csrc/ndt_image.hpp) as a stand-alone program
(tests/host/ndt_image_model_test.cpp): the header checks of an import over everything a header can be wrong in, sizes that overflow size_t
included, and mirror -> bytes -> mirror on 200 seeded random small maps.  No GPU: host code only, compiled with hipcc because the product
headers include the HIP headers; no HIP runtime call is made.  The program runs twice, the second time built with AddressSanitizer and UBSan
on the host side.  The Python mirror of the layout (_lib.ndt_image_layout, NdtImageHeader) is held against the C header here as well."""
import ctypes as C
import os
import re
import subprocess

import pytest

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ndt_image_model_test.cpp")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])])
def test_header_checks_and_mirror_round_trip(name, flags, tmp_path):
    exe = os.path.join(str(tmp_path), "ndt_image_model_test_" + name)
    subprocess.check_call(HIPCC + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_the_header_file_and_its_python_mirror(built):
    src = open(os.path.join(ROOT, "include", "fls_map_ndt.h")).read()
    assert "#define FLS_NDT_IMAGE_REVISION 1" in src and '#define FLS_NDT_IMAGE_MAGIC "FLSNDT01"' in src and "#define FLS_NDT_IMAGE_CARRY 8" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", code)) == set(_lib.NDT_IMAGE_SYMBOLS)
    L = _lib.lib()
    assert L.fls_ndt_image_revision() == 1 and L.fls_abi_revision() == 9
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS +
              _lib.BATCH_SYMBOLS + _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS)
    assert not set(_lib.NDT_IMAGE_SYMBOLS) & set(others)
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    assert hasattr(dpp, "fls_ndt_image_revision")
    # the struct: 64 bytes, fields in the header's order
    assert C.sizeof(_lib.NdtImageHeader) == _lib.NDT_IMAGE_HEADER_BYTES == 64
    body = code[code.index("typedef struct fls_ndt_image_header"):code.index("} fls_ndt_image_header")]
    names = re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    assert names == [f[0] for f in _lib.NdtImageHeader._fields_]
    # the layout: 378 bytes per voxel, every array on a 16-byte boundary
    for n in (0, 1, 2, 15, 16, 17, 1000):
        lay = _lib.ndt_image_layout(n)
        assert all(v % 16 == 0 for v in lay.values()) and 64 + 378 * n <= lay["total"] < 64 + 378 * n + 9 * 16
    assert _lib.ndt_image_layout(0)["total"] == 64


def test_no_device_needed_to_refuse_null_arguments(built):
    L = _lib.lib()
    assert L.fls_map_export(None, None, 0) == 0 and L.fls_map_image_bytes(None) == 0
    assert L.fls_map_import(None, None, 0) == _lib.FLS_ERR_INVALID
    assert L.fls_map_image_import(None, None, 0, 0) == _lib.FLS_ERR_INVALID and L.fls_map_image_export(None, None, 0, 0) == _lib.FLS_ERR_INVALID
