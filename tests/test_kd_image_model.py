"""The host side of the flat image of the kd-tree kinds' local maps (include/fls_map_kd.h, csrc/kd_image.hpp) as a stand-alone program
(tests/host/kd_image_model_test.cpp): the checks of an import over everything a header can be wrong in, sizes that overflow size_t
included, and deque -> bytes -> deque on 200 seeded random small deques.  No GPU: host code only, compiled with hipcc because the product
headers include the HIP headers; no HIP runtime call is made.  The program runs twice, the second time built with AddressSanitizer and UBSan
on the host side.  The Python mirror of the layout (_lib.kd_image_layout, KdImageHeader) is held against the C header here as well."""
import ctypes as C
import os
import re
import subprocess

import pytest

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "kd_image_model_test.cpp")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])])
def test_image_checks_and_deque_round_trip(name, flags, tmp_path):
    exe = os.path.join(str(tmp_path), "kd_image_model_test_" + name)
    subprocess.check_call(HIPCC + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_the_header_file_and_its_python_mirror(built):
    src = open(os.path.join(ROOT, "include", "fls_map_kd.h")).read()
    assert "#define FLS_KD_IMAGE_REVISION 1" in src and '#define FLS_KD_IMAGE_MAGIC "FLSKDM01"' in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", code)) == set(_lib.KD_IMAGE_SYMBOLS) and len(_lib.KD_IMAGE_SYMBOLS) == 2
    L = _lib.lib()
    assert L.fls_kd_image_revision() == 1 and L.fls_abi_revision() == 9 and L.fls_abi_version() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    assert len(_lib.EXPORTED_SYMBOLS) == 44 and len(_lib.BATCH_SYMBOLS) == 3
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS +
              _lib.BATCH_SYMBOLS + _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS + _lib.NDT_IMAGE_SYMBOLS)
    assert not set(_lib.KD_IMAGE_SYMBOLS) & set(others)
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for name in _lib.KD_IMAGE_SYMBOLS:
        assert hasattr(L, name) and hasattr(dpp, name), name
    # the struct: 224 bytes, fields in the header's order, no hidden padding
    assert C.sizeof(_lib.KdImageHeader) == _lib.KD_IMAGE_HEADER_BYTES == 224 and _lib.KD_IMAGE_HEADER_BYTES % 16 == 0
    body = code[code.index("typedef struct fls_kd_image_header"):code.index("} fls_kd_image_header")]
    names = re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    assert names == [f[0] for f in _lib.KdImageHeader._fields_]
    assert sum(C.sizeof(f[1]) for f in _lib.KdImageHeader._fields_) == 224
    assert _lib.KdImageHeader.gate_last_T.offset == 64 and _lib.KdImageHeader.n_clouds.offset == 192
    # the layout: every array on a 16-byte boundary, 4 bytes per cloud and 16 per point
    for n in (0, 1, 3, 4, 5, 1000):
        for clouds in (0, 1, 3, 4, 5):
            one = _lib.kd_image_layout([clouds], [n])
            two = _lib.kd_image_layout([clouds, 2], [n, 7])
            for lay in (one, two):
                assert all(v % 16 == 0 for v in lay["sizes"] + lay["rows"] + [lay["total"]])
            assert one["sizes"] == [224] and one["rows"][0] == 224 + ((4 * clouds + 15) & ~15) and one["total"] == one["rows"][0] + 16 * n
            assert two["sizes"][1] == one["total"] and two["rows"][1] == two["sizes"][1] + 16 and two["total"] == two["rows"][1] + 7 * 16
    assert _lib.kd_image_layout([0], [0])["total"] == 224 and _lib.kd_image_layout([0, 0], [0, 0])["total"] == 224


def test_no_device_needed_to_refuse_null_arguments(built):
    L = _lib.lib()
    assert L.fls_map_export(None, None, 0) == 0 and L.fls_map_image_bytes(None) == 0
    assert L.fls_map_import(None, None, 0) == _lib.FLS_ERR_INVALID
    assert L.fls_map_image_import(None, None, 0, 0) == _lib.FLS_ERR_INVALID and L.fls_map_image_export(None, None, 0, 0) == _lib.FLS_ERR_INVALID
    assert L.fls_replicas_match_batch_fused(None, 0, None, None, None, None, 4, None, None, None, 8) == _lib.FLS_ERR_INVALID
