"""The host side of the iVox blob built on the device (include/fls_map_ivox.h, csrc/ivox_blob.hpp) as a stand-alone program
(tests/host/ivox_blob_model_test.cpp): the header checks of an import over hand-made good and bad headers, sizes that wrap a 64-bit product
included, and the closed form of "a blob into an empty map" -- order, capacities, begins, stamps -- against HostIvox::assign_layout after the
mirror was loaded from the same records, for 300 seeded random voxel lists.  No GPU: host code only, compiled with hipcc because the product
headers include the HIP headers; no HIP runtime call is made.  The program runs twice, the second time built with AddressSanitizer and UBSan
on the host side."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ivox_blob_model_test.cpp")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])])
def test_header_checks_and_closed_form(name, flags, tmp_path):
    exe = os.path.join(str(tmp_path), "ivox_blob_model_test_" + name)
    subprocess.check_call(HIPCC + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
