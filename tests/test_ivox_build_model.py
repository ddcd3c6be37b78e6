"""The closed form the device-side bulk build of the iVox map computes, restated on the host as a stable sort plus scans and
compared with the product's sequential insert and image layout (tests/host/ivox_build_model_test.cpp): hand-made clouds for every edge the
form has and 200 seeded random ones.  No GPU: host code only, compiled with hipcc because the product headers include the HIP headers; no
HIP runtime call is made.  The program runs twice, the second time built with AddressSanitizer and UBSan on the host side."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ivox_build_model_test.cpp")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])])
def test_bulk_build_closed_form_model(name, flags, tmp_path):
    exe = os.path.join(str(tmp_path), "ivox_build_model_test_" + name)
    subprocess.check_call(HIPCC + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    # the random clouds must have reached the decline side of the capacity rule as well as the build side
    assert "0 random clouds declined" not in out.stdout, out.stdout[-500:]
