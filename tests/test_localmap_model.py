"""The host logic of the device local-map source (csrc/localmap.hpp) as a stand-alone program (tests/host/localmap_model_test.cpp): the
hysteresis decision of the crop box, the edge and corner casts, the box test on its faces, the tile index of a pose, the enter / leave
rule of the resident tile set and the stitch table, hand-made and on 240 seeded random pose walks against a direct restatement of
Localization::LoadLocalMap.  No GPU: host code only, compiled with hipcc because the product headers include the HIP headers; no HIP
runtime call is made.  The program runs twice, the second time built with AddressSanitizer and UBSan on the host side."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "localmap_model_test.cpp")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])])
def test_decisions_and_random_walks(name, flags, tmp_path):
    exe = os.path.join(str(tmp_path), "localmap_model_test_" + name)
    subprocess.check_call(HIPCC + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "240 walks, mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
