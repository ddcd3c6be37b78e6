"""The bookkeeping of the kd-tree kinds' lazy host deque (csrc/kd_lazy_deque.hpp) as a stand-alone program
(tests/host/kd_push_model_test.cpp): 200 seeded random sequences of push-device, push-host, trim, reset, fetch and import against a plain
std::deque of vectors, host arrays standing in for the device ring.  No GPU: host code only, compiled with hipcc because the product
headers include the HIP headers; no HIP runtime call is made.  The program runs twice, the second time built with AddressSanitizer and
UBSan on the host side.  The counter slots of the device push are held against include/fls_reg.h here as well."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "kd_push_model_test.cpp")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])])
def test_lazy_deque_against_a_plain_deque(name, flags, tmp_path):
    exe = os.path.join(str(tmp_path), "kd_push_model_test_" + name)
    subprocess.check_call(HIPCC + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_the_counter_slots_are_documented():
    doc = open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    for slot in ("164 = ", "165 = ", "166 = ", "167 = "):
        assert slot in doc, slot
    assert "FLS_KD_DEVICE_PUSH=0" in doc and "#define FLS_ABI_REVISION 9" in doc
