"""The reference's neighbour selection as csrc/knn_reference_order.hpp restates it, against the toolchain's own std::nth_element, as a
stand-alone program (tests/host/knn_reference_order_model_test.cpp): (a) the restated nth_element on every n in 1..300, nth in {0, 4, n - 1,
random}, keys of 1, 2, 3, 8 distinct values and all distinct, the whole permutation compared; (b) the same up to n = 4,096 on sequences an
adversary made bad for the median of three, where the depth-limit branch (heap select) has to be reached; (c) the whole GetClosestPoint replay
against a restatement written with std::vector and std::nth_element, on neighbourhoods of 19 voxels with 0..40 points on a 1/8 m lattice.
No GPU: host code only, built as tests/test_kd_push_model.py builds its program; the second build runs under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "knn_reference_order_model_test.cpp")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])])
def test_restated_selection_against_std_nth_element(name, flags, tmp_path):
    exe = os.path.join(str(tmp_path), "knn_reference_order_model_test_" + name)
    subprocess.check_call(HIPCC + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    depth = re.search(r"depth_limit_cases (\d+)", out.stdout)
    assert depth and int(depth.group(1)) > 0, out.stdout[-3000:]  # the heap-select branch was compared, not only the partition loop
