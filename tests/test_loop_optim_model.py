"""The host optimisers of the loop-closure matcher (csrc/loop_optim.hpp) as a stand-alone program (tests/host/loop_optim_test.cpp) against the
oracle (oracle/flo_loop.h): svd_solve6 on seeded SPD, indefinite, rank-deficient and zero systems, ndt_align driven by the oracle's derivatives at
10 m and 2 m, gicp_estimate / Bfgs driven by the oracle's cost function -- counts, poses and solutions bit for bit, on a small synthetic pair.
No GPU: host code only, compiled with hipcc because the product headers include the HIP headers; no HIP runtime call is made.  The program runs
twice, the second time built with AddressSanitizer and UBSan on the host side."""
import os
import subprocess

import pytest

from tests import loopdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "loop_optim_test.cpp")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    src, tgt, _ = loopdata.make_pair(job=1, n_az=90, n_t=2, n_s=1)
    d = tmp_path_factory.mktemp("loop_optim")
    paths = [str(d / "source.f32"), str(d / "target.f32")]
    for path, cloud in zip(paths, (src, tgt)):
        cloud[:, :3].astype("<f4").tofile(path)
    return paths


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])])
def test_optimisers_equal_the_oracle(name, flags, tmp_path, pair):
    exe = os.path.join(str(tmp_path), "loop_optim_test_" + name)
    subprocess.check_call(HIPCC + flags + [SRC, "-o", exe])
    out = subprocess.run([exe] + pair, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "loop optimisers: 0 failures" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
