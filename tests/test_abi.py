"""The C-ABI shared library: loads, exports every symbol include/fls_reg.h declares, struct layouts agree with
the ctypes mirrors, argument validation works, and -- without a GPU -- every compute entry point fails
loudly instead of falling back to anything (no compute calls are made here)."""
import ctypes as C
import os
import re

import pytest

from funny_lidar_slam_amd import _lib
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    syms = set()
    for header in ("fls_reg.h", "fls_features.h"):
        src = open(os.path.join(ROOT, "include", header)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        syms |= set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))
    return sorted(syms)


def test_header_symbols_all_exported(built):
    L = _lib.lib()
    syms = declared_symbols()
    assert len(syms) >= 16
    for s in syms:
        assert hasattr(L, s), f"libfls_reg.so does not export {s}"
    assert sorted(_lib.EXPORTED_SYMBOLS) == syms
    assert L.fls_abi_version() == 1 and L.fls_abi_revision() >= 4  # (additive revisions: include/fls_reg.h)


def test_debug_linalg_hooks_declared_exported_and_listed(built):
    """include/fls_debug_linalg.h (test hooks of the device linear-algebra primitives): a revision of its own, every declared symbol exported and
    listed, FLS_ABI_REVISION and the symbol list of fls_reg.h untouched; arguments are validated before the device is looked at, n == 0 is OK."""
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fls_debug_linalg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))
    assert len(declared) == 6 and declared == set(_lib.DEBUG_LINALG_SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s
    assert "#define FLS_DEBUG_LINALG_REVISION 1" in src and L.fls_debug_linalg_revision() == 1 and L.fls_abi_revision() == 9
    assert not set(_lib.DEBUG_LINALG_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    a = (C.c_double * 64)()
    inv = _lib.FLS_ERR_INVALID
    assert L.fls_debug_plane_fit_5x3(0, None, 1, a) == inv and L.fls_debug_plane_fit_5x3(0, a, 1, None) == inv and L.fls_debug_plane_fit_5x3(0, a, -1, a) == inv
    assert L.fls_debug_svd3(0, None, 1, a, a) == inv and L.fls_debug_svd3(0, a, 1, None, a) == inv and L.fls_debug_svd3(0, a, 1, a, None) == inv
    assert L.fls_debug_lu6(0, a, None, 1, a, a, a) == inv and L.fls_debug_lu6(0, a, a, 1, None, a, a) == inv and L.fls_debug_lu6(0, a, a, -2, a, a, a) == inv
    assert L.fls_debug_so3(0, None, a, 1, a, a, a) == inv and L.fls_debug_so3(0, a, a, 1, a, a, None) == inv
    assert L.fls_debug_wave_sum(0, None, 1, a) == inv and L.fls_debug_wave_sum(0, a, 1, None) == inv
    assert L.fls_debug_plane_fit_5x3(0, a, 0, a) == 0 and L.fls_debug_svd3(0, a, 0, a, a) == 0 and L.fls_debug_lu6(0, a, a, 0, a, a, a) == 0
    assert L.fls_debug_so3(0, a, a, 0, a, a, a) == 0 and L.fls_debug_wave_sum(0, a, 0, a) == 0


def test_struct_layouts_match_header(built):
    src = open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    body = re.search(r"typedef struct fls_params \{(.*?)\} fls_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b([a-z_0-9]+)\s*;", body)
    assert names == [f[0] for f in _lib.Params._fields_]
    assert [f[0] for f in O.Params._fields_] == names  # the oracle mirrors the same layout independently
    assert C.sizeof(_lib.Params) == 128 and C.sizeof(_lib.Stats) == 96
    from funny_lidar_slam_amd import registration as reg
    assert C.sizeof(reg.LoopStats) == C.sizeof(O.LoopStats) == 256 and [f[0] for f in reg.LoopStats._fields_] == [f[0] for f in O.LoopStats._fields_]
    src = open(os.path.join(ROOT, "include", "fls_features.h")).read()
    body = re.search(r"typedef struct fls_feature_params \{(.*?)\} fls_feature_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"(?:uint32_t|int32_t|float)\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [f[0] for f in _lib.FeatureParams._fields_]
    assert C.sizeof(_lib.FeatureParams) == 40 and C.sizeof(_lib.PointLayout) == 16


def test_invalid_arguments_rejected(built):
    L = _lib.lib()
    h = C.c_void_p()
    p = _lib.Params(max_iterations=10, point_to_planar_thres=0.1, position_converge_thres=0.005, rotation_converge_thres=0.001)
    assert L.fls_create(_lib.P2PLANE_IVOX, None, 0, C.byref(h)) == _lib.FLS_ERR_INVALID
    bad = _lib.Params(max_iterations=10)
    bad.struct_size = 7
    assert L.fls_create(_lib.P2PLANE_IVOX, C.byref(bad), 0, C.byref(h)) == _lib.FLS_ERR_INVALID
    zero_iter = _lib.Params(max_iterations=0)
    assert L.fls_create(_lib.P2PLANE_IVOX, C.byref(zero_iter), 0, C.byref(h)) == _lib.FLS_ERR_INVALID
    assert L.fls_create(_lib.P2PLANE_IVOX, C.byref(p), 0, None) == _lib.FLS_ERR_INVALID
    assert L.fls_match_resident(None, None, 0, None) == _lib.FLS_ERR_INVALID
    assert L.fls_map_size(None, 0) == 0
    assert b"gfx950" in L.fls_status_string(_lib.FLS_ERR_DEVICE)


def test_no_cpu_fallback_without_gpu(built):
    L = _lib.lib()
    if L.fls_device_count() > 0:
        pytest.skip("a gfx950 device is visible; the no-GPU behaviour is checked on the CPU runner")
    h = C.c_void_p()
    p = _lib.Params(max_iterations=10, point_to_planar_thres=0.1, position_converge_thres=0.005, rotation_converge_thres=0.001)
    for kind in range(5):
        rc = L.fls_create(kind, C.byref(p), 0, C.byref(h))
        assert rc in (_lib.FLS_ERR_DEVICE, _lib.FLS_ERR_INVALID) and not h.value
    from funny_lidar_slam_amd import registration as reg
    with pytest.raises(_lib.FlsError):
        reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
    from funny_lidar_slam_amd import features
    with pytest.raises(_lib.FlsError):
        features.FeatureFrontEnd(1800, 64, 0.00349, 4.0, 100.0, 1.0, 0.1)


def test_product_does_not_reference_the_oracle():
    """The shipped package must not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "funny_lidar_slam_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hpp", ".hip", ".h", "Makefile")):
                txt = open(os.path.join(d, f), errors="ignore").read()
                assert "liboracle" not in txt and "flo_" not in txt and "from oracle" not in txt and "import oracle" not in txt, os.path.join(d, f)
    import subprocess
    out = subprocess.run(["ldd", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "oracle" not in out


REF_INCLUDE = "/root/reference/include"


def _build_adapter(tmp_path, real_headers=None):
    """real_headers: None = the reference's real headers when /root/reference exists (this container), else the stand-ins of
    tests/stubs (the GPU box has no /root/reference)."""
    import subprocess
    if real_headers is None:
        real_headers = os.path.isdir(os.path.join(REF_INCLUDE, "registration"))
    exe = os.path.join(str(tmp_path), "adapter_smoke_real" if real_headers else "adapter_smoke")
    if real_headers:
        incs = ["-DFLS_REAL_REFERENCE_HEADERS", "-w", "-I" + os.path.join(ROOT, "oracle", "ref_shim", "include"), "-I" + os.path.join(ROOT, "oracle"),
                "-I" + REF_INCLUDE]
    else:
        incs = ["-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs")]
    cmd = ["g++", "-std=c++17"] + incs + ["-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "adapter_smoke.cpp"), "-o", exe, "-L" + os.path.dirname(_lib.LIB_PATH), "-lfls_reg",
           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_cpp_adapter_compiles_and_links(built, tmp_path):
    """include/fls_hip_registration.h (RegistrationInterface on top of the C ABI) builds with plain g++ against the reference's
    REAL registration/registration_interface.h + common/data_type.h + lidar/pointcloud_cluster.h (through the Eigen / PCL / glog
    include shadow of oracle/ref_shim) when /root/reference exists, and against the stand-in headers everywhere; links to
    libfls_reg.so."""
    import subprocess
    for real in ([True, False] if os.path.isdir(os.path.join(REF_INCLUDE, "registration")) else [False]):
        exe = _build_adapter(tmp_path, real)
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0 and "adapter compiled" in out.stdout, (real, out.stdout, out.stderr)


@pytest.mark.gpu
def test_cpp_adapter_runs_on_gpu(built, tmp_path):
    import subprocess
    exe = _build_adapter(tmp_path)
    out = subprocess.run([exe, "run"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok=1" in out.stdout


def _build_features_adapter(tmp_path):
    import subprocess
    exe = os.path.join(str(tmp_path), "features_smoke")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-invalid-offsetof", "-I" + os.path.join(ROOT, "tests", "stubs"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "features_smoke.cpp"), "-o", exe, "-L" + os.path.dirname(_lib.LIB_PATH), "-lfls_reg",
           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_cpp_features_adapter_compiles_and_links(built, tmp_path):
    """include/fls_hip_features.h (the PointcloudProjector + FeatureExtractor drop-in) builds with plain g++ against the
    stand-in reference headers and links to libfls_reg.so."""
    import subprocess
    exe = _build_features_adapter(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "features adapter compiled" in out.stdout


@pytest.mark.gpu
def test_cpp_features_adapter_runs_on_gpu(built, tmp_path):
    """The C++ drop-in, fed a raw driver cloud from a file, returns exactly the clouds the Python binding returns."""
    import subprocess
    import numpy as np
    from funny_lidar_slam_amd import features, synth
    exe = _build_features_adapter(tmp_path)
    raw = synth.cast_raw_scan(synth.make_scene(), np.eye(4), rng=synth.rng_for(3, 0, 12), **synth.VELODYNE_64)
    inp, outp = os.path.join(str(tmp_path), "raw.bin"), os.path.join(str(tmp_path), "out")
    raw.tofile(inp)
    out = subprocess.run([exe, inp, outp], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    f = features.FeatureFrontEnd(1800, 64, float(np.float32(0.2) / np.float32(180.0) * np.float32(3.14159265358979323846)), 4.0, 100.0, 1.0, 0.1)
    f.project(raw)
    f.extract()
    for name in ("ordered", "corner", "planar"):
        got = np.fromfile(outp + "." + name, dtype=np.float32).reshape(-1, 4)
        assert np.array_equal(got, f.get(name)), name


def test_voxel_grid_cloud_exact_mode_equals_the_reference_filter_without_a_gpu(built):
    """fls_voxel_grid_cloud(FLS_VOXELGRID_EXACT) -- the VoxelGridCloud / preprocessing filter entry point (pointcloud_utility.h:216-271,
    preprocessing.cpp:224-237) -- is host code and must equal the oracle's pcl::VoxelGrid restatement (itself pinned by the compiled
    reference's replays) bit for bit: small cloud (sequential path), 120k points (worker pool), stride 8 (PCL rows), the
    "leaf size too small" case (input copied), non-finite points dropped."""
    import numpy as np
    from funny_lidar_slam_amd import registration as reg
    rng = np.random.default_rng(11)
    for n, leaf in ((3000, 0.4), (120000, 0.5), (120000, 0.2)):
        c = np.concatenate([rng.uniform(-40, 40, (n, 2)), rng.uniform(-2, 6, (n, 1)), rng.uniform(0, 255, (n, 1))], axis=1).astype(np.float32)
        c[::97, 0] = np.nan
        ref = O.voxel_grid(c, leaf)
        got = reg.VoxelGridCloud(c, leaf)
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (n, leaf)
        pcl = np.zeros((n, 8), np.float32)
        pcl[:, :3], pcl[:, 4] = c[:, :3], c[:, 3]
        assert np.array_equal(reg.VoxelGridCloud(pcl, leaf).view(np.uint32), ref.view(np.uint32))
    far = np.array([[0, 0, 0, 1], [1e6, 1e6, 1e6, 2]], np.float32)
    assert np.array_equal(reg.VoxelGridCloud(far, 0.1), np.asarray(O.voxel_grid(far, 0.1)))
    assert reg.VoxelGridCloud(np.zeros((0, 4), np.float32), 0.5).shape == (0, 4)
