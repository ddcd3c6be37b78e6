"""include/fls_map_ivox.h against the library and its Python mirror (_lib.IVOX_BLOB_SYMBOLS, IvoxBlobHeader, IvoxBlobVoxel): symbols, revision,
header constants, record sizes.  No GPU: the calls made here are refused before a device is touched."""
import ctypes as C
import os
import re

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    return open(os.path.join(ROOT, "include", "fls_map_ivox.h")).read()


def test_symbols_and_revision(built):
    src = header_text()
    assert "#define FLS_IVOX_BLOB_REVISION 1" in src and '#define FLS_IVOX_BLOB_MAGIC "FLSIVOX1"' in src and "#define FLS_IVOX_BLOB_VERSION 1" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", code)) == set(_lib.IVOX_BLOB_SYMBOLS) and len(_lib.IVOX_BLOB_SYMBOLS) == 4
    L = _lib.lib()
    assert L.fls_ivox_blob_revision() == 1 and L.fls_abi_revision() == 9
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.LOCALMAP_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS +
              _lib.DEBUG_FIT_SYMBOLS + _lib.BATCH_SYMBOLS + _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS + _lib.NDT_IMAGE_SYMBOLS + _lib.KD_IMAGE_SYMBOLS)
    assert not set(_lib.IVOX_BLOB_SYMBOLS) & set(others)
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for name in _lib.IVOX_BLOB_SYMBOLS:
        assert hasattr(L, name) and hasattr(dpp, name), name


def test_the_records_and_their_python_mirror():
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert (_lib.IVOX_BLOB_MAGIC, _lib.IVOX_BLOB_VERSION) == (b"FLSIVOX1", 1)
    assert C.sizeof(_lib.IvoxBlobHeader) == _lib.IVOX_BLOB_HEADER_BYTES == 56
    assert C.sizeof(_lib.IvoxBlobVoxel) == _lib.IVOX_BLOB_VOXEL_BYTES == _lib.IVOX_BLOB_POINT_BYTES == 16
    for struct, cls in (("fls_ivox_blob_header", _lib.IvoxBlobHeader), ("fls_ivox_blob_voxel", _lib.IvoxBlobVoxel)):
        body = code[code.index("typedef struct " + struct):code.index("} " + struct)]
        assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [f[0] for f in cls._fields_], struct
    # field offsets as the C compiler lays them out (natural alignment, no padding): what the blob's readers rely on
    want = dict(magic=0, version=8, kind=12, resolution=16, is_first=20, capacity=24, n_voxels=32, n_points=40, next_id=48)
    assert {f[0]: getattr(_lib.IvoxBlobHeader, f[0]).offset for f in _lib.IvoxBlobHeader._fields_} == want
    # the sections start 8 bytes off a 16-byte boundary of the blob (the header documents it: the library shifts its staging buffer)
    assert _lib.IVOX_BLOB_HEADER_BYTES % 16 == 8 and _lib.IVOX_BLOB_HEADER_BYTES % 8 == 0


def test_no_device_needed_to_refuse_null_arguments(built):
    L = _lib.lib()
    assert L.fls_ivox_map_bytes(None) == 0
    assert L.fls_ivox_map_export(None, None, 0, 0) == _lib.FLS_ERR_INVALID and L.fls_ivox_map_export(None, None, 0, 1) == _lib.FLS_ERR_INVALID
    assert L.fls_ivox_map_import(None, None, 0, 0) == _lib.FLS_ERR_INVALID and L.fls_ivox_map_import(None, None, 0, 1) == _lib.FLS_ERR_INVALID
