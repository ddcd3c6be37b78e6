"""The iVox map update on constructed batches (csrc/kernels_ivox_update.hpp, IvoxMap::enqueue_update / await_update / fall_back, the host mirror's
journal scatter) against the sequential model of tests/ivox_update_cases.py.  Every history runs through fls_debug_ivox_add_points
(include/fls_debug_ivox_update.h), which applies a decided batch through the code Match(update_map=True) runs behind its decision launch.  After
the first cloud and after every batch the whole logical state (the FLSIVOX1 blob, byte for byte against the model's encoding) and the whole kNN-side
image (FLSIMG01 through check_image: every voxel's cell, every other cell empty, regions disjoint, every face / edge halo cell, every mirror brick,
the directory) are compared.  Two arms: the device update, and FLS_IVOX_DEVICE_UPDATE=0 (host mirror + journal scatter, a writer bound by the same
halo invariant).  Two ways to observe: ExportMapBlob (does not move the map) and ExportMap (a device-held map goes through to_mirror and back
through enter_device between batches).  In the device arm the path a batch takes -- applied on the device, short or long chain, evictions and
re-creations, or refused and for which reason -- is asserted from the model, not read off the handle.  Nothing here has a tolerance."""
import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg
from tests import ivox_update_cases as U
from tests.test_gpu_ndt_image import DevMem

pytestmark = pytest.mark.gpu

MODE, Y = "PointToPlane_IVOX", reg.YAML_NCLT_IVOX
ARMS = {"device": {}, "host": {"FLS_IVOX_DEVICE_UPDATE": "0"}}
PATH_SLOTS = (103, 104, 117, 119, 120, 121, 123, 126)
UPD_NEED_HOST, UPD_CONFLICT, UPD_FULL, UPD_OUTSIDE = 1, 2, 4, 8  # kernels_ivox_update.hpp kUpd*
# chain_limit, the largest case (a model loop over 934k points, 15 MB blobs), keeps one parametrisation
CASES = [(n, a, o) for n in U.NAMES for a in ARMS for o in ("blob", "mirror") if n != "chain_limit" or (a, o) == ("device", "blob")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"
    assert U.HDR.itemsize == _lib.IVOX_BLOB_HEADER_BYTES and U.VOX.itemsize == _lib.IVOX_BLOB_VOXEL_BYTES and U.PT.itemsize == _lib.IVOX_BLOB_POINT_BYTES


def make(monkeypatch, capacity=None, arm="device", loc=False, mode=MODE, y=Y):
    """the switches are read when the handle is created"""
    env = dict(ARMS[arm])
    if capacity is not None:
        env["FLS_IVOX_CAPACITY"] = str(capacity)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = reg.make_matcher(mode, y, is_localization_mode=loc)
    for k in env:
        monkeypatch.delenv(k)
    return m


def blob_of(m):
    """ExportMapBlob to host memory: it must not move the map (no mirror, no rebuild, no counter of slots 100-147)"""
    before = [m.map_size(s) for s in range(100, 148)]
    n = m.MapBlobBytes()
    out = np.full(n, 0xA5, np.uint8)
    m.ExportMapBlob(out.ctypes.data, n, False)
    assert [m.map_size(s) for s in range(100, 148)] == before
    return out


def image_of(m):
    n = m.MapImageBytes()
    assert n > 0
    out = np.zeros(n, np.uint8)
    m.ExportMapImage(out.ctypes.data, n, False)
    return out


def check_state(m, step, observe, where):
    """the handle against step = (BatchInfo, blob, voxels, next_id) of the model's replay"""
    _, want, vox, next_id = step
    got = blob_of(m) if observe == "blob" else m.ExportMap()
    if got.tobytes() != want.tobytes():  # say what differs before failing
        gh, gv = U.decode_blob(got)
        wh, wv = U.decode_blob(want)
        assert gh == wh, (where, "header", gh, wh)
        assert list(gv) == list(wv), (where, "voxels or their LRU order", [k for k in gv if k not in wv][:5], [k for k in wv if k not in gv][:5])
        bad = [k for k in wv if gv[k].tobytes() != wv[k].tobytes()]
        assert not bad, (where, "points of", bad[:3], gv[bad[0]], wv[bad[0]])
        raise AssertionError((where, "the blob differs from the model's encoding"))
    assert int(U.decode_blob(got)[0]["next_id"]) == next_id, where
    U.check_image(image_of(m), vox)
    assert m.map_size(102) == len(vox) and m.map_size() == sum(len(p) for p in vox.values()), where


def check_path(h, i, info, rc, dst, d, where):
    """device arm: what batch i (0-based) of history h must have done to the counters, from the model"""
    reasons = (d[119], d[120], d[121])
    if info.n_source > U.CHAIN_MAX_POINTS:
        assert dst == U.NO_CHAIN and (d[103], d[104], d[117], d[126]) == (0, 1, 0, 0) and reasons == (0, 0, 0), (where, hex(dst), d)
        return "host (beyond the chain)"
    if info.device_can_apply and i not in h.room:
        assert rc == _lib.FLS_OK and dst == 0, (where, "the device refused a batch the model admits", rc, hex(dst), d)
        assert (d[103], d[104], d[117], d[126]) == (1, 0, info.n_evicted, info.n_recreated) and reasons == (0, 0, 0), (where, d, info.n_evicted, info.n_recreated)
        assert d[123] == (1 if info.short_chain else 0), (where, "short chain", d[123], info.short_chain)
        return "device, short chain" if info.short_chain else "device, long chain"
    assert dst not in (0, U.NO_CHAIN), (where, "the device applied a batch the model rejects", hex(dst))
    assert (d[103], d[104], d[117], d[126]) == (0, 1, 0, 0) and d[123] == (1 if info.short_chain else 0), (where, d)  # (slot 123 counts the short chains queued)
    why = "room" if i in h.room else info.refusal
    want, bit = {"room": ((0, 1, 0), UPD_FULL), "outside": ((0, 0, 1), UPD_OUTSIDE), "conflict": ((1, 0, 0), UPD_CONFLICT), "need_host": ((0, 0, 0), UPD_NEED_HOST)}[why]
    assert reasons == want and dst & bit, (where, why, reasons, hex(dst))
    return f"refused ({why}), host replay"


def run_history(m, h, steps, arm, observe=None):
    """the first cloud and every batch into m; with `observe` the state is checked after each and the paths are collected"""
    m.AddCloudToLocalMap([h.first])
    paths = []
    if observe:
        check_state(m, steps[0], observe, (h.name, "first cloud"))
    for i, (pts, codes) in enumerate(h.batches):
        info = steps[i + 1][0]
        before = {s: m.map_size(s) for s in PATH_SLOTS}
        rc, dst = m.DebugAddPoints(pts, codes)
        d = {s: m.map_size(s) - before[s] for s in PATH_SLOTS}
        where = (h.name, arm, observe, f"batch {i + 1}")
        assert rc == info.rc, (where, rc, info.rc)
        if arm == "device":
            paths.append(check_path(h, i, info, rc, dst, d, where))
        else:
            assert dst == U.NO_CHAIN and d[103] == 0, (where, hex(dst), d)
        if observe:
            check_state(m, steps[i + 1], observe, where)
            if info.outside:  # the map after FLS_ERR_RANGE, against the handle's own account of it
                U.check_image(image_of(m), U.decode_blob(blob_of(m))[1])
    return paths


@pytest.mark.parametrize("name,arm,observe", CASES)
def test_history(built, monkeypatch, name, arm, observe):
    h = U.history(name)
    steps, model = U.replay(name)
    a = make(monkeypatch, h.capacity, arm)
    paths = run_history(a, h, steps, arm, observe)
    info = [s[0] for s in steps[1:]]
    print(f"{name} [{arm}, {observe}]: " + "; ".join(f"batch {i + 1}: {p}, {f.n_evicted} evicted, {f.n_recreated} re-created"
                                                      for i, (p, f) in enumerate(zip(paths or ["host"] * len(info), info))))
    end = a.ExportMap()
    assert end.tobytes() == blob_of(a).tobytes() == steps[-1][1].tobytes()
    b = make(monkeypatch, h.capacity, arm)  # a second handle, the same history, never observed on the way
    run_history(b, h, steps, arm)
    assert blob_of(b).tobytes() == end.tobytes()
    a.close()
    b.close()


def test_argument_and_state_errors_on_live_handles(built, monkeypatch):
    """what tests/test_debug_ivox_update_abi.py cannot reach without a device: another kind and a code above 2 are FLS_ERR_INVALID; a handle without
    its first cloud, a localization-mode handle and a replica are FLS_ERR_STATE; none of them changes a map; an empty batch is FLS_OK and runs no chain"""
    h = U.history("lru")
    pts, codes = h.batches[0]
    ndt = reg.make_matcher("IncrementalNDT", dict(reg.YAML_NCLT_NDT))
    assert ndt.DebugAddPoints(pts, codes) == (_lib.FLS_ERR_INVALID, 0)
    ndt.close()
    m = make(monkeypatch)
    assert m.DebugAddPoints(pts, codes)[0] == _lib.FLS_ERR_STATE, "no map yet"
    m.AddCloudToLocalMap([h.first])
    want = blob_of(m).tobytes()
    bad = codes.copy()
    bad[-1] = 3
    assert m.DebugAddPoints(pts, bad)[0] == _lib.FLS_ERR_INVALID
    assert m.DebugAddPoints(np.zeros((0, 3), np.float32), np.zeros(0, np.uint8)) == (_lib.FLS_OK, U.NO_CHAIN)
    assert blob_of(m).tobytes() == want
    loc = make(monkeypatch, loc=True)
    loc.AddCloudToLocalMap([h.first])
    assert loc.DebugAddPoints(pts, codes)[0] == _lib.FLS_ERR_STATE
    n = m.MapImageBytes()
    d = DevMem(n)
    m.ExportMapImage(d.p.value, n, True)
    rep = make(monkeypatch)
    rep.ImportMapImage(d.p.value, n, True)
    d.free()
    assert rep.DebugAddPoints(pts, codes)[0] == _lib.FLS_ERR_STATE
    assert m.DebugAddPoints(pts, codes) == (_lib.FLS_OK, 0) and blob_of(m).tobytes() == U.replay("lru")[0][1][1].tobytes()
    for x in (m, loc, rep):
        x.close()
