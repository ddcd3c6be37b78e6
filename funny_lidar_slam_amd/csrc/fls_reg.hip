// fls_reg.hip -- libfls_reg.so: C ABI (include/fls_reg.h) over the gfx950 registration back-end.
// Single translation unit: device kernels (kernels_*.hpp) + host matchers (matcher*.hpp).
// Built by csrc/Makefile:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// There is no CPU fallback: without a gfx950 device fls_create fails with FLS_ERR_DEVICE.
#include <chrono>
#include "matcher_p2plane_ivox.hpp"
#include "matchers_kd.hpp"
#include "matcher_ndt.hpp"
#include "features_host.hpp"
#include "preprocess_host.hpp"
#include "loop_closure.hpp"
#include "replicas.hpp"
#include "keyframes.hpp"
#include "localmap.hpp"
#include "kernels_debug_linalg.hpp"
#include "kernels_debug_fit.hpp"
#include "../../include/fls_keyframes.h"
#include "../../include/fls_localmap.h"
#include "../../include/fls_batch.h"
#include "../../include/fls_batch_ivox.h"
#include "../../include/fls_debug_linalg.h"
#include "../../include/fls_debug_fit.h"
#include "../../include/fls_debug_ndt.h"
#include "../../include/fls_debug_loop.h"
#include "../../include/fls_debug_knn.h"
#include "../../include/fls_map_kd.h"
#include <new>

using namespace fls;

namespace {

int gfx950_device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) continue;
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

// test hooks of include/fls_debug_linalg.h: inputs up, one launch, outputs down: every array holds `w` doubles per system
struct DebugIn { const double* p; int w; };
struct DebugOut { double* p; int w; };
template <typename Launch>
fls_status debug_linalg_run(int device_id, int n, const std::vector<DebugIn>& in, const std::vector<DebugOut>& out, Launch&& launch) {
    for (const DebugIn& a : in) if (!a.p) return FLS_ERR_INVALID;
    for (const DebugOut& a : out) if (!a.p) return FLS_ERR_INVALID;
    if (n < 0) return FLS_ERR_INVALID;
    if (n == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        std::vector<DevBuf<double>> din(in.size()), dout(out.size());
        std::vector<const double*> pin(in.size());
        std::vector<double*> pout(out.size());
        for (size_t i = 0; i < in.size(); ++i) {
            din[i].reserve(size_t(n) * in[i].w);
            FLS_HIP(hipMemcpy(din[i].p, in[i].p, size_t(n) * in[i].w * sizeof(double), hipMemcpyHostToDevice));
            pin[i] = din[i].p;
        }
        for (size_t i = 0; i < out.size(); ++i) { dout[i].reserve(size_t(n) * out[i].w); pout[i] = dout[i].p; }
        launch(pin.data(), pout.data());
        FLS_HIP(hipGetLastError());
        for (size_t i = 0; i < out.size(); ++i) FLS_HIP(hipMemcpy(out[i].p, dout[i].p, size_t(n) * out[i].w * sizeof(double), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}
inline dim3 debug_linalg_lanes(int n) { return dim3(unsigned((n + kDebugLinalgBlock - 1) / kDebugLinalgBlock)); }

// one matcher per device, kept for the life of the process (stream, result block, device buffers: ~3 ms to set up, the reference's
// loop-closure thread calls Match once per candidate); calls on one device are serialised (run_mx).  Never destroyed: static
// destruction would run after the HIP runtime's own teardown.
fls_status loop_matcher_for(int device_id, LoopMatcher*& m) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return FLS_ERR_DEVICE;
    hipDeviceProp_t prop;
    FLS_HIP(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FLS_ERR_DEVICE;
    static std::mutex mx;
    static std::map<int, LoopMatcher*>* cache = new std::map<int, LoopMatcher*>();
    std::lock_guard<std::mutex> lk(mx);
    LoopMatcher*& slot = (*cache)[device_id];
    if (!slot) {
        std::unique_ptr<LoopMatcher> fresh(new LoopMatcher());
        fresh->init(device_id);
        slot = fresh.release();
    }
    m = slot;
    return FLS_OK;
}

// helpers of the test hooks of include/fls_debug_loop.h: the hook's body on the device's own LoopMatcher, under its run mutex (the ticket is NOT reset: see the header)
template <class F>
fls_status debug_loop_run(int device_id, F&& body) {
    return guarded([&]() -> fls_status {
        LoopMatcher* m = nullptr;
        const fls_status got = loop_matcher_for(device_id, m);
        if (got != FLS_OK) return got;
        std::lock_guard<std::mutex> run_lk(m->run_mx);
        m->read_env();
        FLS_HIP(hipSetDevice(m->device));
        return body(*m);
    });
}

// a cloud's cell grid as LoopMatcher::run builds it: on the device, else (or with host_grid) on the host
fls_status debug_loop_grid(LoopMatcher& m, CellGridImage& g, const LoopMatcher::DevCloud& dev, const std::vector<PtI>& c, float cell, bool by_id, bool host_grid) {
    if (!host_grid && m.builder.run(g, dev.x(), dev.y(), dev.z(), c.size(), cell, 1, by_id, m.stream)) return FLS_OK;
    return g.build(c, cell, m.stream, 1, by_id);
}

LoopMat4f debug_loop_mat(const float* T) { LoopMat4f r; for (int i = 0; i < 16; ++i) r.m[i] = T[i]; return r; }

constexpr float kDebugLoopCell = 1.5f;  // LoopMatcher::run's GICP cell

// helpers of the test hooks of include/fls_debug_knn.h: one search (map cloud, its cell grid, queries, the three output arrays of grid_knn_kernel<5>)
// with buffers of its own on the null stream; the outputs are filled with the byte 0x7b before the launch, so a row the kernel did not write shows
fls_status debug_knn_device(int device_id) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return FLS_ERR_DEVICE;
    hipDeviceProp_t prop;
    FLS_HIP(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FLS_ERR_DEVICE;
    FLS_HIP(hipSetDevice(device_id));
    return FLS_OK;
}
inline bool debug_knn_common_ok(const float* map, int nm, const float* query, int nq, int stride, float cell, int host_grid) {
    return map && query && nm >= 0 && nq >= 0 && stride >= 3 && cell > 0.f && std::isfinite(cell) && (host_grid == 0 || host_grid == 1);
}
struct DebugKnnSide {
    LoopMatcher::DevCloud map, query;
    CellGridImage grid;
    DeviceGridBuilder builder;
    DevBuf<float4> pts;
    DevBuf<unsigned char> cnt, flag;
    DevBuf<float> kth;
    int nq = 0;
    // the grid as KdLocalMap::rebuild makes it: on the device, else (or with host_grid) on the host
    fls_status prepare_grid(const float* m, int nm, const float* q, int n_query, int stride, float cell, int rings, bool host_grid) {
        const std::vector<PtI> mc = cloud_from(m, size_t(nm), stride), qc = cloud_from(q, size_t(n_query), stride);
        nq = n_query;
        map.upload(mc, nullptr);
        query.upload(qc, nullptr);
        if (!host_grid && builder.run(grid, map.x(), map.y(), map.z(), mc.size(), cell, rings, false, nullptr)) return FLS_OK;
        return grid.build(mc, cell, nullptr, rings, false);
    }
    void prepare_outputs() {
        pts.reserve(size_t(nq) * 5); cnt.reserve(size_t(nq)); flag.reserve(size_t(nq)); kth.reserve(size_t(nq));
        FLS_HIP(hipMemset(pts.p, 0x7b, size_t(nq) * 5 * sizeof(float4)));
        FLS_HIP(hipMemset(cnt.p, 0x7b, size_t(nq)));
        FLS_HIP(hipMemset(flag.p, 0x7b, size_t(nq)));
        FLS_HIP(hipMemset(kth.p, 0x7b, size_t(nq) * sizeof(float)));
    }
    GridKnnArgs args(float gate) { return GridKnnArgs{query.x(), query.y(), query.z(), nq, cell_dev(grid), gate, pts.p, cnt.p, kth.p, flag.p}; }
    void fetch(float* out_pts, uint8_t* out_cnt, float* out_kth, int32_t* out_has_window) {
        FLS_HIP(hipMemcpy(out_pts, pts.p, size_t(nq) * 5 * sizeof(float4), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(out_cnt, cnt.p, size_t(nq), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(out_kth, kth.p, size_t(nq) * sizeof(float), hipMemcpyDeviceToHost));
        *out_has_window = grid.have_window ? 1 : 0;
    }
};
inline void debug_knn_empty(int nq, float* out_pts, uint8_t* out_cnt, float* out_kth, int32_t* out_has_window) {
    const int32_t none = -1;
    for (size_t i = 0; i < size_t(nq) * 5; ++i) {
        out_pts[4 * i] = out_pts[4 * i + 1] = out_pts[4 * i + 2] = 0.f;
        std::memcpy(out_pts + 4 * i + 3, &none, sizeof(none));
    }
    for (int i = 0; i < nq; ++i) { out_cnt[i] = 0; out_kth[i] = INFINITY; }
    *out_has_window = 0;
}
inline Pose16 debug_knn_pose(const double* T16) { Pose16 T; std::memcpy(T.m, T16, sizeof(T.m)); return T; }

}  // namespace

extern "C" {

int fls_abi_version(void) { return FLS_ABI_VERSION; }
int fls_abi_revision(void) { return FLS_ABI_REVISION; }
int fls_device_count(void) { return gfx950_device_count(); }

const char* fls_status_string(int s) {
    switch (s) {
        case FLS_OK: return "ok (Match returned true)";
        case FLS_NOT_CONVERGED: return "not converged (Match returned false)";
        case FLS_SKIPPED: return "batch job not run";
        case FLS_ERR_INVALID: return "invalid argument or unset parameter";
        case FLS_ERR_DEVICE: return "HIP error or no gfx950 device";
        case FLS_ERR_RANGE: return "coordinate outside the voxel key range";
        case FLS_ERR_NOMEM: return "out of memory";
        case FLS_ERR_STATE: return "call order violated";
        default: return "unknown status";
    }
}

fls_status fls_create(fls_kind kind, const fls_params* params, int device_id, fls_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    if (!params) return FLS_ERR_INVALID;
    const fls_status pc = check_common(*params);
    if (pc != FLS_OK) return pc;
    return guarded([&]() -> fls_status {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return FLS_ERR_DEVICE;
        hipDeviceProp_t prop;
        FLS_HIP(hipGetDeviceProperties(&prop, device_id));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            std::fprintf(stderr, "[fls_reg] device %d is %s; this library is built for gfx950 only\n", device_id, prop.gcnArchName);
            return FLS_ERR_DEVICE;
        }
        std::unique_ptr<fls_matcher> m;
        fls_status rc = FLS_ERR_INVALID;
        switch (kind) {
            case FLS_P2PLANE_IVOX: { auto* q = new P2PlaneIvoxMatcher(); m.reset(q); q->kind = kind; q->p = *params; q->device = device_id; rc = q->init(); break; }
            case FLS_ICP_OPTIMIZED: { auto* q = new IcpMatcher(); m.reset(q); q->kind = kind; q->p = *params; q->device = device_id; rc = q->init(); break; }
            case FLS_INCREMENTAL_NDT: { auto* q = new NdtMatcher(); m.reset(q); q->kind = kind; q->p = *params; q->device = device_id; rc = q->init(); break; }
            case FLS_LOAM_FULL: { auto* q = new LoamFullMatcher(); m.reset(q); q->kind = kind; q->p = *params; q->device = device_id; rc = q->init(); break; }
            case FLS_P2PLANE_KDTREE: { auto* q = new P2PlaneKdMatcher(); m.reset(q); q->kind = kind; q->p = *params; q->device = device_id; rc = q->init(); break; }
            default: return FLS_ERR_INVALID;
        }
        if (rc != FLS_OK) return rc;
        *out = m.release();
        return FLS_OK;
    });
}

void fls_destroy(fls_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    h->lanes.clear();  // the batch lanes read this handle's map: they go first
    delete h;
}

fls_status fls_add_cloud_to_local_map(fls_handle h, const float* c0, size_t n0, const float* c1, size_t n1, int stride) {
    if (!h || (!c0 && n0) || stride < 3) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->add_cloud(c0, n0, c1, n1, stride);
    });
}

fls_status fls_scan_upload(fls_handle h, const float* s0, size_t n0, const float* s1, size_t n1, int stride) {
    if (!h || (!s0 && n0) || stride < 3) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        const fls_status rc = h->scan_upload(s0, n0, s1, n1, stride);
        FLS_HIP(hipStreamSynchronize(h->stream));
        return rc;
    });
}

fls_status fls_scan_upload_raw(fls_handle h, const float* s0, size_t n0, const float* s1, size_t n1, int stride) {
    if (!h || (!s0 && n0) || stride < 3) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        const fls_status rc = h->scan_upload_raw(s0, n0, s1, n1, stride);
        FLS_HIP(hipStreamSynchronize(h->stream));
        return rc;
    });
}

fls_status fls_match_resident(fls_handle h, double T[16], int update_map, fls_stats* stats) {
    if (!h || !T) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->match_resident(T, update_map, stats);
    });
}

fls_status fls_match(fls_handle h, const float* s0, size_t n0, const float* s1, size_t n1, int stride, double T[16], int update_map,
                     fls_stats* stats) {
    if (!h || !T || (!s0 && n0) || stride < 3) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        const fls_status rc = h->scan_upload_for_match(s0, n0, s1, n1, stride);
        if (rc != FLS_OK) return rc;
        return h->match_resident(T, update_map, stats);
    });
}

size_t fls_map_image_bytes(fls_handle h) {
    if (!h) return 0;
    size_t n = 0;
    guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); n = h->map_image_bytes(); return FLS_OK; });
    return n;
}
fls_status fls_map_image_export(fls_handle h, void* dst, size_t cap_bytes, int dst_on_device) {
    if (!h || !dst) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); return h->map_image_export(dst, cap_bytes, dst_on_device); });
}
fls_status fls_map_image_import(fls_handle h, const void* src, size_t n_bytes, int src_on_device) {
    if (!h || !src) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); return h->map_image_import(src, n_bytes, src_on_device); });
}

fls_status fls_match_batch(fls_handle h, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                           const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int lanes) {
    if (!h || stride < 3 || (n_jobs && (!src0 || !n0 || !T))) return FLS_ERR_INVALID;
    if ((src1 == nullptr) != (n1 == nullptr)) return FLS_ERR_INVALID;
    for (size_t j = 0; j < n_jobs; ++j)
        if (!src0[j] && n0[j]) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->match_batch(n_jobs, src0, n0, src1, n1, stride, T, stats, status, lanes);
    });
}

// ---- include/fls_batch.h ----
int fls_batch_revision(void) { return FLS_BATCH_REVISION; }

fls_status fls_match_batch_fused(fls_handle h, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                 const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int n_slots) {
    if (!h || stride < 3 || (n_jobs && (!src0 || !n0 || !T))) return FLS_ERR_INVALID;
    if ((src1 == nullptr) != (n1 == nullptr)) return FLS_ERR_INVALID;
    for (size_t j = 0; j < n_jobs; ++j)
        if (!src0[j] && n0[j]) return FLS_ERR_INVALID;
    if (n_jobs == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->match_batch_fused(n_jobs, src0, n0, src1, n1, stride, T, stats, status, n_slots);
    });
}

size_t fls_batch_stat(fls_handle h, int slot) { return (h && slot >= 0 && slot < 4) ? h->batch_counters[slot] : 0; }

// ---- include/fls_batch_ivox.h ----
int fls_batch_ivox_revision(void) { return FLS_BATCH_IVOX_REVISION; }

fls_status fls_match_batch_shared_ivox(fls_handle h, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                       const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int n_slots) {
    if (!h || stride < 3 || (n_jobs && (!src0 || !n0 || !T))) return FLS_ERR_INVALID;
    if ((src1 == nullptr) != (n1 == nullptr)) return FLS_ERR_INVALID;
    for (size_t j = 0; j < n_jobs; ++j)
        if (!src0[j] && n0[j]) return FLS_ERR_INVALID;
    if (n_jobs == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->match_batch_shared_ivox(n_jobs, src0, n0, src1, n1, stride, T, stats, status, n_slots);
    });
}

size_t fls_batch_ivox_stat(fls_handle h, int slot) { return (h && slot >= 0 && slot < 5) ? h->batch_ivox_counters[slot] : 0; }

size_t fls_map_export(fls_handle h, void* blob, size_t cap) {
    if (!h) return 0;
    size_t n = 0;
    (void)guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); n = h->map_export(blob, cap); return FLS_OK; });
    return n;
}

fls_status fls_map_import(fls_handle h, const void* blob, size_t n) {
    if (!h || !blob) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); return h->map_import(blob, n); });
}

// ---- include/fls_map_ivox.h: the blob of fls_map_export / fls_map_import for an FLS_P2PLANE_IVOX handle, packed and built on the device ----
unsigned fls_ivox_blob_revision(void) { return FLS_IVOX_BLOB_REVISION; }

size_t fls_ivox_map_bytes(fls_handle h) {
    if (!h) return 0;
    size_t n = 0;
    (void)guarded([&]() -> fls_status { n = h->ivox_blob_bytes(); return FLS_OK; });
    return n;
}

fls_status fls_ivox_map_export(fls_handle h, void* dst, size_t cap_bytes, int dst_on_device) {
    if (!h || !dst) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); return h->ivox_blob_export(dst, cap_bytes, dst_on_device); });
}

fls_status fls_ivox_map_import(fls_handle h, const void* src, size_t n_bytes, int src_on_device) {
    if (!h || !src) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); return h->ivox_blob_import(src, n_bytes, src_on_device); });
}

// ---- include/fls_map_ndt.h: the format fls_map_export / fls_map_image_export write for an FLS_INCREMENTAL_NDT handle ----
int fls_ndt_image_revision(void) { return FLS_NDT_IMAGE_REVISION; }

fls_status fls_replicas_create(fls_handle owner, const int* device_ids, int n_devices, fls_replicas_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    if (!owner || !device_ids || n_devices <= 0 || n_devices > 64) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FLS_ERR_DEVICE;
        for (int i = 0; i < n_devices; ++i)
            if (device_ids[i] < 0 || device_ids[i] >= n) return FLS_ERR_DEVICE;
        std::unique_ptr<fls_replicas> r(new fls_replicas());
        r->owner = owner;
        bool owner_used = false;
        for (int i = 0; i < n_devices; ++i) {
            r->devices.push_back(device_ids[i]);
            r->import_ms.push_back(0.0);
            if (device_ids[i] == owner->device && !owner_used) {
                owner_used = true;
                r->handles.push_back(owner);
                r->owned.push_back(0);
                continue;
            }
            fls_handle h = nullptr;
            const fls_status rc = fls_create(owner->kind, &owner->p, device_ids[i], &h);
            if (rc < 0) return rc;  // (the set's destructor releases what was created so far)
            r->handles.push_back(h);
            r->owned.push_back(1);
        }
        const fls_status rc = r->refresh();
        if (rc < 0) return rc;
        *out = r.release();
        return FLS_OK;
    });
}

fls_status fls_replicas_refresh(fls_replicas_handle r) {
    if (!r) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { return r->refresh(); });
}

fls_status fls_replicas_match_batch(fls_replicas_handle r, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                    const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int lanes) {
    if (!r || stride < 3 || (n_jobs && (!src0 || !n0 || !T))) return FLS_ERR_INVALID;
    if ((src1 == nullptr) != (n1 == nullptr)) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { return r->match_batch(n_jobs, src0, n0, src1, n1, stride, T, stats, status, lanes); });
}

// ---- include/fls_map_kd.h: the format fls_map_export / fls_map_image_export write for the kd-tree kinds, and the fused batch over a replica set ----
int fls_kd_image_revision(void) { return FLS_KD_IMAGE_REVISION; }

fls_status fls_replicas_match_batch_fused(fls_replicas_handle r, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                          const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int slots) {
    if (!r || stride < 3 || (n_jobs && (!src0 || !n0 || !T))) return FLS_ERR_INVALID;
    if ((src1 == nullptr) != (n1 == nullptr)) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { return r->match_batch(n_jobs, src0, n0, src1, n1, stride, T, stats, status, slots, true); });
}

int fls_replicas_import_ms(fls_replicas_handle r, double* ms, int cap) {
    if (!r) return 0;
    const int n = int(r->import_ms.size());
    for (int i = 0; i < std::min(n, cap); ++i)
        if (ms) ms[i] = r->import_ms[size_t(i)];
    return n;
}

void fls_replicas_destroy(fls_replicas_handle r) { delete r; }

fls_status fls_get_fitness_score(fls_handle h, float max_range, float* score) {
    if (!h || !score) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->fitness(max_range, score);
    });
}

int fls_get_iteration_log(fls_handle h, double* T_iters, int32_t* n_valid, double* sum_res, int cap) {
    if (!h || !h->h_state.p) return 0;
    if (guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); h->refresh_log(); return FLS_OK; }) != FLS_OK) return 0;
    const GnState& s = *h->h_state.p;
    const int n = std::min(cap, h->log_n);
    for (int i = 0; i < n; ++i) {
        if (T_iters) std::memcpy(T_iters + 16 * i, s.log_T[i], sizeof(double) * 16);
        if (n_valid) n_valid[i] = s.log_nv[i];
        if (sum_res) sum_res[i] = s.log_res[i];
    }
    return h->log_n;
}

int fls_get_correspondences(fls_handle h, int slot, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) {
    if (!h || !ids || !cnt || !valid) return -1;
    int n = -1;
    const fls_status rc = guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        n = h->correspondences(slot, ids, cnt, valid, cap);
        return FLS_OK;
    });
    return rc == FLS_OK ? n : -1;
}

size_t fls_map_size(fls_handle h, int slot) { return h ? h->map_size(slot) : 0; }

fls_status fls_set_profiling(fls_handle h, int enable) {
    if (!h) return FLS_ERR_INVALID;
    h->profiling = (enable & 1) != 0;       // accumulators are only reset by fls_get_kernel_time, so the flag can be
    h->count_traffic = (enable & 2) != 0;   // toggled per Match (e.g. to bracket every n-th step of a timed region)
    return FLS_OK;
}

fls_status fls_get_kernel_time(fls_handle h, double* ms_total, int64_t* launches, uint64_t* point_iters) {
    if (!h) return FLS_ERR_INVALID;
    const fls_status rc = guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); h->settle_events(); return FLS_OK; });
    if (rc != FLS_OK) return rc;
    if (ms_total) *ms_total = h->prof_ms;
    if (launches) *launches = h->prof_launches;
    if (point_iters) *point_iters = h->prof_point_iters;
    h->prof_ms = 0.0;
    h->prof_launches = 0;
    h->prof_point_iters = 0;
    return FLS_OK;
}

fls_status fls_get_debug_stamps(fls_handle h, int64_t out[16]) {
    if (!h || !out || !h->h_state.p) return FLS_ERR_INVALID;
    (void)guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); h->refresh_log(); return FLS_OK; });
    for (int i = 0; i < 16; ++i) out[i] = h->h_state.p->dbg[i];
    return FLS_OK;
}

fls_status fls_debug_fullpiv_qr6(int device_id, const double* H, const double* g, int n, double* x) {
    if (!H || !g || !x || n < 0) return FLS_ERR_INVALID;
    if (n == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevBuf<double> dH, dg, dx;
        dH.reserve(size_t(n) * 36); dg.reserve(size_t(n) * 6); dx.reserve(size_t(n) * 6);
        FLS_HIP(hipMemcpy(dH.p, H, size_t(n) * 36 * sizeof(double), hipMemcpyHostToDevice));
        FLS_HIP(hipMemcpy(dg.p, g, size_t(n) * 6 * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(debug_fullpiv_qr6_kernel, dim3(unsigned(n)), dim3(64), 0, nullptr, (const double*)dH.p, (const double*)dg.p, n, dx.p);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpy(x, dx.p, size_t(n) * 6 * sizeof(double), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

fls_status fls_debug_ldlt6(int device_id, const double* H, const double* g, int n, double* x, int32_t* ok) {
    if (!H || !g || !x || !ok || n < 0) return FLS_ERR_INVALID;
    if (n == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevBuf<double> dH, dg, dx;
        DevBuf<int> dok;
        dH.reserve(size_t(n) * 36); dg.reserve(size_t(n) * 6); dx.reserve(size_t(n) * 6); dok.reserve(size_t(n));
        FLS_HIP(hipMemcpy(dH.p, H, size_t(n) * 36 * sizeof(double), hipMemcpyHostToDevice));
        FLS_HIP(hipMemcpy(dg.p, g, size_t(n) * 6 * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(debug_ldlt6_kernel, dim3(unsigned(n)), dim3(64), 0, nullptr, (const double*)dH.p, (const double*)dg.p, n, dx.p, dok.p);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpy(x, dx.p, size_t(n) * 6 * sizeof(double), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(ok, dok.p, size_t(n) * sizeof(int), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

// ---- test hooks of the device linear-algebra primitives (include/fls_debug_linalg.h, kernels_debug_linalg.hpp) --------------------------
int fls_debug_linalg_revision(void) { return FLS_DEBUG_LINALG_REVISION; }

fls_status fls_debug_plane_fit_5x3(int device_id, const double* A, int n, double* x) {
    return debug_linalg_run(device_id, n, {{A, 15}}, {{x, 3}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_plane_fit_5x3_kernel, debug_linalg_lanes(n), dim3(kDebugLinalgBlock), 0, nullptr, in[0], n, out[0]);
    });
}

fls_status fls_debug_svd3(int device_id, const double* A, int n, double* S, double* V) {
    return debug_linalg_run(device_id, n, {{A, 9}}, {{S, 3}, {V, 9}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_svd3_kernel, debug_linalg_lanes(n), dim3(kDebugLinalgBlock), 0, nullptr, in[0], n, out[0], out[1]);
    });
}

fls_status fls_debug_lu6(int device_id, const double* H, const double* b, int n, double* det, double* inv, double* x) {
    return debug_linalg_run(device_id, n, {{H, 36}, {b, 6}}, {{det, 1}, {inv, 36}, {x, 6}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_lu6_kernel, dim3(unsigned(n)), dim3(64), 0, nullptr, in[0], in[1], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_so3(int device_id, const double* v, const double* R, int n, double* Rd, double* R_Rd, double* Rd_R) {
    return debug_linalg_run(device_id, n, {{v, 3}, {R, 9}}, {{Rd, 9}, {R_Rd, 9}, {Rd_R, 9}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_so3_kernel, debug_linalg_lanes(n), dim3(kDebugLinalgBlock), 0, nullptr, in[0], in[1], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_wave_sum(int device_id, const double* v, int n, double* total) {
    return debug_linalg_run(device_id, n, {{v, 64}}, {{total, 1}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_wave_sum_kernel, dim3(unsigned(n)), dim3(64), 0, nullptr, in[0], n, out[0]);
    });
}

// ---- test hooks of the stages of the fit launch (include/fls_debug_fit.h, kernels_debug_fit.hpp) ----------------------------------------
int fls_debug_fit_revision(void) { return FLS_DEBUG_FIT_REVISION; }

fls_status fls_debug_plane_residual(int device_id, const double* nn, const double* ps, const double* pt, const double* T, const double* gate, int n,
                                    double* valid, double* J, double* d) {
    return debug_linalg_run(device_id, n, {{nn, 15}, {ps, 3}, {pt, 3}, {T, 16}, {gate, 1}}, {{valid, 1}, {J, 6}, {d, 1}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_residual_kernel<false>, debug_linalg_lanes(n), dim3(kDebugFitBlock), 0, nullptr, in[0], in[1], in[2], in[3], in[4], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_line_residual(int device_id, const double* nn, const double* ps, const double* pt, const double* T, const double* gate, int n,
                                   double* valid, double* J, double* d) {
    return debug_linalg_run(device_id, n, {{nn, 15}, {ps, 3}, {pt, 3}, {T, 16}, {gate, 1}}, {{valid, 1}, {J, 6}, {d, 1}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_residual_kernel<true>, debug_linalg_lanes(n), dim3(kDebugFitBlock), 0, nullptr, in[0], in[1], in[2], in[3], in[4], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_icp_point_rows(int device_id, const double* T, const double* p, const double* m, int n, double* J, double* e, double* res) {
    return debug_linalg_run(device_id, n, {{T, 16}, {p, 3}, {m, 3}}, {{J, 18}, {e, 3}, {res, 1}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_icp_point_rows_kernel, debug_linalg_lanes(n), dim3(kDebugFitBlock), 0, nullptr, in[0], in[1], in[2], n, out[0], out[1], out[2]);
    });
}

fls_status fls_debug_rank1_mfma(int device_id, const double* contrib, const double* J, const double* r, int n, double* row) {
    return debug_linalg_run(device_id, n, {{contrib, 64}, {J, 64 * 6}, {r, 64}}, {{row, 32}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_rank1_kernel<0>, dim3(unsigned((n + 3) / 4)), dim3(256), 0, nullptr, in[0], in[1], in[2], n, out[0]);
    });
}

fls_status fls_debug_rank1_dpp(int device_id, const double* contrib, const double* J, const double* r, int n, double* row) {
    return debug_linalg_run(device_id, n, {{contrib, 64}, {J, 64 * 6}, {r, 64}}, {{row, 32}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_rank1_kernel<1>, dim3(unsigned((n + 3) / 4)), dim3(256), 0, nullptr, in[0], in[1], in[2], n, out[0]);
    });
}

fls_status fls_debug_rank1x3_mfma(int device_id, const double* contrib, const double* J, const double* e, int n, double* row) {
    return debug_linalg_run(device_id, n, {{contrib, 64}, {J, 64 * 18}, {e, 64 * 3}}, {{row, 32}}, [&](const double* const* in, double* const* out) {
        hipLaunchKernelGGL(debug_rank1_kernel<2>, dim3(unsigned((n + 3) / 4)), dim3(256), 0, nullptr, in[0], in[1], in[2], n, out[0]);
    });
}

fls_status fls_debug_reduce_partials(int device_id, int variant, const double* rows, int nrows, double* tot) {
    if (!rows || !tot || nrows < 0 || variant < 0 || variant > 3) return FLS_ERR_INVALID;
    if (nrows == 0) return FLS_OK;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        // one trip of NaN rows behind the caller's: a load past nrows shows in the totals instead of leaving the allocation
        const size_t pad = size_t(32) * 32;
        std::vector<double> h((size_t(nrows) + pad) * kPartialStride, std::numeric_limits<double>::quiet_NaN());
        std::memcpy(h.data(), rows, size_t(nrows) * kPartialStride * sizeof(double));
        DevBuf<double> drows, dtot;
        drows.reserve(h.size()); dtot.reserve(32);
        FLS_HIP(hipMemcpy(drows.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        const double* r = drows.p;
        if (variant == 0) hipLaunchKernelGGL((debug_reduce_partials_kernel<256, true, 32, LuTailSmem>), dim3(1), dim3(256), 0, nullptr, r, nrows, dtot.p);
        else if (variant == 1) hipLaunchKernelGGL((debug_reduce_partials_kernel<512, true, 16, LoamTailSmem>), dim3(1), dim3(512), 0, nullptr, r, nrows, dtot.p);
        else if (variant == 2) hipLaunchKernelGGL((debug_reduce_partials_kernel<512, true, 32, LuTailSmem>), dim3(1), dim3(512), 0, nullptr, r, nrows, dtot.p);
        else hipLaunchKernelGGL((debug_reduce_partials_kernel<1024, false, 16, LoamTailSmem>), dim3(1), dim3(1024), 0, nullptr, r, nrows, dtot.p);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpy(tot, dtot.p, 32 * sizeof(double), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

fls_status fls_debug_fanin(int device_id, int nblocks, int shards, double* tot, uint32_t* last, uint32_t* ticket) {
    static_assert(FLS_DEBUG_TICKET_WORDS == kTicketWords && kPartialStride == 32, "fls_debug_fit.h states the layout");
    if (!tot || !last || !ticket || nblocks < 1 || nblocks > 65535 || shards < 1) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevBuf<double> dpart, dtot;
        DevBuf<unsigned> dticket, dlast;
        const size_t pad = size_t(32) * 8;  // (NaN rows behind the last one, as in fls_debug_reduce_partials)
        std::vector<double> h((size_t(nblocks) + pad) * kPartialStride, std::numeric_limits<double>::quiet_NaN());
        std::fill(h.begin(), h.begin() + size_t(nblocks) * kPartialStride, 0.0);
        dpart.reserve(h.size()); dtot.reserve(64); dticket.reserve(kTicketWords); dlast.reserve(2);
        FLS_HIP(hipMemcpy(dpart.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        const std::vector<double> canary(64, 7.0);
        FLS_HIP(hipMemcpy(dtot.p, canary.data(), 64 * sizeof(double), hipMemcpyHostToDevice));
        FLS_HIP(hipMemset(dticket.p, 0, kTicketWords * sizeof(unsigned)));
        FLS_HIP(hipMemset(dlast.p, 0, 2 * sizeof(unsigned)));
        for (int k = 0; k < 2; ++k) {
            hipLaunchKernelGGL(debug_fanin_kernel, dim3(unsigned(nblocks)), dim3(256), 0, nullptr, dpart.p, dticket.p, shards, double(k + 1), 1000.0 * k, dlast.p + k,
                               dtot.p + 32 * k);
            FLS_HIP(hipGetLastError());
        }
        FLS_HIP(hipMemcpy(tot, dtot.p, 64 * sizeof(double), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(last, dlast.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(ticket, dticket.p, kTicketWords * sizeof(unsigned), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

// ---- test read-out of the NDT voxel map (include/fls_debug_ndt.h) ----------------------------------------------------------------------
int fls_debug_ndt_revision(void) { return FLS_DEBUG_NDT_REVISION; }

fls_status fls_debug_ndt_voxels(fls_handle h, size_t cap, int32_t* keys, int32_t* vid, int32_t* num_points, uint8_t* estimated, uint8_t* pending,
                                double* mu, double* sigma, double* info, size_t* n) {
    if (!h || !n || h->kind != FLS_INCREMENTAL_NDT) return FLS_ERR_INVALID;
    if (cap && (!keys || !vid || !num_points || !estimated || !pending || !mu || !sigma || !info)) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        NdtMatcher& m = *static_cast<NdtMatcher*>(h);
        if (m.device_mode) FLS_HIP(hipSetDevice(h->device));
        *n = m.dump_voxels(cap, NdtMatcher::VoxelDump{keys, vid, num_points, estimated, pending, mu, sigma, info});
        return cap < *n ? FLS_ERR_NOMEM : FLS_OK;
    });
}

fls_status fls_debug_last_system(fls_handle h, double* H36, double* g6) {
    if (!h || !H36 || !g6) return FLS_ERR_INVALID;
    if (!h->d_state.p) return FLS_ERR_STATE;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        FLS_HIP(hipStreamSynchronize(h->stream));
        FLS_HIP(hipMemcpy(H36, reinterpret_cast<const char*>(h->d_state.p) + offsetof(GnState, H), 36 * sizeof(double), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(g6, reinterpret_cast<const char*>(h->d_state.p) + offsetof(GnState, g), 6 * sizeof(double), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

fls_status fls_debug_voxel_grid(int device_id, const float* pts, size_t n, int stride, float leaf, float* out, size_t cap, size_t* n_out) {
    if (!pts || !n_out || stride < 3 || !(leaf > 0.f) || (cap && !out)) return FLS_ERR_INVALID;
    *n_out = 0;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevScan raw;
        DeviceVoxelGrid vg;
        raw.upload_raw(pts, n, stride, nullptr, true);
        if (n == 0 || !vg.run(raw.x.p, raw.y.p, raw.z.p, raw.xyz.p + 3 * n, n, leaf, nullptr)) return FLS_ERR_STATE;
        *n_out = vg.n_out;
        if (vg.n_out > cap) return FLS_ERR_INVALID;
        std::vector<float> tmp;
        const std::vector<PtI> c = vg.download(nullptr, tmp);
        std::memcpy(out, c.data(), c.size() * sizeof(PtI));
        return FLS_OK;
    });
}

fls_status fls_debug_voxel_grid_timed(int device_id, const float* pts, size_t n, int stride, float leaf, int reps, double* ms, size_t* n_out) {
    if (!pts || !n_out || !ms || reps <= 0 || stride < 3 || !(leaf > 0.f)) return FLS_ERR_INVALID;
    *n_out = 0;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevScan raw;
        DeviceVoxelGrid vg;  // one filter object for all repetitions: the buffers are allocated by the first one, as in a matcher
        raw.upload_raw(pts, n, stride, nullptr, true);
        FLS_HIP(hipDeviceSynchronize());
        for (int r = 0; r < reps; ++r) {
            const auto t0 = std::chrono::steady_clock::now();
            const bool ok = n != 0 && vg.run(raw.x.p, raw.y.p, raw.z.p, raw.xyz.p + 3 * n, n, leaf, nullptr);
            FLS_HIP(hipStreamSynchronize(nullptr));
            ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (!ok) return FLS_ERR_STATE;
        }
        *n_out = vg.n_out;
        return FLS_OK;
    });
}

fls_status fls_debug_exact_sort(int device_id, uint32_t* key, uint32_t* val, size_t n, int on_host) {
    if ((!key || !val) && n) return FLS_ERR_INVALID;
    if (on_host != 0 && on_host != 1 && on_host != 2) return FLS_ERR_INVALID;
    if (on_host == 1)
        return guarded([&]() -> fls_status {  // (an allocation failure must not cross the C ABI: ADVICE r4)
            std::vector<VoxelLeafRec> r(n);
            for (size_t i = 0; i < n; ++i) r[i] = VoxelLeafRec{key[i], val[i]};
            std::sort(r.begin(), r.end());  // operator< compares idx only: libstdc++'s introsort decides the order of equal keys
            for (size_t i = 0; i < n; ++i) { key[i] = r[i].idx; val[i] = r[i].pt; }
            return FLS_OK;
        });
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        if (n == 0) return FLS_OK;
        DevBuf<unsigned> dk, dv;
        dk.reserve(n); dv.reserve(n);
        FLS_HIP(hipMemcpy(dk.p, key, n * sizeof(unsigned), hipMemcpyHostToDevice));
        FLS_HIP(hipMemcpy(dv.p, val, n * sizeof(unsigned), hipMemcpyHostToDevice));
        DeviceExactSort es;  // (on_host 0 and 2: the same launch sequence, the one the VoxelGrid queues)
        if (!es.run_sync(dk.p, dv.p, n)) return FLS_ERR_STATE;
        FLS_HIP(hipMemcpy(key, dk.p, n * sizeof(unsigned), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(val, dv.p, n * sizeof(unsigned), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

extern "C" int fls_debug_exact_sort_marks(unsigned* out, int n) {  // diagnostics only (declared in fls_reg.h): progress stamps of the sort in flight
    if (!out || n <= 0) return -1;
    EsMailbox* m = es_debug_mailbox().load(std::memory_order_acquire);
    if (!m) return -1;
    for (int i = 0; i < n && i < 12; ++i) out[i] = __atomic_load_n(&m->mark[i], __ATOMIC_RELAXED);
    return 0;
}

fls_status fls_voxel_grid_cloud(int device_id, fls_voxelgrid_mode mode, const float* pts, size_t n, int stride, float leaf, float* out, size_t cap,
                                size_t* n_out) {
    if (mode == FLS_VOXELGRID_DEVICE) return fls_debug_voxel_grid(device_id, pts, n, stride, leaf, out, cap, n_out);
    if (mode != FLS_VOXELGRID_EXACT || (!pts && n) || !n_out || stride < 3 || !(leaf > 0.f) || (cap && !out)) return FLS_ERR_INVALID;
    *n_out = 0;
    return guarded([&]() -> fls_status {
        const std::vector<PtI> c = voxel_grid_strided(pts, n, stride, leaf);  // host_maps.hpp: the exact filter (pooled introsort order)
        *n_out = c.size();
        if (c.size() > cap) return FLS_ERR_INVALID;
        if (!c.empty()) std::memcpy(out, c.data(), c.size() * sizeof(PtI));
        return FLS_OK;
    });
}

fls_status fls_loop_match(int device_id, const float* source, size_t n_source, const float* target, size_t n_target, int stride, double T[16], float* fitness,
                          fls_loop_stats* stats) {
    if (!T || !fitness || stride < 3 || (!source && n_source) || (!target && n_target)) return FLS_ERR_INVALID;
    *fitness = std::numeric_limits<float>::max();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return guarded([&]() -> fls_status {
        const bool timing = host_timing_enabled();
        const auto t0 = std::chrono::steady_clock::now();
        LoopMatcher* m = nullptr;
        const fls_status got = loop_matcher_for(device_id, m);
        if (got != FLS_OK) return got;
        std::lock_guard<std::mutex> run_lk(m->run_mx);  // (devices run side by side, calls on one device one after the other)
        if (timing) std::fprintf(stderr, "[fls loop] ms: matcher set-up %.2f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        const fls_status rc = m->run(cloud_from(source, n_source, stride), cloud_from(target, n_target, stride), T, fitness);
        if (stats) *stats = m->st;
        return rc;
    });
}

// ---- test hooks of the stages of the loop-closure matcher (include/fls_debug_loop.h) ------------------------------------------------------
int fls_debug_loop_revision(void) { return FLS_DEBUG_LOOP_REVISION; }

fls_status fls_debug_loop_ndt(int device_id, const float* src, int ns, const float* tgt, int nt, int stride, float resolution, const double* p,
                              int want_hessian, double* score, double* grad, double* hess, int64_t* pairs, int32_t* leaves, int32_t* sparse) {
    if (!src || !tgt || !p || !score || !grad || !hess || !pairs || !leaves || !sparse || ns < 0 || nt < 0 || stride < 3 || !(resolution > 0.f) ||
        !std::isfinite(resolution))
        return FLS_ERR_INVALID;
    auto zero = [&] {
        *score = 0.0; *pairs = 0; *leaves = 0; *sparse = 0;
        for (int i = 0; i < 6; ++i) grad[i] = 0.0;
        if (want_hessian) for (int i = 0; i < 36; ++i) hess[i] = 0.0;
    };
    if (ns == 0 || nt == 0) { zero(); return FLS_OK; }
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        const std::vector<PtI> s = cloud_from(src, size_t(ns), stride), t = cloud_from(tgt, size_t(nt), stride);
        zero();
        if (!m.build_target(t, resolution, m.leaves)) return FLS_OK;
        *leaves = int32_t(m.leaves.rows);
        *sparse = m.leaves.sparse ? 1 : 0;
        LoopMatcher::NdtRun run;
        run.resolution = resolution;
        const double c1 = 10.0 * (1.0 - run.outlier_ratio), c2 = run.outlier_ratio / std::pow(double(resolution), 3), d3 = -std::log(c2);  // (ndt_align)
        run.pose.gauss_d1 = -std::log(c1 + c2) - d3;
        run.pose.gauss_d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / run.pose.gauss_d1);
        m.src_dev.upload(s, m.stream);
        run.src = &m.src_dev;
        run.tl = &m.leaves;
        *score = m.ndt_eval(run, LoopMatcher::pose_xyz(p), p, want_hessian != 0, grad, hess);
        *pairs = int64_t(m.mail_host->v[want_hessian ? 43 : 7]);
        return FLS_OK;
    });
}

fls_status fls_debug_loop_gicp_cov(int device_id, const float* cloud, int n, int stride, float cell, double epsilon, int host_grid, double* cov) {
    if (!cloud || !cov || n < 20 || stride < 3 || !(cell > 0.f) || !std::isfinite(cell) || !(epsilon > 0.0) || (host_grid != 0 && host_grid != 1)) return FLS_ERR_INVALID;
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        const std::vector<PtI> c = cloud_from(cloud, size_t(n), stride);
        m.src_own.upload(c, m.stream);
        const fls_status rc = debug_loop_grid(m, m.src_grid, m.src_own, c, cell, false, host_grid != 0);
        if (rc != FLS_OK) return rc;
        m.g.cov_src.reserve(size_t(n) * 9);
        hipLaunchKernelGGL(gicp_cov_kernel, dim3(unsigned((size_t(n) + kCovWaves - 1) / kCovWaves)), dim3(64 * kCovWaves), 0, m.stream, m.src_own.x(), m.src_own.y(), m.src_own.z(), n,
                           cell_dev(m.src_grid), epsilon, m.g.cov_src.p);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpyAsync(cov, m.g.cov_src.p, size_t(n) * 9 * sizeof(double), hipMemcpyDeviceToHost, m.stream));
        FLS_HIP(hipStreamSynchronize(m.stream));
        return FLS_OK;
    });
}

fls_status fls_debug_loop_gicp_corr(int device_id, const float* moved, int ns, const float* tgt, int nt, int stride, const float* T, const double* R,
                                    const double* cov_src, const double* cov_tgt, double corr_dist, int host_grid, int32_t* corr, double* mahal) {
    if (!moved || !tgt || !T || !R || !cov_src || !cov_tgt || !corr || !mahal || ns < 0 || nt < 0 || stride < 3 || !(corr_dist > 0.0) || !std::isfinite(corr_dist) ||
        (host_grid != 0 && host_grid != 1))
        return FLS_ERR_INVALID;
    if (ns == 0) return FLS_OK;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (nt == 0) {
        for (int i = 0; i < ns; ++i) corr[i] = -1;
        std::fill(mahal, mahal + size_t(ns) * 9, nan);
        return FLS_OK;
    }
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        const std::vector<PtI> s = cloud_from(moved, size_t(ns), stride), t = cloud_from(tgt, size_t(nt), stride);
        m.g.moved.upload(s, m.stream);
        m.tgt_dev.upload(t, m.stream);
        const fls_status rc = debug_loop_grid(m, m.g.tgt_grid, m.tgt_dev, t, kDebugLoopCell, true, host_grid != 0);
        if (rc != FLS_OK) return rc;
        m.g.cov_src.reserve(size_t(ns) * 9); m.g.cov_tgt.reserve(size_t(nt) * 9); m.g.mahal.reserve(size_t(ns) * 9); m.g.corr.reserve(size_t(ns));
        std::fill(mahal, mahal + size_t(ns) * 9, nan);
        FLS_HIP(hipMemcpyAsync(m.g.cov_src.p, cov_src, size_t(ns) * 9 * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipMemcpyAsync(m.g.cov_tgt.p, cov_tgt, size_t(nt) * 9 * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipMemcpyAsync(m.g.mahal.p, mahal, size_t(ns) * 9 * sizeof(double), hipMemcpyHostToDevice, m.stream));
        GicpRot rot;
        for (int i = 0; i < 9; ++i) rot.R[i] = R[i];
        const double dist_threshold = corr_dist * corr_dist;
        hipLaunchKernelGGL(gicp_corr_kernel, dim3(unsigned((ns + 63) / 64)), dim3(64), 0, m.stream, m.g.moved.x(), m.g.moved.y(), m.g.moved.z(), ns, debug_loop_mat(T),
                           cell_dev(m.g.tgt_grid), float(dist_threshold), dist_threshold, rot, (const double*)m.g.cov_src.p, (const double*)m.g.cov_tgt.p, m.g.corr.p, m.g.mahal.p);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpyAsync(corr, m.g.corr.p, size_t(ns) * sizeof(int), hipMemcpyDeviceToHost, m.stream));
        FLS_HIP(hipMemcpyAsync(mahal, m.g.mahal.p, size_t(ns) * 9 * sizeof(double), hipMemcpyDeviceToHost, m.stream));
        FLS_HIP(hipStreamSynchronize(m.stream));
        return FLS_OK;
    });
}

fls_status fls_debug_loop_gicp_fdf(int device_id, const float* moved, int ns, const float* tgt, int nt, int stride, const double* x, const int32_t* corr,
                                   const double* mahal, int want_grad, double* v) {
    if (!moved || !tgt || !x || !corr || !mahal || !v || ns < 0 || nt < 0 || stride < 3) return FLS_ERR_INVALID;
    for (int i = 0; i < ns; ++i) if (corr[i] < -1 || corr[i] >= nt) return FLS_ERR_INVALID;  // (the kernel indexes the target with it)
    const int nv = want_grad ? 14 : 2;
    if (ns == 0) { for (int i = 0; i < nv; ++i) v[i] = 0.0; return FLS_OK; }
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        const std::vector<PtI> s = cloud_from(moved, size_t(ns), stride);
        m.g.moved.upload(s, m.stream);
        std::vector<Pt4> by_id(size_t(std::max(nt, 1)), Pt4{0.f, 0.f, 0.f, 0});
        for (int i = 0; i < nt; ++i) by_id[size_t(i)] = Pt4{tgt[size_t(i) * stride], tgt[size_t(i) * stride + 1], tgt[size_t(i) * stride + 2], i};
        m.g.tgt_grid.d_by_id.reserve(by_id.size());
        m.g.corr.reserve(size_t(ns)); m.g.mahal.reserve(size_t(ns) * 9);
        FLS_HIP(hipMemcpyAsync(m.g.tgt_grid.d_by_id.p, by_id.data(), by_id.size() * sizeof(Pt4), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipMemcpyAsync(m.g.corr.p, corr, size_t(ns) * sizeof(int), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipMemcpyAsync(m.g.mahal.p, mahal, size_t(ns) * 9 * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipStreamSynchronize(m.stream));  // (by_id is a local)
        m.g.n_src = size_t(ns); m.g.n_tgt = size_t(nt);
        double f, grad[6];
        m.gicp_fdf(m.g, x, &f, want_grad ? grad : nullptr);
        for (int i = 0; i < nv; ++i) v[i] = m.mail_host->v[i];
        return FLS_OK;
    });
}

fls_status fls_debug_loop_fitness(int device_id, const float* src, int ns, const float* tgt, int nt, int stride, const float* T, int host_grid,
                                  double* sum_d2, int64_t* count) {
    if (!src || !tgt || !T || !sum_d2 || !count || ns < 0 || nt < 0 || stride < 3 || (host_grid != 0 && host_grid != 1)) return FLS_ERR_INVALID;
    if (ns == 0 || nt == 0) { *sum_d2 = 0.0; *count = 0; return FLS_OK; }
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        const std::vector<PtI> s = cloud_from(src, size_t(ns), stride), t = cloud_from(tgt, size_t(nt), stride);
        m.src_own.upload(s, m.stream);
        m.tgt_dev.upload(t, m.stream);
        const fls_status rc = debug_loop_grid(m, m.g.tgt_grid, m.tgt_dev, t, kDebugLoopCell, true, host_grid != 0);
        if (rc != FLS_OK) return rc;
        const LoopMat4f fin = debug_loop_mat(T);
        const CellGridDev cg_tgt = cell_dev(m.g.tgt_grid);
        const int nb = (ns + kLoopBlock - 1) / kLoopBlock;
        const double* v = m.reduce(nb, [&](const LoopOut rows) {
            hipLaunchKernelGGL(loop_fitness_kernel, dim3(unsigned(nb)), dim3(kLoopBlock), 0, m.stream, m.src_own.x(), m.src_own.y(), m.src_own.z(), ns, fin, cg_tgt, rows);
        });
        *sum_d2 = v[0];
        *count = int64_t(v[1]);
        FLS_HIP(hipStreamSynchronize(m.stream));
        return FLS_OK;
    });
}

// ---- test hooks of the cooperative grid k-NN kernels (include/fls_debug_knn.h) ----------------------------------------------------------
int fls_debug_knn_revision(void) { return FLS_DEBUG_KNN_REVISION; }

fls_status fls_debug_grid_knn5(int device_id, const float* map, int nm, const float* query, int nq, int stride, float cell, int rings, float gate,
                               const double* T16, int host_grid, float* out_pts, uint8_t* out_cnt, float* out_kth, int32_t* out_has_window) {
    if (!debug_knn_common_ok(map, nm, query, nq, stride, cell, host_grid) || !T16 || !out_pts || !out_cnt || !out_kth || !out_has_window || (rings != 1 && rings != 2) ||
        gate != gate)
        return FLS_ERR_INVALID;
    if (nm == 0 || nq == 0) { debug_knn_empty(nq, out_pts, out_cnt, out_kth, out_has_window); return FLS_OK; }
    return guarded([&]() -> fls_status {
        fls_status rc = debug_knn_device(device_id);
        if (rc != FLS_OK) return rc;
        DebugKnnSide s;
        rc = s.prepare_grid(map, nm, query, nq, stride, cell, rings, host_grid != 0);
        if (rc != FLS_OK) return rc;
        s.prepare_outputs();
        DevBuf<GnState> st;
        st.reserve(1);
        FLS_HIP(hipMemset(st.p, 0, sizeof(GnState)));
        const GridKnnArgs a = s.args(gate);
        const dim3 knn_grid_dim(knn_grid_blocks(size_t(nq)));
        const Pose16 T0 = debug_knn_pose(T16);
        if (std::isinf(gate))  // (FeatureDev::launch)
            hipLaunchKernelGGL((grid_knn_kernel<5, false, true>), knn_grid_dim, dim3(256), 0, nullptr, a.sx, a.sy, a.sz, a.n, (const GnState*)st.p, 1, T0, a.cg, gate, a.nn_pts,
                               a.nn_cnt, a.kth_d2, a.flag_to_clear);
        else
            hipLaunchKernelGGL((grid_knn_kernel<5, false>), knn_grid_dim, dim3(256), 0, nullptr, a.sx, a.sy, a.sz, a.n, (const GnState*)st.p, 1, T0, a.cg, gate, a.nn_pts,
                               a.nn_cnt, a.kth_d2, a.flag_to_clear);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipDeviceSynchronize());
        s.fetch(out_pts, out_cnt, out_kth, out_has_window);
        return FLS_OK;
    });
}

fls_status fls_debug_grid_knn5_dual(int device_id, const float* map_a, int nm_a, const float* query_a, int nq_a, float cell_a, int rings_a, float gate_a,
                                    const float* map_b, int nm_b, const float* query_b, int nq_b, float cell_b, int rings_b, float gate_b, int stride,
                                    const double* T16, int host_grid, float* out_pts_a, uint8_t* out_cnt_a, float* out_kth_a, int32_t* out_has_window_a,
                                    float* out_pts_b, uint8_t* out_cnt_b, float* out_kth_b, int32_t* out_has_window_b) {
    if (!debug_knn_common_ok(map_a, nm_a, query_a, nq_a, stride, cell_a, host_grid) || !debug_knn_common_ok(map_b, nm_b, query_b, nq_b, stride, cell_b, host_grid) || !T16 ||
        !out_pts_a || !out_cnt_a || !out_kth_a || !out_has_window_a || !out_pts_b || !out_cnt_b || !out_kth_b || !out_has_window_b || (rings_a != 1 && rings_a != 2) ||
        (rings_b != 1 && rings_b != 2) || !std::isfinite(gate_a) || !std::isfinite(gate_b) || nm_a == 0 || nq_a == 0 || nm_b == 0 || nq_b == 0)
        return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        fls_status rc = debug_knn_device(device_id);
        if (rc != FLS_OK) return rc;
        DebugKnnSide sa, sb;
        rc = sa.prepare_grid(map_a, nm_a, query_a, nq_a, stride, cell_a, rings_a, host_grid != 0);
        if (rc != FLS_OK) return rc;
        rc = sb.prepare_grid(map_b, nm_b, query_b, nq_b, stride, cell_b, rings_b, host_grid != 0);
        if (rc != FLS_OK) return rc;
        sa.prepare_outputs();
        sb.prepare_outputs();
        DevBuf<GnState> st;
        st.reserve(1);
        FLS_HIP(hipMemset(st.p, 0, sizeof(GnState)));
        const int ka = int(knn_grid_blocks(size_t(nq_a))), kb = int(knn_grid_blocks(size_t(nq_b)));  // (LoamFullMatcher::match_resident)
        hipLaunchKernelGGL((grid_knn_dual_kernel<5, false>), dim3(unsigned(ka + kb)), dim3(256), 0, nullptr, (const GnState*)st.p, 1, debug_knn_pose(T16), sa.args(gate_a),
                           sb.args(gate_b), ka);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipDeviceSynchronize());
        sa.fetch(out_pts_a, out_cnt_a, out_kth_a, out_has_window_a);
        sb.fetch(out_pts_b, out_cnt_b, out_kth_b, out_has_window_b);
        return FLS_OK;
    });
}

fls_status fls_debug_icp_knn1(int device_id, const float* map, int nm, const float* query, int nq, int stride, float cell, double max_corr_sq,
                              const double* T16, int host_grid, int32_t* out_id, uint8_t* out_eff, int32_t* out_has_window) {
    if (!debug_knn_common_ok(map, nm, query, nq, stride, cell, host_grid) || !T16 || !out_id || !out_eff || !out_has_window || !(max_corr_sq > 0.0) ||
        !std::isfinite(max_corr_sq))
        return FLS_ERR_INVALID;
    if (nm == 0 || nq == 0) {
        for (int i = 0; i < nq; ++i) { out_id[i] = -1; out_eff[i] = 0; }
        *out_has_window = 0;
        return FLS_OK;
    }
    return guarded([&]() -> fls_status {
        fls_status rc = debug_knn_device(device_id);
        if (rc != FLS_OK) return rc;
        DebugKnnSide s;
        rc = s.prepare_grid(map, nm, query, nq, stride, cell, 1, host_grid != 0);
        if (rc != FLS_OK) return rc;
        const unsigned rows = knn_grid_blocks(size_t(nq));
        DevBuf<GnState> st;
        DevBuf<int> nn_id;
        DevBuf<unsigned char> eff;
        DevBuf<double> partials;
        st.reserve(1); nn_id.reserve(size_t(nq)); eff.reserve(size_t(nq)); partials.reserve(size_t(rows) * kPartialStride);
        FLS_HIP(hipMemset(st.p, 0, sizeof(GnState)));
        FLS_HIP(hipMemset(nn_id.p, 0x7b, size_t(nq) * sizeof(int)));
        FLS_HIP(hipMemset(eff.p, 0x7b, size_t(nq)));
        const LuTailArgs tail{0, 0.0, 0.0, 0, nullptr, 0u};
        // (IcpMatcher::match_launch: gate = float(point_search_thres), max_corr = point_search_thres; no ticket: the tail does not run)
        hipLaunchKernelGGL(icp_knn_fit_kernel, dim3(rows), dim3(256), 0, nullptr, s.query.x(), s.query.y(), s.query.z(), nq, st.p, 1, debug_knn_pose(T16), cell_dev(s.grid),
                           float(max_corr_sq), max_corr_sq, nn_id.p, eff.p, partials.p, (unsigned*)nullptr, kTicketShards, tail);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipDeviceSynchronize());
        FLS_HIP(hipMemcpy(out_id, nn_id.p, size_t(nq) * sizeof(int), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(out_eff, eff.p, size_t(nq), hipMemcpyDeviceToHost));
        *out_has_window = s.grid.have_window ? 1 : 0;
        return FLS_OK;
    });
}

fls_status fls_get_traffic_counters(fls_handle h, uint64_t* probes, uint64_t* hit_voxels, uint64_t* cand_points) {
    if (!h) return FLS_ERR_INVALID;
    if (probes) *probes = h->last_tc.probes;
    if (hit_voxels) *hit_voxels = h->last_tc.hits;
    if (cand_points) *cand_points = h->last_tc.cand;
    return FLS_OK;
}

// ---- LOAM feature front-end (include/fls_features.h) ------------------------------------------------------------
fls_status fls_features_create(const fls_feature_params* params, int device_id, fls_features_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    if (!params) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return FLS_ERR_DEVICE;
        hipDeviceProp_t prop;
        FLS_HIP(hipGetDeviceProperties(&prop, device_id));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FLS_ERR_DEVICE;
        std::unique_ptr<fls_features> f(new fls_features());
        f->p = *params;
        f->device = device_id;
        const fls_status rc = f->init();
        if (rc != FLS_OK) return rc;
        *out = f.release();
        return FLS_OK;
    });
}

void fls_features_destroy(fls_features_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

fls_status fls_features_project(fls_features_handle h, const void* raw, size_t n, const fls_point_layout* layout, size_t* n_ordered) {
    if (!h || !layout || (!raw && n)) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->project(raw, n, *layout, n_ordered);
    });
}

fls_status fls_features_extract(fls_features_handle h, size_t* n_corner, size_t* n_planar) {
    if (!h) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->extract(n_corner, n_planar);
    });
}

size_t fls_features_get(fls_features_handle h, int what, void* out, size_t cap_elems) {
    if (!h) return 0;
    size_t n = 0;
    (void)guarded([&]() -> fls_status { n = h->get(what, out, cap_elems); return FLS_OK; });  // may read an introspection array back
    return n;
}

fls_status fls_features_get_time(fls_features_handle h, double* project_ms, double* extract_ms) {
    if (!h) return FLS_ERR_INVALID;
    if (project_ms) *project_ms = h->project_ms;
    if (extract_ms) *extract_ms = h->extract_ms;
    return FLS_OK;
}

// ---- the feature clouds kept on the device and handed to the LoamFull kind (include/fls_features_device.h) ----------------------
int fls_features_device_revision(void) { return FLS_FEATURES_DEVICE_REVISION; }

fls_status fls_features_keep_on_device(fls_features_handle h, int on) {
    if (!h) return FLS_ERR_INVALID;
    const bool want = on != 0;
    if (want != h->resident) {  // (no array of a projection made in the other mode is read in this one)
        h->resident = want;
        h->projected = h->extracted = false;
    }
    return FLS_OK;
}

fls_status fls_features_get_host_bytes(fls_features_handle h, uint64_t* d2h_bytes) {
    if (!h || !d2h_bytes) return FLS_ERR_INVALID;
    *d2h_bytes = h->d2h_bytes;
    return FLS_OK;
}

size_t fls_features_stat(fls_features_handle h, int what) { return (h && what >= 0 && what < 4) ? h->stats[what] : 0; }

fls_status fls_scan_attach_features(fls_handle m, fls_features_handle f, int filtered) {
    if (!m || !f || m->device != f->device) return FLS_ERR_INVALID;
    if (m->kind != FLS_LOAM_FULL || !f->extracted) return FLS_ERR_STATE;
    if (filtered && (!(f->p.corner_voxel_filter_size > 0.f) || !(f->p.planar_voxel_filter_size > 0.f))) return FLS_ERR_STATE;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(m->device));
        if (!f->resident) {  // the clouds the default mode left on the host: the ordinary upload
            const std::vector<PtI>& pl = filtered ? f->planar_f : f->planar;
            const std::vector<PtI>& co = filtered ? f->corner_f : f->corner;
            const fls_status rc = m->scan_upload(pl.empty() ? nullptr : &pl[0].x, pl.size(), co.empty() ? nullptr : &co[0].x, co.size(), 4);
            FLS_HIP(hipStreamSynchronize(m->stream));
            return rc;
        }
        const HandoffCloud pl = filtered ? f->rc_planar.filtered() : f->rc_planar.cloud();
        const HandoffCloud co = filtered ? f->rc_corner.filtered() : f->rc_corner.cloud();
        if (pl.n == 0 && co.n == 0) return m->scan_attach_features(pl, co);
        // the copies wait for the extraction and the filters (and anything else queued on the front end's stream); the front end's next
        // projection waits for the copies
        FLS_HIP(hipEventRecord(f->ev_ready, f->stream));
        FLS_HIP(hipStreamWaitEvent(m->stream, f->ev_ready, 0));
        const fls_status rc = m->scan_attach_features(pl, co);
        FLS_HIP(hipEventRecord(f->next_consumed_event(), m->stream));
        return rc;
    });
}

// ---- per-scan preprocessing: IMU de-skew, range gate, subsample, planar VoxelGrid (include/fls_preprocess.h) --------------------
fls_status fls_preprocess_create(const fls_preprocess_params* params, int device_id, fls_preprocess_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    if (!params || fls_preprocess::check(*params) != FLS_OK) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return FLS_ERR_DEVICE;
        hipDeviceProp_t prop;
        FLS_HIP(hipGetDeviceProperties(&prop, device_id));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FLS_ERR_DEVICE;
        std::unique_ptr<fls_preprocess> f(new fls_preprocess());
        f->p = *params;
        f->device = device_id;
        const fls_status rc = f->init();
        if (rc != FLS_OK) return rc;
        *out = f.release();
        return FLS_OK;
    });
}

void fls_preprocess_destroy(fls_preprocess_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

fls_status fls_preprocess_scan(fls_preprocess_handle h, const void* raw, size_t n, const fls_raw_layout* layout, uint64_t stamp_us, const uint64_t* imu_t_us,
                               const double* imu_q_xyzw, size_t n_imu, fls_preprocess_result* result) {
    if (!h || !layout || (!raw && n) || (result && result->struct_size != sizeof(fls_preprocess_result))) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->scan(raw, n, *layout, stamp_us, imu_t_us, imu_q_xyzw, n_imu, result);
    });
}

fls_status fls_preprocess_scan_device(fls_preprocess_handle h, const void* raw, size_t n, const fls_raw_layout* layout, uint64_t stamp_us,
                                      const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, fls_preprocess_result* result) {
    if (!h || !layout || (!raw && n) || (result && result->struct_size != sizeof(fls_preprocess_result))) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->scan(raw, n, *layout, stamp_us, imu_t_us, imu_q_xyzw, n_imu, result, /*on_device=*/true);
    });
}

size_t fls_preprocess_get(fls_preprocess_handle h, int what, void* out, size_t cap_elems) {
    if (!h) return 0;
    size_t n = 0;
    (void)guarded([&]() -> fls_status {  // (after a device scan the first request of an array downloads it)
        FLS_HIP(hipSetDevice(h->device));
        n = h->get(what, out, cap_elems);
        return FLS_OK;
    });
    return n;
}

fls_status fls_preprocess_get_host_bytes(fls_preprocess_handle h, uint64_t* d2h_bytes) {
    if (!h || !d2h_bytes) return FLS_ERR_INVALID;
    *d2h_bytes = h->d2h_bytes;
    return FLS_OK;
}

fls_status fls_scan_attach_preprocessed(fls_handle m, fls_preprocess_handle pre, int what) {
    if (!m || !pre || (what != FLS_PRE_ORDERED && what != FLS_PRE_PLANAR && what != FLS_PRE_PLANAR_FILTERED) || m->device != pre->device)
        return FLS_ERR_INVALID;
    if (m->kind == FLS_LOAM_FULL || m->is_lane || !pre->scan_done) return FLS_ERR_STATE;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(m->device));
        HandoffCloud c;
        const std::vector<PtI>* rows = nullptr;
        if (!pre->device_cloud(what, c, rows))  // the cloud the exact host filter made: the ordinary upload
            return m->scan_upload_raw(rows->empty() ? nullptr : &(*rows)[0].x, rows->size(), nullptr, 0, 4);
        if (c.n == 0) return m->scan_attach_device(c);
        // the copy waits for the scan (and anything else queued on its stream); the next scan's writes wait for the copy
        FLS_HIP(hipEventRecord(pre->ev_ready, pre->stream));
        FLS_HIP(hipStreamWaitEvent(m->stream, pre->ev_ready, 0));
        const fls_status rc = m->scan_attach_device(c);
        FLS_HIP(hipEventRecord(pre->next_consumed_event(), m->stream));
        return rc;
    });
}

fls_status fls_preprocess_get_time(fls_preprocess_handle h, double* deskew_ms, double* filter_ms) {
    if (!h) return FLS_ERR_INVALID;
    if (deskew_ms) *deskew_ms = h->deskew_ms;
    if (filter_ms) *filter_ms = h->filter_ms;
    return FLS_OK;
}

fls_status fls_features_project_deskew(fls_features_handle h, const void* raw, size_t n, const fls_raw_layout* layout, uint64_t stamp_us,
                                       const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, const double T_lidar_to_imu[16], size_t* n_ordered,
                                       int* imu_status) {
    if (!h || !layout || (!raw && n) || !T_lidar_to_imu) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return features_project_deskew(*h, raw, n, *layout, stamp_us, imu_t_us, imu_q_xyzw, n_imu, T_lidar_to_imu, n_ordered, imu_status);
    });
}

// ---- the driver-cloud front end (include/fls_ingest.h) ---------------------------------------------------------------------------
int fls_ingest_revision(void) { return FLS_INGEST_REVISION; }

fls_status fls_ingest_default_layout(int sensor, fls_driver_cloud* out) {
    if (!out || sensor < FLS_SENSOR_VELODYNE || sensor > FLS_SENSOR_NONE) return FLS_ERR_INVALID;
    fls_driver_cloud d{};
    d.struct_size = sizeof(d);
    d.sensor = sensor;
    d.point_step = 32;
    d.is_dense = 1;
    d.x_offset = 0; d.y_offset = 4; d.z_offset = 8; d.intensity_offset = 16;  // PCL_ADD_POINT4D, then the intensity
    switch (sensor) {
        case FLS_SENSOR_VELODYNE: d.ring_offset = 20; d.time_offset = 24; break;
        case FLS_SENSOR_OUSTER: d.time_offset = 20; d.ring_offset = 26; d.point_step = 48; break;  // t, reflectivity, ring, noise, range
        case FLS_SENSOR_LIVOX_AVIA: d.time_offset = 20; d.line_offset = 24; d.tag_offset = 25; break;
        case FLS_SENSOR_ROBOSENSE:
        case FLS_SENSOR_LEISHEN: d.ring_offset = 20; d.time_offset = 24; break;
        case FLS_SENSOR_LIVOX_MID_360: d.tag_offset = 20; d.line_offset = 21; d.time_offset = 24; break;
        default: break;  // pcl::PointXYZI
    }
    *out = d;
    return FLS_OK;
}

fls_status fls_preprocess_scan_driver(fls_preprocess_handle h, const void* msg, size_t n, const fls_driver_cloud* cloud, const fls_ingest_params* ingest,
                                      uint64_t stamp_us, const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, int keep_on_device,
                                      fls_preprocess_result* result, uint64_t* stamp_out_us, fls_ingest_info* info) {
    if (!h || !cloud || !ingest || (!msg && n) || (result && result->struct_size != sizeof(fls_preprocess_result)) ||
        (info && info->struct_size != sizeof(fls_ingest_info)))
        return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->scan_driver(msg, n, *cloud, *ingest, stamp_us, imu_t_us, imu_q_xyzw, n_imu, result, keep_on_device != 0, stamp_out_us, info);
    });
}

fls_status fls_features_project_driver(fls_features_handle h, const void* msg, size_t n, const fls_driver_cloud* cloud, const fls_ingest_params* ingest,
                                       uint64_t stamp_us, const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, const double T_lidar_to_imu[16],
                                       size_t* n_ordered, int* imu_status, uint64_t* stamp_out_us, fls_ingest_info* info) {
    if (!h || !cloud || !ingest || (!msg && n) || !T_lidar_to_imu || (info && info->struct_size != sizeof(fls_ingest_info))) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return features_project_driver(*h, msg, n, *cloud, *ingest, stamp_us, imu_t_us, imu_q_xyzw, n_imu, T_lidar_to_imu, n_ordered, imu_status,
                                       stamp_out_us, info);
    });
}

}  // extern "C"

// ---- the device keyframe store (include/fls_keyframes.h) --------------------------------------------------------------------------
namespace {
// guarded(), with a failed device allocation reported as what it is
template <typename F>
fls_status kf_guarded(F&& f) {
    return guarded([&]() -> fls_status {
        try {
            return f();
        } catch (const HipError& e) {
            if (e.code != hipErrorOutOfMemory) throw;
            (void)hipGetLastError();
            return FLS_ERR_NOMEM;
        }
    });
}
bool kf_leaf_ok(float leaf) { return std::isfinite(leaf) && leaf >= 0.f; }
bool kf_ids_ok(const fls_keyframes& h, const int32_t* ids, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (!h.valid_id(ids[k])) return false;
    return true;
}
}  // namespace

extern "C" {

int fls_keyframes_revision(void) { return FLS_KEYFRAMES_REVISION; }

fls_status fls_keyframes_create(int device_id, fls_keyframes_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    return kf_guarded([&]() -> fls_status {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return FLS_ERR_DEVICE;
        hipDeviceProp_t prop;
        FLS_HIP(hipGetDeviceProperties(&prop, device_id));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FLS_ERR_DEVICE;
        std::unique_ptr<fls_keyframes> s(new fls_keyframes());
        s->device = device_id;
        s->init();
        *out = s.release();
        return FLS_OK;
    });
}

void fls_keyframes_destroy(fls_keyframes_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

fls_status fls_keyframes_add(fls_keyframes_handle h, const float* pts, size_t n, int stride, int32_t* id) {
    if (!h || !id || (!pts && n) || stride < 3) return FLS_ERR_INVALID;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->add(pts, n, stride, id);
    });
}

fls_status fls_keyframes_add_preprocessed(fls_keyframes_handle h, fls_preprocess_handle pre, int what, int32_t* id) {
    if (!h || !pre || !id || (what != FLS_PRE_ORDERED && what != FLS_PRE_PLANAR && what != FLS_PRE_PLANAR_FILTERED) || h->device != pre->device)
        return FLS_ERR_INVALID;
    if (!pre->scan_done) return FLS_ERR_STATE;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->add_preprocessed(*pre, what, id);
    });
}

size_t fls_keyframes_count(fls_keyframes_handle h) { return h ? h->kf.size() : 0; }

fls_status fls_keyframes_get(fls_keyframes_handle h, int32_t id, float leaf, float* out, size_t cap, size_t* n_out) {
    if (!h || !n_out || (cap && !out) || !kf_leaf_ok(leaf) || !h->valid_id(id)) return FLS_ERR_INVALID;
    *n_out = 0;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->get(id, leaf, out, cap, n_out);
    });
}

fls_status fls_keyframes_merge(fls_keyframes_handle h, const int32_t* ids, const double* poses, size_t n_ids, float leaf_each, float leaf_final, float* out,
                               size_t cap, size_t* n_out) {
    if (!h || !n_out || (n_ids && (!ids || !poses)) || (cap && !out) || !kf_leaf_ok(leaf_each) || !kf_leaf_ok(leaf_final) || !kf_ids_ok(*h, ids, n_ids))
        return FLS_ERR_INVALID;
    *n_out = 0;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->merge(ids, poses, n_ids, leaf_each, leaf_final, out, cap, n_out);
    });
}

fls_status fls_keyframes_loop_match(fls_keyframes_handle h, const int32_t* src_ids, const double* src_poses, size_t n_src, const int32_t* tgt_ids,
                                    const double* tgt_poses, size_t n_tgt, double T[16], float* fitness, fls_loop_stats* stats) {
    if (!h || !T || !fitness || (n_src && (!src_ids || !src_poses)) || (n_tgt && (!tgt_ids || !tgt_poses)) || !kf_ids_ok(*h, src_ids, n_src) ||
        !kf_ids_ok(*h, tgt_ids, n_tgt))
        return FLS_ERR_INVALID;
    std::vector<float> src, tgt;
    const fls_status rc = kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        size_t n = 0;  // GetSubMap's leaf (loop_closure.cpp:219)
        const fls_status a = h->merge(src_ids, src_poses, n_src, 0.2f, 0.f, nullptr, 0, &n, &src);
        return a != FLS_OK ? a : h->merge(tgt_ids, tgt_poses, n_tgt, 0.2f, 0.f, nullptr, 0, &n, &tgt);
    });
    if (rc != FLS_OK) return rc;
    return fls_loop_match(h->device, src.data(), src.size() / 4, tgt.data(), tgt.size() / 4, 4, T, fitness, stats);
}

size_t fls_keyframes_stat(fls_keyframes_handle h, int slot) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    return h->stat(slot);
}

}  // extern "C"

// ---- the device local-map source (include/fls_localmap.h) ------------------------------------------------------------------------
namespace {
bool lm_grid_ok(double g) { return std::isfinite(g) && g > 0.0; }
bool lm_pose_ok(const double* T) { return T && std::isfinite(T[12]) && std::isfinite(T[13]) && std::isfinite(T[14]); }
}  // namespace

extern "C" {

int fls_localmap_revision(void) { return FLS_LOCALMAP_REVISION; }

fls_status fls_localmap_create(int device_id, fls_localmap_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    return kf_guarded([&]() -> fls_status {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return FLS_ERR_DEVICE;
        hipDeviceProp_t prop;
        FLS_HIP(hipGetDeviceProperties(&prop, device_id));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FLS_ERR_DEVICE;
        std::unique_ptr<fls_localmap> s(new fls_localmap());
        s->device = device_id;
        s->init();
        *out = s.release();
        return FLS_OK;
    });
}

void fls_localmap_destroy(fls_localmap_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

fls_status fls_localmap_set_global(fls_localmap_handle h, const float* pts, size_t n, int stride, float leaf, size_t* n_stored) {
    if (!h || (!pts && n) || stride < 3 || !kf_leaf_ok(leaf) || n > kLmMaxPoints) return FLS_ERR_INVALID;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->set_global(pts, n, stride, leaf, n_stored);
    });
}

fls_status fls_localmap_crop(fls_localmap_handle h, const double pose[16], int force, int* updated, size_t* n_local) {
    if (!h || !updated || !n_local || !lm_pose_ok(pose)) return FLS_ERR_INVALID;
    if (!h->global) return FLS_ERR_STATE;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->crop(pose, force, updated, n_local);
    });
}

fls_status fls_localmap_split(fls_localmap_handle h, double grid_size, size_t* n_tiles) {
    if (!h || !n_tiles || !lm_grid_ok(grid_size)) return FLS_ERR_INVALID;
    if (!h->global) return FLS_ERR_STATE;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->split(grid_size, n_tiles);
    });
}

fls_status fls_localmap_add_tile(fls_localmap_handle h, double grid_size, int32_t gx, int32_t gy, const float* pts, size_t n, int stride) {
    if (!h || (!pts && n) || stride < 3 || !lm_grid_ok(grid_size) || n > kLmMaxPoints || (h->grid_size != 0.0 && h->grid_size != grid_size)) return FLS_ERR_INVALID;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->add_tile(grid_size, gx, gy, pts, n, stride);
    });
}

fls_status fls_localmap_tiles(fls_localmap_handle h, int32_t* gxgy, uint32_t* counts, size_t cap, size_t* n_tiles) {
    if (!h || !n_tiles || (cap && (!gxgy || !counts))) return FLS_ERR_INVALID;
    return h->list_tiles(gxgy, counts, cap, n_tiles);
}

fls_status fls_localmap_get_tile(fls_localmap_handle h, int32_t gx, int32_t gy, float leaf, float* out, size_t cap, size_t* n_out) {
    if (!h || !n_out || (cap && !out) || !kf_leaf_ok(leaf) || !h->tiles.count(LmTileKey{gx, gy})) return FLS_ERR_INVALID;
    *n_out = 0;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->get_tile(gx, gy, leaf, out, cap, n_out);
    });
}

fls_status fls_localmap_load_tiles(fls_localmap_handle h, const double pose[16], float leaf, int* updated, size_t* n_local) {
    if (!h || !updated || !n_local || !lm_pose_ok(pose) || !kf_leaf_ok(leaf)) return FLS_ERR_INVALID;
    if (h->tiles.empty()) return FLS_ERR_STATE;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->load_tiles(pose, leaf, updated, n_local);
    });
}

fls_status fls_localmap_reset(fls_localmap_handle h) {
    if (!h) return FLS_ERR_INVALID;
    h->reset();
    return FLS_OK;
}

fls_status fls_localmap_get_local(fls_localmap_handle h, float* out, size_t cap, size_t* n_out) {
    if (!h || !n_out || (cap && !out)) return FLS_ERR_INVALID;
    *n_out = 0;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(h->device));
        return h->get_local(out, cap, n_out);
    });
}

fls_status fls_add_localmap_to_local_map(fls_handle m, fls_localmap_handle h) {
    if (!m || !h || m->device != h->device) return FLS_ERR_INVALID;
    if (h->n_local == 0) return FLS_ERR_STATE;
    return kf_guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(m->device));
        return h->add_to(*m);
    });
}

size_t fls_localmap_stat(fls_localmap_handle h, int slot) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    return h->stat(slot);
}

}  // extern "C"
