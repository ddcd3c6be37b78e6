// matcher_base.hpp -- common host state of one registration handle (stream, device
// Gauss-Newton state, wave partials, profiling events), the launch loop and the Match
// epilogue every kind shares (run_mailbox_loop = begin_match, run_chunks over wait_mailboxes, end_match;
// take_result), the group driver of the shared-launch batches (run_job_groups), the batch-lane clone (make_lane, make_owned_lane) and the
// scan upload helper.
#pragma once
#include "host_maps.hpp"
#include "kernels_handoff.hpp"
#include "kernels_p2plane.hpp"  // kTicketWords
#include <functional>
#include <memory>
#include <thread>
#if defined(__SSE__)
#include <xmmintrin.h>
#endif

struct fls_matcher {
    fls_kind kind;
    fls_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    fls_stats stats{};

    fls::DevBuf<fls::GnState> d_state;
    fls::PinnedBuf<fls::GnState> h_state;
    fls::DevBuf<double> d_partials_a, d_partials_b;
    fls::DevBuf<fls::TrafficCounters> d_tc;
    fls::PinnedBuf<fls::TrafficCounters> h_tc;

    // profiling (fls_set_profiling)
    bool profiling = false;      // hipEvents around every correspondence launch
    bool count_traffic = false;  // run the <COUNT=true> kernel variants (device traffic counters)
    // hipEvent pairs around the correspondence launches: a ring of kEvRing Matches so that nothing is resolved
    // (hipEventSynchronize / ElapsedTime) on the timed path; fls_get_kernel_time settles the pending pairs
    static constexpr int kEvRing = 64;
    std::vector<hipEvent_t> ev_pool;   // kEvRing x 2 x kMaxIter, created lazily
    hipEvent_t* ev = nullptr;          // the current Match's slice: ev[2 * it], ev[2 * it + 1]
    int ev_slot = -1;
    struct PendingEv { int slot, iters; };
    std::vector<PendingEv> ev_pending;
    double prof_ms = 0.0;
    int64_t prof_launches = 0;
    uint64_t prof_point_iters = 0;
    fls::TrafficCounters last_tc{0, 0, 0, 0};

    // iteration log of the last Match
    int log_n = 0;
    bool log_stale = false;  // mailbox path: the full GnState (with the per-iteration log) is fetched on demand

    // result mailbox (host-mapped pinned memory, see device_common.hpp)
    fls::Mailbox* mb_host = nullptr;
    fls::Mailbox* mb_dev = nullptr;
    unsigned match_id = 0;
    bool tail_exact = false;  // FLS_TAIL_EXACT=1: every 6x6 system through the Eigen-arithmetic solver (no LDL^T fast path)
    unsigned launch_word() const { return fls::LaunchWord::pack(match_id, tail_exact, p.max_iterations).w; }  // what the tail kernels get

    virtual ~fls_matcher() {
        for (hipEvent_t e : slot_ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : batch_tail_ev) if (e) (void)hipEventDestroy(e);
        if (batch_stream) { (void)hipStreamSynchronize(batch_stream); (void)hipStreamDestroy(batch_stream); }
        for (auto e : ev_pool) if (e) (void)hipEventDestroy(e);
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (mb_host) (void)hipHostFree(mb_host);
    }
    virtual fls_status add_cloud(const float* c0, size_t n0, const float* c1, size_t n1, int stride) = 0;
    // fls_add_localmap_to_local_map: what add_cloud(rows of `c`, 4 floats each) would leave, from a cloud that lies on this device as x | y | z |
    // intensity planes (the caller has ordered this handle's stream behind the producer).  rows(): the same cloud on the host, fetched when a
    // path needs it.  *took_planes: a device builder read the planes; otherwise the host entry point ran (default: every kind without one).
    using HostRows = std::function<const std::vector<fls::PtI>&()>;
    virtual fls_status add_cloud_device(const fls::HandoffCloud&, const HostRows& rows, bool* took_planes) {
        *took_planes = false;
        const std::vector<fls::PtI>& r = rows();
        return add_cloud(r.empty() ? nullptr : &r[0].x, r.size(), nullptr, 0, 4);
    }
    virtual fls_status scan_upload(const float* s0, size_t n0, const float* s1, size_t n1, int stride) = 0;
    // fls_match's upload: the Match follows at once, so a kind may leave the scan in its pinned staging buffer and let the first
    // iteration's kernels read it from there (default: the ordinary upload)
    virtual fls_status scan_upload_for_match(const float* s0, size_t n0, const float* s1, size_t n1, int stride) { return scan_upload(s0, n0, s1, n1, stride); }
    // fls_scan_upload_raw: kinds whose Match filters its source (ICP, NDT) keep the RAW scan resident and filter inside match_resident
    virtual fls_status scan_upload_raw(const float* s0, size_t n0, const float* s1, size_t n1, int stride) { return scan_upload(s0, n0, s1, n1, stride); }
    // fls_scan_attach_preprocessed: what fls_scan_upload_raw(rows of `c`) would leave, from a cloud that already lies on this device.  The
    // copy kernel is queued on this handle's stream (the caller has ordered it behind the producer); host copies are fetched on demand.
    virtual fls_status scan_attach_device(const fls::HandoffCloud&) { return FLS_ERR_STATE; }
    // fls_scan_attach_features: what fls_scan_upload(rows of `planar`, rows of `corner`) would leave, from the two feature clouds lying
    // on this device (the LoamFull kind; same ordering contract as scan_attach_device)
    virtual fls_status scan_attach_features(const fls::HandoffCloud& /*planar*/, const fls::HandoffCloud& /*corner*/) { return FLS_ERR_STATE; }
    virtual fls_status match_resident(double* T, int update_map, fls_stats* out) = 0;
    virtual fls_status fitness(float max_range, float* score) = 0;
    virtual int correspondences(int slot, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) = 0;
    virtual size_t map_size(int slot) const = 0;
    virtual size_t map_export(void*, size_t) { return 0; }                       // 0: this kind has no exportable image
    virtual fls_status map_import(const void*, size_t) { return FLS_ERR_STATE; }
    // the DEVICE image as one flat buffer (fls_map_image_*): 0 / FLS_ERR_STATE: this kind has none
    virtual size_t map_image_bytes() { return 0; }
    virtual fls_status map_image_export(void*, size_t, int /*buffer on this handle's device*/) { return FLS_ERR_STATE; }
    virtual fls_status map_image_import(const void*, size_t, int) { return FLS_ERR_STATE; }
    // the iVox blob at device speed (include/fls_map_ivox.h): 0 / FLS_ERR_STATE: not an iVox handle
    virtual size_t ivox_blob_bytes() { return 0; }
    virtual fls_status ivox_blob_export(void*, size_t, int /*buffer on this handle's device*/) { return FLS_ERR_STATE; }
    virtual fls_status ivox_blob_import(const void*, size_t, int) { return FLS_ERR_STATE; }
    // fls_replicas_*: this handle becomes a READ-ONLY copy of `owner`'s device map image (device to device, no host mirror): it serves
    // fls_match_batch (and fls_match with update_map == 0) and nothing else until fls_map_import makes it an ordinary handle again (fls_add_cloud_to_local_map is refused: FLS_ERR_STATE)
    virtual bool can_replicate() const { return false; }
    virtual fls_status replicate_from(fls_matcher&) { return FLS_ERR_STATE; }
    // state a FRESH reference matcher would not have (e.g. nearest_points_ of an earlier Match): cleared per batch job
    virtual void reset_job_state() {}
    // Batch of independent registrations against the CURRENT map (BASELINE configs[4]): every job is what a
    // fresh reference process holding this map would compute for Match(scan_j, T_j) -- no map update, no state carried
    // from job to job.  With lanes > 1 the jobs run on `lanes` clones of this handle (own stream, own
    // Gauss-Newton state, mailbox and per-point buffers; one host thread each, spinning on its own mailbox) that READ
    // this handle's resident map: while one job runs its single-workgroup tail or an under-occupied fit kernel, the
    // correspondence kernels of the other jobs fill the machine.  lanes <= 1: one clone, jobs one after the other.
    std::vector<std::unique_ptr<fls_matcher>> lanes;
    bool is_lane = false;
    virtual std::unique_ptr<fls_matcher> clone_for_lane() { return nullptr; }  // same kind, borrowing this handle's map
    bool have_map = false;  // a map has been built on the device (every kind but iVox, whose image is built on demand)
    // the map image current and complete on the device, the owner's stream idle
    virtual fls_status prepare_batch() { FLS_HIP(hipStreamSynchronize(stream)); return have_map ? FLS_OK : FLS_ERR_STATE; }
    virtual void tune_lane(fls_matcher&) {}                                    // copy run-time switches to a lane
    // fls_knn_order.h: only the iVox point-to-plane kind has a reference order to select
    virtual fls_status set_knn_order(int mode) { return mode == FLS_KNN_ORDER_DEFAULT ? FLS_OK : FLS_ERR_STATE; }
    virtual int knn_order() const { return FLS_KNN_ORDER_DEFAULT; }
    // at least `want` lane clones, if they can be set up; returns how many of `want` exist
    size_t ensure_lanes(size_t want) {
        while (lanes.size() < want) {
            std::unique_ptr<fls_matcher> q = clone_for_lane();
            if (!q) break;
            q->is_lane = true;
            lanes.push_back(std::move(q));
        }
        return std::min(want, lanes.size());
    }
    // The start of fls_match_batch / fls_match_batch_fused: every status FLS_SKIPPED (overwritten by every job that runs), the map made
    // ready; returns how many of the `want` lanes (clamped to [1, kMaxLanes] and to n_jobs) exist, or the status (<= 0) to return at once.  Jobs never
    // run on the owner itself: its Match state (nearest_points_, keyframe gate, resident scan, final pose) belongs to the SLAM thread's next fls_match.
    static constexpr int kMaxLanes = 16;
    int begin_batch(size_t n_jobs, int32_t* status, int want) {
        if (is_lane) return FLS_ERR_STATE;
        if (status) for (size_t j = 0; j < n_jobs; ++j) status[j] = FLS_SKIPPED;
        if (n_jobs == 0) return FLS_OK;
        const fls_status prc = prepare_batch();
        if (prc != FLS_OK) return prc;
        const size_t width = ensure_lanes(std::min(size_t(std::max(1, std::min(want, kMaxLanes))), n_jobs));
        return width ? int(width) : int(FLS_ERR_NOMEM);  // (the clone could not be set up)
    }
    fls_status match_batch(size_t n_jobs, const float* const* s0, const size_t* n0, const float* const* s1, const size_t* n1, int stride,
                           double* T, fls_stats* st, int32_t* status, int n_lanes) {
        const int width = begin_batch(n_jobs, status, n_lanes);  // lanes <= 1 (or a single job) = one lane clone, back to back
        if (width <= 0) return fls_status(width);
        const size_t L = size_t(width);
        std::vector<fls_status> lane_rc(L, FLS_OK);
        fls::Threads th;
        for (size_t l = 0; l < L; ++l) {
            fls_matcher* q = lanes[l].get();
            tune_lane(*q);
            q->expect_iters = expect_iters;
            th.start([=, &lane_rc]() {
                lane_rc[l] = fls::guarded([&]() -> fls_status {
                    FLS_HIP(hipSetDevice(q->device));
                    for (size_t j = l; j < n_jobs; j += L) {
                        q->reset_job_state();
                        fls_status rc = q->scan_upload(s0[j], n0[j], s1 ? s1[j] : nullptr, n1 ? n1[j] : 0, stride);
                        if (rc == FLS_OK) rc = q->match_resident(T + 16 * j, 0, st ? &st[j] : nullptr);
                        if (status) status[j] = int32_t(rc);
                        if (rc < 0) return rc;  // (the lane's remaining jobs stay FLS_SKIPPED)
                    }
                    return FLS_OK;
                }, "batch lane", l);
            });
        }
        th.join();
        for (const fls_status rc : lane_rc) if (rc < 0) return rc;
        return FLS_OK;
    }

    // fls_match_batch_fused (include/fls_batch.h): the same jobs, but the iteration launches of up to n_slots jobs are SHARED (one launch per
    // iteration for the whole group; slots = the lane clones above).  A kind without that form runs the jobs as match_batch does, on n_slots lanes.
    // fls_batch_stat: [0] shared iteration launches queued, [1] jobs that ran in shared launches, [2] jobs that took the per-lane path, [3] groups
    // (since the handle was created)
    size_t batch_counters[4] = {0, 0, 0, 0};
    virtual fls_status match_batch_fused(size_t n_jobs, const float* const* s0, const size_t* n0, const float* const* s1, const size_t* n1, int stride,
                                         double* T, fls_stats* st, int32_t* status, int n_slots) {
        if (!is_lane) batch_counters[2] += n_jobs;
        return match_batch(n_jobs, s0, n0, s1, n1, stride, T, st, status, n_slots);
    }

    // fls_match_batch_shared_ivox (include/fls_batch_ivox.h): the shared form of the iVox point-to-plane kind; every other kind answers as
    // fls_match_batch_fused does.  fls_batch_ivox_stat: [0] shared kNN launches queued, [1] shared fit launches queued, [2] jobs that ran in
    // shared launches, [3] jobs that ran outside them, [4] groups (since the handle was created)
    size_t batch_ivox_counters[5] = {0, 0, 0, 0, 0};
    virtual fls_status match_batch_shared_ivox(size_t n_jobs, const float* const* s0, const size_t* n0, const float* const* s1, const size_t* n1, int stride,
                                               double* T, fls_stats* st, int32_t* status, int n_slots) {
        return match_batch_fused(n_jobs, s0, n0, s1, n1, stride, T, st, status, n_slots);
    }

    // ---- the group driver of the shared-launch batches (IcpMatcher::match_batch_fused, P2PlaneIvoxMatcher::match_batch_shared_ivox) ----
    // Slots are the lane clones.  Per group: every slot uploads and prepares its job on its own stream and its own host thread (the ICP source filters
    // are latency chains with a host wait each: they overlap), records an event, and the batch stream, behind those events, carries the group's iteration
    // launches through run_chunks; the host waits on all the group's mailboxes.  Prepare, begin / end and finish are the single-job path's.
    // With more than one group there are two sets of slots: the next group's uploads run while this group iterates.
    // A kind supplies: prepare(q, slot, job, shared&) -- reset_job_state has run; upload + prepare of one job on slot q, `shared` = it waits for the
    // group's launches (otherwise the status returned is the job's answer); table(call) -- the job-table entries of call.act (a Match has begun on each)
    // and whatever else the group's launches need, queued on the batch stream; queue(call, first) -- one iteration's launches for the group on the batch
    // stream; finish(q, job, word) -- end_match + the epilogue of one job.
    hipStream_t batch_stream = nullptr;
    hipEvent_t batch_tail_ev[2] = {nullptr, nullptr};  // per slot set: behind the last launch queued for the set's previous group
    std::vector<hipEvent_t> slot_ev;                   // per slot: its job's scan is resident and prepared
    int fused_expect_iters = 4;                        // the first chunk of a group: the previous group's largest iteration count
    static hipEvent_t new_event() { hipEvent_t e = nullptr; FLS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return e; }
    // what the steps of one call share
    template <class M>
    struct GroupCall {
        const float* const* s0; const size_t* n0; int stride;  // the caller's arrays
        double* T; fls_stats* st; int32_t* status;
        size_t G;                          // slots per set
        std::vector<fls_status> job_rc;    // per job
        std::vector<char> shared;          // per slot: its job waits for the group's shared launches
        bool tail_pending[2] = {false, false};  // launches of the set's previous group may still be queued on the batch stream
        // the jobs of the current group that run in its shared launches
        std::vector<M*> act;
        std::vector<size_t> act_job, act_slot;
        std::vector<unsigned> word;             // what each published last
        void set_rc(const size_t j, const fls_status rc) { job_rc[j] = rc; if (status) status[j] = int32_t(rc); }
        fls_stats* stats_of(const size_t j) const { return st ? &st[j] : nullptr; }
    };
    struct GroupCounters { size_t *shared_jobs, *outside_jobs, *groups; };
    template <class M, class Prep, class Table, class Queue, class Finish>
    fls_status run_job_groups(size_t n_jobs, const float* const* s0, const size_t* n0, int stride, double* T, fls_stats* st, int32_t* status, int n_slots,
                              const GroupCounters ctr, Prep&& prepare, Table&& table, Queue&& queue, Finish&& finish) {
        const int width = begin_batch(n_jobs, status, n_slots);
        if (width <= 0) return fls_status(width);
        GroupCall<M> c{s0, n0, stride, T, st, status, size_t(width)};
        const size_t G = c.G, n_groups = (n_jobs + G - 1) / G;
        const size_t n_sets = (n_groups > 1 && ensure_lanes(2 * G) == 2 * G) ? 2 : 1;
        if (!batch_stream) {
            FLS_HIP(hipStreamCreateWithFlags(&batch_stream, hipStreamNonBlocking));
            for (hipEvent_t& e : batch_tail_ev) e = new_event();
        }
        while (slot_ev.size() < n_sets * G) { slot_ev.push_back(nullptr); slot_ev.back() = new_event(); }
        c.job_rc.assign(n_jobs, FLS_SKIPPED);
        c.shared.resize(n_sets * G);
        // (1) per slot, side by side: upload + prepare.  A rejected job keeps its status; a job that does not wait for the shared launches is
        // answered here (on the slot's own stream, if it launches at all).
        auto slot_step = [this, &c, &prepare](const size_t set, const size_t l, const size_t j) {
            const size_t s = set * c.G + l;
            M* q = static_cast<M*>(lanes[s].get());
            c.shared[s] = 0;
            c.set_rc(j, fls::guarded([&]() -> fls_status {
                FLS_HIP(hipSetDevice(q->device));
                // an exit-at-once launch of the set's previous group reads this slot's state words: the slot's stream stays behind it
                if (c.tail_pending[set]) FLS_HIP(hipStreamWaitEvent(q->stream, batch_tail_ev[set], 0));
                tune_lane(*q);
                q->reset_job_state();
                bool shared = false;
                const fls_status rc = prepare(q, s, j, shared);
                if (rc == FLS_OK && shared) { FLS_HIP(hipEventRecord(slot_ev[s], q->stream)); c.shared[s] = 1; }
                return rc;
            }, "shared batch slot", s));
        };
        fls::Threads th[2];  // per slot set
        auto start_group = [&](const size_t k) {
            const size_t base = k * G, g = std::min(G, n_jobs - base), set = k % n_sets;
            if (n_jobs == 1) { slot_step(set, 0, base); return; }
            for (size_t l = 0; l < g; ++l) th[set].start([&slot_step, set, l, base] { slot_step(set, l, base + l); });
        };
        start_group(0);
        for (size_t k = 0; k < n_groups; ++k) {
            const size_t base = k * G, g = std::min(G, n_jobs - base), set = k % n_sets;
            ++*ctr.groups;
            th[set].join();
            if (n_sets == 2 && k + 1 < n_groups) start_group(k + 1);  // the next group's uploads run beside this group's iterations
            // (2) a Match begins on every slot of [set * G, set * G + g) that waits for the shared launches
            c.act.clear(); c.act_job.clear(); c.act_slot.clear();
            for (size_t l = 0; l < g; ++l) {
                const size_t s = set * G + l;
                if (!c.shared[s]) {
                    if (c.job_rc[base + l] >= 0) ++*ctr.outside_jobs;  // (it ran, outside the shared launches)
                    continue;
                }
                M* q = static_cast<M*>(lanes[s].get());
                q->begin_match(int(p.max_iterations));
                FLS_HIP(hipStreamWaitEvent(batch_stream, slot_ev[s], 0));
                c.act.push_back(q);
                c.act_job.push_back(base + l);
                c.act_slot.push_back(s);
            }
            c.word.assign(c.act.size(), 0u);
            if (!c.act.empty()) {
                // (3) the group's launches on the batch stream, until every job has stopped or run max_iterations
                const size_t A = c.act.size();
                *ctr.shared_jobs += A;
                table(c);
                run_chunks(int(p.max_iterations), fused_expect_iters, [&](int, int first) { queue(c, first); }, [](int) {},
                           [&](int launched) { return wait_mailboxes(batch_stream, c.act.data(), A, c.word.data(), launched); });
                FLS_HIP(hipEventRecord(batch_tail_ev[set], batch_stream));
                c.tail_pending[set] = true;
                // (4) the epilogue per job
                fused_expect_iters = 2;
                for (size_t i = 0; i < A; ++i) {
                    M* q = c.act[i];
                    c.set_rc(c.act_job[i], finish(q, c.act_job[i], c.word[i]));
                    fused_expect_iters = std::max(fused_expect_iters, q->expect_iters);
                }
            }
            if (n_sets == 1 && k + 1 < n_groups) start_group(k + 1);
        }
        // the slots are also match_batch's lanes, which launch on their own streams: nothing of this call stays queued behind the return
        if (c.tail_pending[0] || c.tail_pending[1]) FLS_HIP(hipStreamSynchronize(batch_stream));
        for (size_t j = 0; j < n_jobs; ++j)
            if (c.job_rc[j] < 0) return c.job_rc[j];  // the first negative status by job index; every job has run
        return FLS_OK;
    }

    void init_common() {
        if (const char* e = std::getenv("FLS_TAIL_EXACT")) tail_exact = std::atoi(e) != 0;
        FLS_HIP(hipSetDevice(device));
        FLS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        d_state.reserve(1);
        h_state.reserve(1);
        d_tc.reserve(1);
        h_tc.reserve(1);
        FLS_HIP(hipMemsetAsync(d_tc.p, 0, sizeof(fls::TrafficCounters), stream));
        FLS_HIP(hipHostMalloc((void**)&mb_host, sizeof(fls::Mailbox), hipHostMallocMapped));
        std::memset(mb_host, 0, sizeof(fls::Mailbox));
        mb_host->seq = 0u;
        FLS_HIP(hipHostGetDevicePointer((void**)&mb_dev, mb_host, 0));
    }
    void ensure_events(int iters) {
        if (ev_pool.empty()) {
            // the whole ring at once, on the first profiled Match (bench.py makes that an untimed one): creating a slot's events lazily
            // put ~20 hipEventCreate calls (30+ us) inside every bracketed step that met a fresh slot
            ev_pool.assign(size_t(kEvRing) * 2 * fls::kMaxIter, nullptr);
            for (hipEvent_t& e : ev_pool) FLS_HIP(hipEventCreate(&e));
        }
        ev_slot = (ev_slot + 1) % kEvRing;
        for (const PendingEv& pe : ev_pending)
            if (pe.slot == ev_slot) { settle_events(); break; }  // the ring wrapped around
        ev = ev_pool.data() + size_t(ev_slot) * 2 * fls::kMaxIter;
        for (int i = 0; i < 2 * iters; ++i)
            if (!ev[i]) FLS_HIP(hipEventCreate(&ev[i]));
    }
    void settle_events() {
        for (const PendingEv& pe : ev_pending) {
            hipEvent_t* e = ev_pool.data() + size_t(pe.slot) * 2 * fls::kMaxIter;
            for (int i = 0; i < pe.iters; ++i) {
                float ms = 0.f;
                FLS_HIP(hipEventSynchronize(e[2 * i + 1]));
                FLS_HIP(hipEventElapsedTime(&ms, e[2 * i], e[2 * i + 1]));
                prof_ms += ms;
                prof_launches += 1;
            }
        }
        ev_pending.clear();
    }
    // Spin on the mailboxes of hs[0, n) (all launched on `s`) until every one carries its handle's current Match and that Match has
    // run `target` iterations or has hit the stop rule.  words[i] = what hs[i] published; returns whether every Match has stopped.
    // Falls back to the stream state every few thousand polls so that a faulted kernel cannot hang the host.
    template <class M>
    static bool wait_mailboxes(hipStream_t s, M* const* hs, size_t n, unsigned* words, int target) {
        bool all_stopped = true;
        auto ready = [&] {
            bool ok = all_stopped = true;
            for (size_t i = 0; i < n; ++i) {
                const fls::SeqWord sq{__atomic_load_n(&hs[i]->mb_host->seq, __ATOMIC_ACQUIRE)};
                words[i] = sq.w;
                if (!sq.reached(hs[i]->match_id, target)) ok = false;
                if (!sq.done()) all_stopped = false;
            }
            return ok;
        };
        if (!fls::spin_until(s, ready)) (void)ready();  // everything drained: the words are final
        return all_stopped;
    }
    // the part of the Match epilogue every kind shares: the iteration count of the published word and the mailbox's residual block into `stats`
    const fls::Mailbox& take_result(unsigned word) {
        const fls::Mailbox& mb = *mb_host;
        stats.iterations = fls::SeqWord{word}.iterations();
        stats.n_valid = mb.n_valid;
        stats.sum_res = mb.sum_res;
        std::memcpy(stats.last_dx, mb.last_dx, sizeof(stats.last_dx));
        return mb;
    }
    // the fan-in ticket words of a kind's fused tail: zero between launches (their last arrivers reset them), so zeroed once here
    void init_tickets(fls::DevBuf<unsigned>& t) {
        t.reserve(fls::kTicketWords);
        FLS_HIP(hipMemsetAsync(t.p, 0, fls::kTicketWords * sizeof(unsigned), stream));
    }
    // fetch the full device state (iteration log) after a mailbox-path Match
    void refresh_log() {
        if (!log_stale) return;
        FLS_HIP(hipMemcpyAsync(h_state.p, d_state.p, sizeof(fls::GnState), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        log_n = std::min(h_state.p->iter, fls::kMaxIter);
        log_stale = false;
    }
    // remember the hipEvent-bracketed launches of the executed iterations (settled lazily)
    void account_profile(int iters, size_t points_per_iter) {
        if (!profiling) return;
        ev_pending.push_back(PendingEv{ev_slot, std::min(iters, fls::kMaxIter)});
        prof_point_iters += uint64_t(iters) * points_per_iter;
    }
    // Gauss-Newton launch loop shared by every kind.  Iterations are enqueued in chunks sized by the previous
    // Match (steady-state SLAM needs about the same number every scan); the device decides convergence, kernels
    // of a finished Match exit at once, and the host learns the outcome from the mailbox without a blocking
    // synchronisation.  Three parts, so that a group of handles can share the middle one (run_job_groups):
    // begin_match per handle, run_chunks once, end_match per handle with the word that handle published.
    int expect_iters = 4;
    void begin_match(int iters) {
        match_id = fls::LaunchWord::next_id(match_id);
        if (profiling) ensure_events(iters);
        if (count_traffic) FLS_HIP(hipMemsetAsync(d_tc.p, 0, sizeof(fls::TrafficCounters), stream));
    }
    // queue(it, first) enqueues one iteration; after_chunk(launched) runs once a chunk is queued, before the host waits (speculative work
    // behind the chunk); wait(launched) returns once every mailbox it watches shows `launched` iterations or a stop: true when all stopped
    template <class Q, class A, class W>
    static void run_chunks(int iters, int first_chunk, Q&& queue, A&& after_chunk, W&& wait) {
        int launched = 0;
        int chunk = std::max(1, std::min(iters, first_chunk));
        for (;;) {
            const int end = std::min(iters, launched + chunk);
            for (int it = launched; it < end; ++it) queue(it, it == 0 ? 1 : 0);
            launched = end;
            after_chunk(launched);
            FLS_HIP(hipGetLastError());
            if (wait(launched) || launched >= iters) break;
            chunk = 2;
        }
    }
    void end_match(unsigned word, size_t points_per_iter) {
        const int used = fls::SeqWord{word}.iterations();
        expect_iters = std::max(2, used);
        log_stale = true;
        log_n = std::min(used, fls::kMaxIter);
        account_profile(used, points_per_iter);
        if (count_traffic) {
            FLS_HIP(hipMemcpyAsync(h_tc.p, d_tc.p, sizeof(fls::TrafficCounters), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            last_tc = *h_tc.p;
        }
    }
    // launch(it, first) enqueues one iteration; returns the published mailbox word
    template <class F>
    unsigned run_mailbox_loop(int iters, size_t points_per_iter, F&& launch) {
        return run_mailbox_loop(iters, points_per_iter, launch, [](int) {});
    }
    template <class F, class G>
    unsigned run_mailbox_loop(int iters, size_t points_per_iter, F&& launch, G&& after_chunk) {
        begin_match(iters);
        fls_matcher* const self = this;  // the one-handle case of the wait
        unsigned word = 0;
        run_chunks(iters, expect_iters, launch, after_chunk, [&](int launched) { return wait_mailboxes(stream, &self, 1, &word, launched); });
        end_match(word, points_per_iter);
        return word;
    }
};

namespace fls {

// SoA device copy of a source cloud
struct DevScan {
    struct View { float* p = nullptr; };
    DevBuf<float> xyz;  // x[n] | y[n] | z[n] in one allocation: one host-to-device copy per upload
    View x, y, z;
    PinnedBuf<float> stage;
    size_t n = 0;
    std::vector<PtI> host;  // kept for map updates / fitness
    // attach_device: the scan was written on the device (x | y | z | intensity); the pinned staging copy / `host` are fetched only
    // when a map update or a declined device path reads them
    bool stage_stale = false, host_stale = false;
    bool dev_intensity = false;  // the scan's intensity plane lies on the device, at xyz.p + 3 n (an attached scan; an upload sends x | y | z)
    void attach_device(const HandoffCloud& c, hipStream_t s, bool want_host) {
        n = c.n;
        host.clear();
        stage_stale = n != 0;
        dev_intensity = n != 0;
        host_stale = want_host && n != 0;
        if (n == 0) return;
        xyz.reserve(4 * n);
        x.p = xyz.p; y.p = xyz.p + n; z.p = xyz.p + 2 * n;
        handoff_launch(c, xyz.p, s);
        FLS_HIP(hipGetLastError());
    }
    void fetch_stage(hipStream_t s) {
        if (!stage_stale) return;
        stage.reserve(4 * n);
        FLS_HIP(hipMemcpyAsync(stage.p, xyz.p, 4 * n * sizeof(float), hipMemcpyDeviceToHost, s));
        FLS_HIP(hipStreamSynchronize(s));
        stage_stale = false;
    }
    void fetch_host(hipStream_t s) {
        if (!host_stale) return;
        fetch_stage(s);
        host.resize(n);
        for (size_t i = 0; i < n; ++i) host[i] = PtI{stage.p[i], stage.p[n + i], stage.p[2 * n + i], stage.p[3 * n + i]};
        host_stale = false;
    }
    void push(hipStream_t s, int fields = 3) {
        xyz.reserve(size_t(fields) * n);
        x.p = xyz.p; y.p = xyz.p + n; z.p = xyz.p + 2 * n;
        FLS_HIP(hipMemcpyAsync(xyz.p, stage.p, size_t(fields) * n * sizeof(float), hipMemcpyHostToDevice, s));
    }
    // straight from the caller's strided AoS into the pinned SoA staging buffer x[n] | y[n] | z[n] | intensity[n] (no
    // temporary cloud, no per-point host copy).  The first 3 n floats go to the device; the staged intensities stay valid
    // until the next upload, which is all a map update of THIS resident scan needs (fls_match == fls_scan_upload +
    // fls_match_resident for either value of update_map).
    void upload_raw(const float* p, size_t count, int stride, hipStream_t s, bool intensity_too = false) {
        stage_raw(p, count, stride);
        if (n) push(s, intensity_too ? 4 : 3);  // the device VoxelGrid averages the intensity as well
    }
    // device-side address of the staging buffer (pinned host memory is mapped into the device's address space)
    const float* stage_dev() const {
        void* d = nullptr;
        FLS_HIP(hipHostGetDevicePointer(&d, stage.p, 0));
        return static_cast<const float*>(d);
    }
    // the device allocation x | y | z of the staged scan, without the copy (a kernel fills it: ivox_knn_kernel's first launch)
    void reserve_device() {
        xyz.reserve(size_t(3) * n);
        x.p = xyz.p; y.p = xyz.p + n; z.p = xyz.p + 2 * n;
    }
    void stage_raw(const float* p, size_t count, int stride) {
        n = count;
        host.clear();
        stage_stale = host_stale = false;
        dev_intensity = false;
        if (n == 0) return;
        stage.reserve(4 * n);
        float* sx = stage.p; float* sy = stage.p + n; float* sz = stage.p + 2 * n; float* si = stage.p + 3 * n;
        size_t i = 0;
#if defined(__SSE__)
        if (stride == 4) {  // packed xyzi rows: 4 x 4 transposes (45 -> ~12 us for 115,200 points)
            for (; i + 4 <= n; i += 4) {
                __m128 r0 = _mm_loadu_ps(p + 4 * i), r1 = _mm_loadu_ps(p + 4 * i + 4), r2 = _mm_loadu_ps(p + 4 * i + 8), r3 = _mm_loadu_ps(p + 4 * i + 12);
                _MM_TRANSPOSE4_PS(r0, r1, r2, r3);
                _mm_storeu_ps(sx + i, r0); _mm_storeu_ps(sy + i, r1); _mm_storeu_ps(sz + i, r2); _mm_storeu_ps(si + i, r3);
            }
        } else if (stride == 3) {  // packed xyz: three vectors hold four points
            const __m128 zero = _mm_setzero_ps();
            for (; i + 4 <= n; i += 4) {
                const __m128 a = _mm_loadu_ps(p + 3 * i), b = _mm_loadu_ps(p + 3 * i + 4), c = _mm_loadu_ps(p + 3 * i + 8);
                const __m128 m2 = _mm_shuffle_ps(b, c, _MM_SHUFFLE(2, 1, 3, 2));  // b2 b3 c1 c2
                const __m128 m1 = _mm_shuffle_ps(a, b, _MM_SHUFFLE(1, 0, 2, 1));  // a1 a2 b0 b1
                _mm_storeu_ps(sx + i, _mm_shuffle_ps(a, m2, _MM_SHUFFLE(2, 0, 3, 0)));   // a0 a3 b2 c1
                _mm_storeu_ps(sy + i, _mm_shuffle_ps(m1, m2, _MM_SHUFFLE(3, 1, 2, 0)));  // a1 b0 b3 c2
                _mm_storeu_ps(sz + i, _mm_shuffle_ps(m1, c, _MM_SHUFFLE(3, 0, 3, 1)));   // a2 b1 c0 c3
                _mm_storeu_ps(si + i, zero);
            }
        } else if (stride == 8) {  // pcl::PointXYZI: {x, y, z, pad | intensity, pad, pad, pad}
            for (; i + 4 <= n; i += 4) {
                __m128 r0 = _mm_loadu_ps(p + 8 * i), r1 = _mm_loadu_ps(p + 8 * i + 8), r2 = _mm_loadu_ps(p + 8 * i + 16), r3 = _mm_loadu_ps(p + 8 * i + 24);
                _MM_TRANSPOSE4_PS(r0, r1, r2, r3);
                _mm_storeu_ps(sx + i, r0); _mm_storeu_ps(sy + i, r1); _mm_storeu_ps(sz + i, r2);
                si[i] = p[8 * i + 4]; si[i + 1] = p[8 * i + 12]; si[i + 2] = p[8 * i + 20]; si[i + 3] = p[8 * i + 28];
            }
        }
#endif
        for (; i < n; ++i) {
            const float* q = p + i * stride;
            sx[i] = q[0]; sy[i] = q[1]; sz[i] = q[2]; si[i] = intensity_of(q, stride);
        }
    }
    float staged_intensity(size_t i) const { return stage.p[3 * n + i]; }
    void upload(const std::vector<PtI>& c, hipStream_t s) {
        host = c;
        n = c.size();
        stage_stale = host_stale = false;
        dev_intensity = false;
        if (n == 0) return;
        stage.reserve(3 * n);
        for (size_t i = 0; i < n; ++i) { stage.p[i] = c[i].x; stage.p[n + i] = c[i].y; stage.p[2 * n + i] = c[i].z; }
        push(s);
    }
};

// a batch lane of `self` (fls_matcher::clone_for_lane): a fresh handle of the same kind, parameters and device; the caller points it at its map
template <class M>
std::unique_ptr<M> make_lane(const M& self) {
    auto q = std::make_unique<M>();
    q->kind = self.kind; q->p = self.p; q->device = self.device;
    if (q->init() != FLS_OK) return nullptr;
    return q;
}
template <class M>  // the same for the kinds whose lanes read the map through an `owner` pointer
std::unique_ptr<M> make_owned_lane(const M& self) { auto q = make_lane(self); if (q) q->owner = &self; return q; }

inline fls_status check_common(const fls_params& p) {
    if (p.struct_size != sizeof(fls_params)) return FLS_ERR_INVALID;
    if (p.max_iterations == 0 || p.max_iterations > (uint32_t)kMaxIter) return FLS_ERR_INVALID;
    return FLS_OK;
}
inline bool unset_d(double v) { return v == std::numeric_limits<double>::max() || !(v == v); }
inline bool unset_f(float v) { return v == std::numeric_limits<float>::max() || !(v == v); }

}  // namespace fls
