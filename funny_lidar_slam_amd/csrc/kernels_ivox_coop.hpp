// kernels_ivox_coop.hpp -- the production iVox point-to-plane path, split for the machine:
//
//   ivox_knn_kernel      four lanes cooperate on ONE source point, for the brick image (DENSE) and the hash-table image alike:
//                        the 19 voxel probes are dealt round-robin to the four lanes (all probe loads of a wave are in
//                        flight together); the hit voxels are compacted into a per-group LDS table and their points,
//                        concatenated, cut into four equal contiguous ranges, one per lane (balanced split); every lane
//                        scans its range four loads at a time into a private sorted top-5 of keys
//                        {float-bits(d2) : map slot} held as IEEE doubles (v_min_f64 / v_max_f64 insertion), and the
//                        four private lists are merged by five rounds of a DPP group-min.  On the brick image's lean form a
//                        wave whose 16 queries fall into <= 3 voxels first stages those voxels' neighbourhoods in LDS once and
//                        scans them from there (shared runs, below).  48-60 VGPRs over the 16
//                        instantiations (52 / 54 for the brick image's product forms, lean / GEN) and 16 KiB of LDS per
//                        256-thread workgroup -> 8 waves/SIMD, four times as many waves as points/64: the dependent
//                        gathers (cell -> voxel points) are hidden by thread-level parallelism instead of being
//                        serialised in one lane (the first, fused kernel spent 117 us per launch that way).
//                        Output: the neighbour list of point i as <= 5 map slots (ids form, nn_ids[i][8]) + count;
//                        untouched when no candidate exists (ivox_map.cpp:21-23 quirk).  (With nn_ids == nullptr the
//                        list leaves as gathered rows nearest_points_[i] instead; the matcher never asks for that.)
//   p2plane_fit_solve_kernel  one lane per source point: 5x3 column-pivoted Householder plane fit, gates,
//                        Jacobian (FP64), the Q1 stale-slot rule, DPP wave reduction of the 6x6 system; the last
//                        workgroup to finish also runs the Gauss-Newton tail (solve, pose update, stop rule).
//                        127-128 VGPRs; the compiler's occupancy figure is 4 waves/SIMD for the 512-thread form, 3 for the 256-thread one.
//   ivox_knn_jobs_kernel / p2plane_fit_solve_jobs_kernel  the same two launches for a group of independent registrations against one map
//                        (fls_match_batch_shared_ivox): grid (rows_max, jobs), a device job table; the bodies are the single-job kernels' own.
//
// Exact-tie rule of the selection: lower map slot wins (the reference's order under exact float ties is
// libstdc++-introselect-defined; parity tests count such queries).
#pragma once
#include "kernels_p2plane.hpp"
#include "lane_group.hpp"

namespace fls {

// NEARBY18 offsets (ivox_map.cpp:50-54) packed 2 bits per entry (value + 1), entry k at bits [2k, 2k+1]:
// a per-lane probe index needs no table load.
//   dx: 0,-1,1,0,0,0,0,1,-1,1,-1,1,-1,1,-1,0,0,0,0
//   dy: 0,0,0,1,-1,0,0,1,1,-1,-1,0,0,0,0,1,-1,1,-1
//   dz: 0,0,0,0,0,-1,1,0,0,0,0,1,1,-1,-1,1,1,-1,-1
__device__ __forceinline__ void nearby18(const int k, int& dx, int& dy, int& dz) {
    constexpr unsigned long long DX = 0x1548889561ull, DY = 0x895429495ull, DZ = 0x282956155ull;
    dx = (int)((DX >> (2 * k)) & 3ull) - 1;
    dy = (int)((DY >> (2 * k)) & 3ull) - 1;
    dz = (int)((DZ >> (2 * k)) & 3ull) - 1;
}

// The same offsets as slab offsets of the brick image, (dz * S + dy) * S + dx with S = kBrickStored (within +-111), for the four probes
// k = sub + 4 r of round r packed as signed bytes, byte `sub`: a lane extracts its offset with one v_bfe_i32 on 8 * sub.
// (k >= 19, the last lane of the last round: offset 0, its count is zeroed by the caller)
constexpr int nearby18_slab(const int k) {
    constexpr unsigned long long DX = 0x1548889561ull, DY = 0x895429495ull, DZ = 0x282956155ull;
    const int dx = (int)((DX >> (2 * k)) & 3ull) - 1, dy = (int)((DY >> (2 * k)) & 3ull) - 1, dz = (int)((DZ >> (2 * k)) & 3ull) - 1;
    return (dz * kBrickStored + dy) * kBrickStored + dx;
}
constexpr unsigned nearby18_slab_pack4(const int r) {
    unsigned pk = 0u;
    for (int s = 0; s < 4; ++s) {
        const int k = s + 4 * r;
        pk |= ((unsigned)(k < 19 ? nearby18_slab(k) : 0) & 0xffu) << (8 * s);
    }
    return pk;
}
static_assert((kBrickStored + 1) * kBrickStored + 1 <= 127, "slab offsets of the 18 neighbours fit a signed byte");

// Selection keys as IEEE doubles: the 64-bit key {float-bits(d2) + kKeyBias : map slot} read as a positive NORMAL
// double orders exactly like the unsigned integer (sign 0, exponent field >= 1 thanks to the bias, never Inf/NaN
// because d2 < 25), so a sorted insertion is nine full-rate v_min_f64 / v_max_f64 instead of five 64-bit
// compares and twenty selects.  "No candidate" = high word kKeyNoneHi (largest finite exponent; any low word).
constexpr unsigned kKeyBias = 0x00100000u, kKeyNoneHi = 0x7FEFFFFFu, kKeyValidLimit = 0x7FE00000u;
__device__ __forceinline__ double kmin_f64(const double a, const double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double kmax_f64(const double a, const double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double make_dkey(const float d2, const unsigned slot, const bool ok) {
    return __hiloint2double((int)(ok ? __float_as_uint(d2) + kKeyBias : kKeyNoneHi), (int)slot);
}
__device__ __forceinline__ bool dkey_valid(const double k) { return (unsigned)__double2hiint(k) < kKeyValidLimit; }
__device__ __forceinline__ unsigned dkey_slot(const double k) { return (unsigned)__double2loint(k); }
__device__ __forceinline__ void top5_insert_dkey(double (&t)[5], const double key) {
    double x = kmin_f64(t[4], key);
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        const double lo = kmin_f64(t[j], x), hi = kmax_f64(t[j], x);
        t[j + 1] = hi;
        x = lo;
    }
    t[0] = x;
}
// minimum over the four lanes of a query's group: two quad-permute exchanges
template <int STEP>
__device__ __forceinline__ double dpp_min_dkey(const double v) {
    const unsigned lo = dpp_pair_u32<STEP>((unsigned)__double2loint(v));
    const unsigned hi = dpp_pair_u32<STEP>((unsigned)__double2hiint(v));
    return kmin_f64(v, __hiloint2double((int)hi, (int)lo));
}
__device__ __forceinline__ double group_min_dkey(const double v) { return dpp_min_dkey<1>(dpp_min_dkey<0>(v)); }

// Rows form (nn_ids == nullptr, the only form before round 3): 9.2 MB of nearest_points_ rows per launch at the benchmark size,
// flushed from the write-back L2 at the kernel boundary
// (2.7 us of this kernel + 3.2 us of re-reads in the fit kernel, measured by removing the stores).  Nontemporal stores
// measured -0.5 us per launch, -0.5 us per Match (inside the noise), write-through (sc1) stores were slower (18.6-21.2 us
// per launch): the rows are plain stores.
// GEN (the general form) keeps two things the host can rule out for a whole map (matcher_p2plane_ivox.hpp::map_view):
//   - the max_range gate d2 < 25 per candidate.  A query lies within half a voxel of its voxel's centre on each axis, a candidate within
//     half a voxel of a centre at most one voxel away: every axis difference is <= 2 res, d2 <= 12 res^2 (3 at the 0.5 m of InitIVox).
//     The host drops the gate where 27 res^2 < 25, i.e. with a whole extra voxel per axis (3 res) for the float rounding of key and
//     difference (at |key| near 2^20 one ulp of a coordinate is res / 8); the selection keys then stay finite doubles as with the gate.
//   - 64-bit candidate addresses.  With slots x 16 bytes < 2^32 the four loads of a trip take a 32-bit byte offset from the uniform base.
// The body of workgroup blockIdx.x of ONE registration: ivox_knn_kernel is that registration alone, ivox_knn_jobs_kernel runs one per blockIdx.y.
// The LDS is the calling kernel's (one array, declared there through FLS_IVOX_KNN_SMEM_DECL, as icp_knn_fit_body's is).
// Shared runs (brick image, !GEN): the 16 queries of a wave are 16 neighbouring azimuths of one ring of the ring-major scan and mostly fall into a
// few voxels.  A RUN is a maximal stretch of consecutive queries of a wave with the same (kx, ky, kz, have).  A wave with at most kIvoxKnnRunMax runs
// whose 19-voxel neighbourhoods hold at most kIvoxKnnStageCap map points together probes each run's 19 cells once (one lane per (run, probe): 3 x 19 = 57
// lanes, one pass), copies the runs' points once into its LDS region as {x, y, z, map slot} -- one flat round trip, every load of the copy in flight
// together, coalesced along the voxels' slot ranges -- and every query scans its run's staged range from LDS.  A query's candidate set stays exactly the
// points of its 19 voxels and the distances are computed from the same float bits in the same order: the key set {d2 bits : slot} of every query, hence
// its list, is the per-query code's.  Any other wave runs the per-query code.  (tools/knn_run_stats.py: what the gate admits on the headline scan.)
constexpr int kIvoxKnnRunMax = 3;
constexpr int kIvoxKnnStageCap = 256;
constexpr int kIvoxKnnQueries = 256 / 4;  // queries per workgroup (four lanes each)
// One LDS region per wave, used either as the per-query voxel tables (16 queries x 24 words of s_end, then 16 x 24 of s_off) or as the staging area.
constexpr int kIvoxKnnWaveWords = kIvoxKnnStageCap * 4;
static_assert(kIvoxKnnWaveWords >= 2 * 16 * 24, "the per-query tables of a wave fit its region");
static_assert(4 * kIvoxKnnWaveWords * sizeof(unsigned) <= 20480, "eight workgroups per CU: the 1,800-workgroup launch stays one round");
static_assert(kIvoxKnnRunMax * 19 <= 64 && kIvoxKnnStageCap <= 4 * 64, "one probe pass, four staged rows per lane");
static_assert(kIvoxKnnRunMax == 3, "the leader and range selects of the shared path are written out for three runs");
#define FLS_IVOX_KNN_SMEM_PARAMS unsigned (&s_knn)[256 / 64][kIvoxKnnWaveWords]
#define FLS_IVOX_KNN_SMEM_DECL __shared__ __attribute__((aligned(16))) unsigned s_knn[256 / 64][kIvoxKnnWaveWords]
#define FLS_IVOX_KNN_SMEM_ARGS s_knn
template <bool COUNT, bool DENSE, bool FIRST, bool GEN, class P>
__device__ __forceinline__ void
ivox_knn_body(FLS_IVOX_KNN_SMEM_PARAMS, const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, const int n,
              const GnState* __restrict__ st, const P& T0p /* Pose16, or Pose16Ref: the pose stays where it is */, const DevGrid grid, const BrickDir bd,
              const float inv_res, float4* __restrict__ nn_pts /* [n][5] */, unsigned char* __restrict__ nn_cnt,
              unsigned char* __restrict__ flag, TrafficCounters* __restrict__ tc, const int chunk,
              unsigned* __restrict__ nn_ids /* [n][8]: map slots of the neighbours (ids form); nullptr: rows form */,
              const int nn_prev /* FIRST: size of nearest_points_ before this Match; the grown tail starts empty (:257 resize) */,
              float* __restrict__ dev_copy /* FIRST, may be null: sx / sy / sz point into the pinned staging buffer (host memory);
                                              leave the device copy x[n] | y[n] | z[n] here for the launches that follow */) {
    const Pose16& T0 = T0p;
    constexpr int G = 4;                 // lanes per query
    constexpr int QPB = kIvoxKnnQueries; // queries per workgroup
    constexpr int R = (19 + G - 1) / G;  // probe rounds per lane
    // XCD-aware block order: the dispatcher deals consecutive workgroups round-robin to the 8 XCDs, each with its own
    // 4 MiB L2.  Re-map so that XCD x walks CHUNKS of `chunk` consecutive workgroups (chunk * QPB consecutive points of
    // the ring-major, hence spatially coherent, scan), the chunks of the 8 XCDs interleaved.  One contiguous eighth of
    // the scan per XCD (the first version) caches best but balances worst: the rings differ in map density, the
    // busiest XCD carried 38 % more candidate work than the mean.  Affects speed only.
    // (the grid is launched rounded up to a multiple of 8 * chunk so that the re-map is a bijection)
    const int nb = (n + QPB - 1) / QPB;
    const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
    const int lb = ((seq / chunk) * 8 + xcd) * chunk + (seq % chunk);
    const int sub = threadIdx.x % G;
    const int q = lb * QPB + threadIdx.x / G;
    // the wave's LDS region, and this query's rows of the per-query voxel tables in it
    unsigned* const s_wave = &s_knn[threadIdx.x >> 6][0];
    unsigned* const s_end = s_wave + 24 * ((threadIdx.x / G) & 15);
    unsigned* const s_off = s_end + 16 * 24;
    const bool active = lb < nb && q < n;
    // issue the state / source loads before looking at the stop flag: one memory round trip instead of three
    // (source loads are unconditional on a clamped index: a guarded load costs a branch and a wait each).
    // The FIRST iteration of a Match takes the initial pose from the launch arguments and ignores the
    // (stale) device state; it also clears the per-point valid flags (std::fill once per Match, Q1).
    const int done = FIRST ? 0 : st->done;
    double T[12];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) T[c * 3 + r] = FIRST ? T0.m[c * 4 + r] : st->T[c * 4 + r];
    const int qq = active ? q : 0;
    const float px = sx[qq], py = sy[qq], pz = sz[qq];
    if (done) return;
    if (FIRST && active && sub == 0) {
        if (dev_copy) { dev_copy[q] = px; dev_copy[(size_t)n + q] = py; dev_copy[2 * (size_t)n + q] = pz; }
        flag[q] = 0;
        if (q >= nn_prev) nn_cnt[q] = 0;  // (an unaligned hipMemsetAsync of the tail cost up to three fill kernels in front of the Match)
    }
    const double x = px, y = py, z = pz;
    const float ptx = (float)(((T[0] * x + T[3] * y) + T[6] * z) + T[9]);
    const float pty = (float)(((T[1] * x + T[4] * y) + T[7] * z) + T[10]);
    const float ptz = (float)(((T[2] * x + T[5] * y) + T[8] * z) + T[11]);
    const float fx = roundf(ptx * inv_res), fy = roundf(pty * inv_res), fz = roundf(ptz * inv_res);
    const bool in_range = active && fabsf(fx) < (float)kKeyLimit && fabsf(fy) < (float)kKeyLimit && fabsf(fz) < (float)kKeyLimit;
    const int kx = in_range ? (int)fx : 0, ky = in_range ? (int)fy : 0, kz = in_range ? (int)fz : 0;

    // phase 1: this lane's probes (k = sub, sub+G, ...): issue every first-slot load before resolving any.
    // Written as explicit per-round scalars (no indexed arrays) so that nothing lands in scratch.
    const double kNone = __hiloint2double((int)kKeyNoneHi, -1);
    double t5[5] = {kNone, kNone, kNone, kNone, kNone};
    unsigned long long c_hits = 0, c_cand = 0, c_probes = 0;
    auto probe_key = [&](const int r, bool& pv) -> unsigned long long {
        const int k = sub + G * r;
        pv = in_range && k < 19;
        int ox, oy, oz;
        nearby18(k < 19 ? k : 0, ox, oy, oz);
        return pack_key(kx + ox, ky + oy, kz + oz);
    };
    auto first_load = [&](const bool pv, const unsigned long long key, unsigned& h) -> HashEntry {
        h = hash_key(key) & grid.mask;
        return pv ? grid.table[h] : HashEntry{kEmptyKey, 0u, 0u};
    };
    // resolve a probe (linear probing on collision) to its voxel's point range; count = 0 on a miss
    auto resolve = [&](const bool pv, const unsigned long long key, unsigned h, HashEntry ek, unsigned& beg, unsigned& cnt) {
        while (pv && ek.key != key && ek.key != kEmptyKey) {
            h = (h + 1) & grid.mask;
            ek = grid.table[h];
        }
        const bool hit = pv && ek.key == key;
        beg = hit ? ek.begin : 0u;
        cnt = hit ? ek.count : 0u;
        if (COUNT && pv) { c_probes++; if (hit) { c_hits++; c_cand += ek.count; } }
    };
    // scan a lane's candidates (the dependent-load latency is paid once per four candidates; the tail of a range re-reads its last point, masked out)
    auto consider = [&](const float4 p, const unsigned s, const bool ok) {
        const float dx = p.x - ptx, dy = p.y - pty, dz = p.z - ptz;
        const float d2 = dx * dx + (dy * dy + dz * dz);  // Eigen Vector3f::squaredNorm order
        top5_insert_dkey(t5, make_dkey(d2, s, GEN ? ok && d2 < 25.0f : ok));  // max_range 5.0 squared (!GEN: cannot bind, see above)
    };
    auto map_pt = [&](const unsigned s) -> float4 {
        if (GEN) return grid.pts[s];
        return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(grid.pts) + (s << 4));  // (32-bit byte offset, as reduce_partials_trip)
    };
    bool have = false;     // brick image: the query's brick exists
    unsigned cbase = 0u;   // ... and the query's own cell in its slab
    if (DENSE) {
        // brick image (device_common.hpp): ONE directory look-up per query -- the same 16-byte entry for the lanes of a group -- then
        // every probe is a slab offset from the query's own cell (the slab's halo mirrors the neighbouring bricks' boundary cells):
        // no bounds checks, one aligned 8-byte load per probe, neighbouring voxels share cache lines
        const int bx = kx >> kBrickLog, by = ky >> kBrickLog, bz = kz >> kBrickLog;
        const unsigned long long bkey = pack_key(bx, by, bz);
        unsigned h = brick_hash(bx, by, bz) & bd.mask;
        HashEntry be = bd.table[h];
        while (be.key != bkey && be.key != kEmptyKey) {  // (linear probing; the directory is at most a quarter full)
            h = (h + 1) & bd.mask;
            be = bd.table[h];
        }
        have = in_range && be.key == bkey && be.begin < bd.n_cap;
        cbase = (have ? be.begin : 0u) * kBrickStride +
                brick_slab_index((kx & (kBrickSide - 1)) + 1, (ky & (kBrickSide - 1)) + 1, (kz & (kBrickSide - 1)) + 1);
    }
    bool shared = false;  // wave-uniform: this wave takes the shared-run path
    if (DENSE && !GEN) {
        const unsigned lane = threadIdx.x & 63u;
        // Run detection: a query starts a run when (kx, ky, kz, have) differs from the query before it in the wave; query 0 always does.  (A query
        // that is inactive or beyond the key range has key 0 and no brick: it belongs to a run without candidates.)  The four lanes of a query agree.
        const int kxh = kx * 2 + (have ? 1 : 0);
        const int pkx = __shfl_up(kxh, G, 64), pky = __shfl_up(ky, G, 64), pkz = __shfl_up(kz, G, 64);
        const bool start = lane < (unsigned)G || pkx != kxh || pky != ky || pkz != kz;
        const unsigned long long starts = __ballot(start) & 0x1111111111111111ull;  // bit 4 g: query g of the wave starts a run
        const int nruns = __popcll(starts);
        if (nruns <= kIvoxKnnRunMax) {
            // the runs' leader lanes (wave-uniform) and what the probe lanes need of them: the leader's cell and whether its brick exists
            const unsigned long long rest1 = starts & (starts - 1ull), rest2 = rest1 & (rest1 - 1ull), have_mask = __ballot(have);
            const int l1 = rest1 ? __ffsll((long long)rest1) - 1 : 0, l2 = rest2 ? __ffsll((long long)rest2) - 1 : 0;
            const unsigned cb0 = (unsigned)__builtin_amdgcn_readlane((int)cbase, 0), cb1 = (unsigned)__builtin_amdgcn_readlane((int)cbase, l1),
                           cb2 = (unsigned)__builtin_amdgcn_readlane((int)cbase, l2);
            const bool hv0 = (have_mask & 1ull) != 0ull, hv1 = rest1 != 0ull && ((have_mask >> l1) & 1ull) != 0ull,
                       hv2 = rest2 != 0ull && ((have_mask >> l2) & 1ull) != 0ull;
            // one lane per (run, probe): lane 19 r + k probes cell k of run r (lanes 57..63 and the lanes of a run the wave does not have load a cell
            // of some run and count nothing); every load stays inside the leader's slab, as the per-query probes do
            const unsigned pr = lane / 19u, pk = lane - 19u * pr;
            int ox, oy, oz;
            nearby18((int)pk, ox, oy, oz);
            const int poff = (oz * kBrickStored + oy) * kBrickStored + ox;
            const unsigned pcb = pr == 0u ? cb0 : pr == 1u ? cb1 : cb2;
            const bool phv = pr == 0u ? hv0 : pr == 1u ? hv1 : pr == 2u ? hv2 : false;
            const uint2 pe = bd.cells[pcb + (unsigned)poff];
            const unsigned pbeg = pe.x, pcnt_all = phv ? pe.y : 0u;
            // wave prefix over the probe lanes' counts: run r's points take the contiguous staging range [S_r, S_r+1).  (Counts enter clamped to
            // CAP + 1, so that the sum cannot wrap; a clamped count fails the gate.)
            const unsigned pcnt = pcnt_all < (unsigned)kIvoxKnnStageCap + 1u ? pcnt_all : (unsigned)kIvoxKnnStageCap + 1u;
            unsigned inc = pcnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = __shfl_up(inc, o, 64);
                if (lane >= (unsigned)o) inc += t;
            }
            const unsigned pex = inc - pcnt;
            const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)inc, 63);
            if (total <= (unsigned)kIvoxKnnStageCap) {
                shared = true;
                const unsigned S1 = (unsigned)__builtin_amdgcn_readlane((int)pex, 19), S2 = (unsigned)__builtin_amdgcn_readlane((int)pex, 38);
                // this query's run: the runs that start at or before its lane
                const int my_run = __popcll(starts & ((2ull << lane) - 1ull)) - 1;
                const unsigned sh_beg = my_run == 0 ? 0u : my_run == 1 ? S1 : S2, sh_end = my_run == 0 ? S1 : my_run == 1 ? S2 : total;
                if (COUNT) {  // every active query: its 19 probes, its run's hit voxels and candidates; the wave counts once as shared
                    const unsigned long long hit_mask = __ballot(pcnt != 0u);
                    const unsigned hits_run = (unsigned)__popcll((hit_mask >> (19 * my_run)) & 0x7FFFFull);
                    if (active && sub == 0) { c_probes += 19u; c_hits += hits_run; c_cand += sh_end - sh_beg; }
                    if (__ballot(active) != 0ull && lane == 0u) atomicAdd(&tc->shared, 1ull);
                }
                // Staging.  (1) every probe lane writes the slots of its voxel into the slot words of its entries, (2) lane l takes entries l, l + 64,
                // l + 128, l + 192: slot from LDS, point from the map -- all loads of the copy issued before the first is used -- (3) the entry becomes
                // {x, y, z, slot}.  Entries [0, total) only; total <= CAP keeps everything inside the wave's region.
                for (unsigned i = 0u; i < pcnt; ++i) s_wave[4u * (pex + i) + 3u] = pbeg + i;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                uint4* const stage = reinterpret_cast<uint4*>(s_wave);
                unsigned sl[4] = {0u, 0u, 0u, 0u};
                float4 sp[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned en = lane + 64u * (unsigned)j;
                    sp[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (en < total) { sl[j] = s_wave[4u * en + 3u]; sp[j] = map_pt(sl[j]); }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned en = lane + 64u * (unsigned)j;
                    if (en < total) stage[en] = make_uint4(__float_as_uint(sp[j].x), __float_as_uint(sp[j].y), __float_as_uint(sp[j].z), sl[j]);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // Scan: the query's four lanes cut its run's range [0, C) into four equal contiguous parts, four entries per trip from LDS
                const unsigned C = sh_end - sh_beg, Q = (C + 3u) >> 2, a = (unsigned)sub * Q, e = a + Q < C ? a + Q : C;
                const uint4* const runp = stage + sh_beg;
                for (unsigned idx = a; idx < e; idx += 4u) {
                    const unsigned last = e - 1u, i1 = idx + 1u, i2 = idx + 2u, i3 = idx + 3u;
                    const uint4 r0 = runp[idx], r1 = runp[i1 < last ? i1 : last], r2 = runp[i2 < last ? i2 : last], r3 = runp[i3 < last ? i3 : last];
                    consider(make_float4(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), 0.f), r0.w, true);
                    consider(make_float4(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z), 0.f), r1.w, i1 <= last);
                    consider(make_float4(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z), 0.f), r2.w, i2 <= last);
                    consider(make_float4(__uint_as_float(r3.x), __uint_as_float(r3.y), __uint_as_float(r3.z), 0.f), r3.w, i3 <= last);
                }
            }
        }
    }
    unsigned b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    if (shared) {
        // (the wave's candidates are in its top-5 lists already)
    } else if (DENSE) {
        constexpr unsigned PK[5] = {nearby18_slab_pack4(0), nearby18_slab_pack4(1), nearby18_slab_pack4(2), nearby18_slab_pack4(3), nearby18_slab_pack4(4)};
        const unsigned sub8 = 8u * (unsigned)sub;
        auto cell = [&](const int r, const unsigned pk4, unsigned& beg, unsigned& cnt) {
            const int k = sub + G * r;
            const int off = __builtin_amdgcn_sbfe((int)pk4, sub8, 8u);
            const bool ok = have && k < 19;
            const uint2 e = bd.cells[cbase + (unsigned)off];  // (always inside the slab)
            beg = e.x;
            cnt = ok ? e.y : 0u;
            if (COUNT && active && k < 19) { c_probes++; if (cnt) { c_hits++; c_cand += cnt; } }  // (a query beyond the key range probes 19 absent voxels)
        };
        cell(0, PK[0], b0, c0);
        cell(1, PK[1], b1, c1);
        cell(2, PK[2], b2, c2);
        cell(3, PK[3], b3, c3);
        cell(4, PK[4], b4, c4);
    } else {
        bool pv0 = false, pv1 = false, pv2 = false, pv3 = false, pv4 = false;
        unsigned long long k0 = 0, k1 = 0, k2 = 0, k3 = 0, k4 = 0;
        unsigned h0 = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0;
        HashEntry e0{kEmptyKey, 0u, 0u}, e1 = e0, e2 = e0, e3 = e0, e4 = e0;
        k0 = probe_key(0, pv0); e0 = first_load(pv0, k0, h0);
        k1 = probe_key(1, pv1); e1 = first_load(pv1, k1, h1);
        k2 = probe_key(2, pv2); e2 = first_load(pv2, k2, h2);
        k3 = probe_key(3, pv3); e3 = first_load(pv3, k3, h3);
        k4 = probe_key(4, pv4); e4 = first_load(pv4, k4, h4);
        resolve(pv0, k0, h0, e0, b0, c0);
        resolve(pv1, k1, h1, e1, b1, c1);
        resolve(pv2, k2, h2, e2, b2, c2);
        resolve(pv3, k3, h3, e3, b3, c3);
        resolve(pv4, k4, h4, e4, b4, c4);
        if (COUNT && active && !in_range) {  // (a query beyond the key range probes 19 absent voxels)
#pragma unroll
            for (int r = 0; r < R; ++r) c_probes += sub + G * r < 19 ? 1u : 0u;
        }
    }
    if (!shared) {
    // per-query scan of this lane's share of the query's voxels, 4 point loads in flight per trip
    const unsigned tot = c0 + c1 + c2 + c3 + c4;  // this lane's candidates
    // Balanced split: the group's candidates (all hit voxels of the query, concatenated) are cut into four equal
    // contiguous ranges, one per lane, instead of whole voxels per lane: a wave runs max-over-lanes trips of the
    // loop below, and voxels hold 1..20+ points (4.7 trips of four candidates per wave before, 2.8 after).
    // The hit voxels are compacted into a per-group LDS table {prefix end, begin - prefix start}; a lane walks
    // its range through a two-entry window of that table (see the loop).
    const unsigned nz = (c0 ? 1u : 0u) + (c1 ? 1u : 0u) + (c2 ? 1u : 0u) + (c3 ? 1u : 0u) + (c4 ? 1u : 0u);
    const unsigned packed = tot * 32u + nz;  // candidates (< 2^27) and hit voxels (<= 19 per group) of this lane
    const unsigned t0 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)packed, 0x00, 0xf, 0xf, true);  // quad broadcasts
    const unsigned t1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)packed, 0x55, 0xf, 0xf, true);
    const unsigned t2 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)packed, 0xAA, 0xf, 0xf, true);
    const unsigned t3 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)packed, 0xFF, 0xf, 0xf, true);
    const unsigned before = (sub > 0 ? t0 : 0u) + (sub > 1 ? t1 : 0u) + (sub > 2 ? t2 : 0u), all = t0 + t1 + t2 + t3;
    const unsigned TOT = all >> 5;
    unsigned pos = before & 31u, run = before >> 5;
    // every entry behind the last real one is a sentinel (the window looks one entry ahead, the start search
    // four): the whole row is filled first, the real entries overwrite (LDS operations of a wave are in order)
    {
        uint2* const rowp = reinterpret_cast<uint2*>(&s_end[6 * sub]);
        rowp[0] = make_uint2(~0u, ~0u); rowp[1] = make_uint2(~0u, ~0u); rowp[2] = make_uint2(~0u, ~0u);
    }
    // predicated, not branched: a missed probe writes its pair to a word of the lane's own behind the table (real entries: 0..18; the
    // window reads k + 1 <= 19, the start search up to entry 18 + 4, so the s_end word is made a sentinel again after the last put)
    const unsigned dmy = 20u + (unsigned)sub;
    auto put = [&](const unsigned b, const unsigned c) {
        const unsigned at = c ? pos : dmy;
        s_off[at] = b - run;
        run += c;
        s_end[at] = run;
        pos += c ? 1u : 0u;
    };
    put(b0, c0);
    put(b1, c1);
    put(b2, c2);
    put(b3, c3);
    put(b4, c4);
    s_end[dmy] = ~0u;
    // a group lives inside one wave and the LDS serves a wave's operations in order: no workgroup barrier, only a
    // compiler-level ordering point between the table writes and the cross-lane reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const unsigned Q = (TOT + 3u) >> 2, a = sub * Q, e = a + Q < TOT ? a + Q : TOT;
    // Start search: k = first table entry whose range reaches past a = number of entries that end at or before a.  The quad
    // broadcasts already say which lane's entries hold candidate a: P_i = packed sum of the lanes before lane i = {candidates before
    // lane i : entries before lane i}, and P_i <= 32 a + 31 <=> candidates before lane i <= a.  With j the last such lane, every entry
    // before lane j's first one ends at or before a, lane j's own (at most five) are compared, and whatever follows them in the table
    // (later lanes' entries, sentinels) ends past a.  Five compares in place of twenty.
    const unsigned P2 = t0 + t1, P3 = P2 + t2, A32 = a * 32u + 31u;
    unsigned ps = t0 <= A32 ? t0 : 0u;
    ps = P2 <= A32 ? P2 : ps;
    ps = P3 <= A32 ? P3 : ps;
    unsigned k = ps & 31u;  // (<= 19: the five words read below stay inside the row)
    {
        const unsigned* const w = &s_end[k];
        const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        k += (w0 <= a ? 1u : 0u) + (w1 <= a ? 1u : 0u) + (w2 <= a ? 1u : 0u) + (w3 <= a ? 1u : 0u) + (w4 <= a ? 1u : 0u);
    }
    // Two-run window: a trip resolves its four candidates against the run idx lies in (entry k: E(k-1) <= idx < E(k)) and the
    // next one, and ends where the second run ends -- 2.2 % of the trips would reach into a third run (runs average 5.1 points),
    // cutting them costs 0.8 % more trips and saves a five-entry select chain per candidate.  The candidates of [a, e) are still
    // taken once each, only grouped differently: the same top-5 set.  (Behind the last run E1 is the sentinel: the trip ends at e.)
    for (unsigned idx = a; idx < e;) {
        const unsigned E0 = s_end[k], E1 = s_end[k + 1];
        const unsigned O0 = s_off[k], O1 = s_off[k + 1];
        const unsigned last = (E1 < e ? E1 : e) - 1;
        const unsigned i1 = idx + 1, i2 = idx + 2, i3 = idx + 3;
        const unsigned j1 = i1 < last ? i1 : last, j2 = i2 < last ? i2 : last, j3 = i3 < last ? i3 : last;
        const unsigned s0 = idx + O0;
        const unsigned s1 = j1 + (j1 < E0 ? O0 : O1);
        const unsigned s2 = j2 + (j2 < E0 ? O0 : O1);
        const unsigned s3 = j3 + (j3 < E0 ? O0 : O1);
        const float4 q0 = map_pt(s0), q1 = map_pt(s1), q2 = map_pt(s2), q3 = map_pt(s3);
        consider(q0, s0, true);
        consider(q1, s1, i1 <= last);
        consider(q2, s2, i2 <= last);
        consider(q3, s3, i3 <= last);
        idx = j3 + 1;  // min(idx + 4, end of the second run, e)
        k += (E0 <= idx ? 1u : 0u) + (E1 <= idx ? 1u : 0u);  // (runs are never empty: E1 == idx puts idx into run k + 2)
    }
    }  // (!shared)
    // phase 2: merge the four private lists: five rounds of group-min + pop (keys are unique -- the slot is the low
    // word -- so exactly one lane pops per round); the neighbour count is the number of valid minima
    const double m0 = group_min_dkey(t5[0]);
    if (dkey_valid(m0)) {  // uniform within the group: at least one candidate (else nothing is written, ivox_map.cpp:21-23)
        int cnt = 0;
        unsigned sid[5] = {~0u, ~0u, ~0u, ~0u, ~0u};
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const double m = j == 0 ? m0 : group_min_dkey(t5[0]);
            const bool mv = dkey_valid(m);
            cnt += mv ? 1 : 0;
            if (mv && __double_as_longlong(t5[0]) == __double_as_longlong(m)) {
                t5[0] = t5[1]; t5[1] = t5[2]; t5[2] = t5[3]; t5[3] = t5[4]; t5[4] = kNone;
            }
            if (nn_ids) sid[j] = mv ? dkey_slot(m) : ~0u;
            else if (sub == 0 && active) {  // rows form: lane 0 writes all five
                nn_pts[(size_t)q * 5 + j] = mv ? grid.pts[dkey_slot(m)] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            }
        }
        // Neighbour lists in IDS form (round 3): 20 bytes of map slots per point instead of 80 bytes of gathered rows -- the rows were the
        // path's only real HBM traffic (9.2 MB written here and re-read by the fit kernel every iteration); the fit kernel gathers
        // the five points from the (cache-resident) map image instead.  Bit 7 of the count byte says which form a point's list has
        // (0x80 = rows): a point without candidates keeps its previous list in whatever form it was (Q15); the lists are turned into
        // rows before anything moves map slots (matcher_p2plane_ivox.hpp::ensure_nn_rows).
        if (nn_ids) {
            if (sub == 0 && active) {
                *reinterpret_cast<uint4*>(nn_ids + (size_t)q * 8) = make_uint4(sid[0], sid[1], sid[2], sid[3]);
                nn_ids[(size_t)q * 8 + 4] = sid[4];
            }
            if (sub == 0 && active) nn_cnt[q] = (unsigned char)cnt;
        } else {
            if (sub == 0 && active) nn_cnt[q] = (unsigned char)(cnt | 0x80);
        }
    }
    if (COUNT) {
        const double p = wave_sum_u((double)c_probes), hsum = wave_sum_u((double)c_hits), c = wave_sum_u((double)c_cand);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&tc->probes, (unsigned long long)p);
            atomicAdd(&tc->hits, (unsigned long long)hsum);
            atomicAdd(&tc->cand, (unsigned long long)c);
        }
    }
}

template <bool COUNT, bool DENSE, bool FIRST, bool GEN>
__global__ void __launch_bounds__(256)
ivox_knn_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, const int n,
                const GnState* __restrict__ st, const Pose16 T0, const DevGrid grid, const BrickDir bd,
                const float inv_res, float4* __restrict__ nn_pts, unsigned char* __restrict__ nn_cnt,
                unsigned char* __restrict__ flag, TrafficCounters* __restrict__ tc, const int chunk,
                unsigned* __restrict__ nn_ids, const int nn_prev, float* __restrict__ dev_copy) {
    FLS_IVOX_KNN_SMEM_DECL;
    ivox_knn_body<COUNT, DENSE, FIRST, GEN>(FLS_IVOX_KNN_SMEM_ARGS, sx, sy, sz, n, st, T0, grid, bd, inv_res, nn_pts, nn_cnt, flag, tc, chunk, nn_ids, nn_prev, dev_copy);
}

// One Gauss-Newton iteration's two launches for a GROUP of independent registrations against one map (fls_match_batch_shared_ivox): grid
// (rows_max, jobs), blockIdx.y the job's entry in a device table (read through a uniform index: scalar loads), blockIdx.x the workgroup of
// that job's OWN grid.  Every job's kNN grid is ceil(n / 64) rounded up to a multiple of 8 * chunk, as the single-job launch's, so the XCD
// re-map of blockIdx.x stays a bijection per job; a workgroup past its job's grid leaves before anything else, a job that has stopped
// leaves where the single-job kernel does.  Per job: the scan, the Gauss-Newton state, the neighbour lists, flags and stored rows, the
// partial rows, ticket words and mailbox.  One for the group: the map image, its resolution and the thresholds.
// A pointer read from the job table is a generic pointer to the compiler: loads through it would be flat loads, and the Gauss-Newton state, which
// the single-job kernels (whose pointers are launch arguments) read with scalar loads, would arrive in vector registers -- 164 VGPRs instead of 128
// in the fit kernel, one wave per SIMD fewer.  Every table pointer is device memory; saying so (through an integer, or the round trip is folded
// away) gives the jobs kernels the single-job kernels' loads and registers.
template <class T>
__device__ __forceinline__ T* job_ptr(T* p) {
    typedef __attribute__((address_space(1))) T* global_ptr;
    return (T*)(global_ptr)(unsigned long long)p;
}
struct IvoxJob {
    const float *sx, *sy, *sz;  // the job's scan
    int n;                      // points
    int knn_blocks;             // workgroups of its kNN grid (a multiple of 8 * chunk)
    int nwg;                    // workgroups of its fit grid = partial rows
    int nn_prev;                // size of nearest_points_ before the Match
    GnState* st;
    float4* nn_pts;
    unsigned char* nn_cnt;
    unsigned char* flag;
    unsigned* nn_ids;
    double* Jst;
    double* partials;           // [nwg][kPartialStride]
    unsigned* ticket;           // kTicketWords words of the job's own, zero between launches
    Mailbox* mb;
    unsigned launch_word, pad;
    Pose16 T0;                  // the initial pose (read by the group's first launches)
};
template <bool DENSE, bool FIRST, bool GEN>
__global__ void __launch_bounds__(256)
ivox_knn_jobs_kernel(const IvoxJob* __restrict__ jobs, const DevGrid grid, const BrickDir bd, const float inv_res, const int chunk) {
    const IvoxJob& j = jobs[blockIdx.y];
    if ((int)blockIdx.x >= j.knn_blocks) return;
    FLS_IVOX_KNN_SMEM_DECL;
    ivox_knn_body<false, DENSE, FIRST, GEN>(FLS_IVOX_KNN_SMEM_ARGS, job_ptr(j.sx), job_ptr(j.sy), job_ptr(j.sz), j.n, (const GnState*)job_ptr(j.st), Pose16Ref{&j.T0},
                                            grid, bd, inv_res, job_ptr(j.nn_pts), job_ptr(j.nn_cnt), job_ptr(j.flag), (TrafficCounters*)nullptr, chunk,
                                            job_ptr(j.nn_ids), j.nn_prev, (float*)nullptr);
}
#undef FLS_IVOX_KNN_SMEM_PARAMS
#undef FLS_IVOX_KNN_SMEM_DECL
#undef FLS_IVOX_KNN_SMEM_ARGS

// ---------------------------------------------------------------------------------------------
// p2plane_fit_solve_kernel: fit + residual + block reduction (one lane per source point, reading what
// ivox_knn_kernel left behind), and the LAST workgroup to finish runs the Gauss-Newton
// tail (reduce the block partials, 6x6 solve, pose update, stop rule) -- one launch per iteration fewer.
// Cross-workgroup hand-off (placement independent, no spinning): every workgroup publishes its partial row with
// write-through (sc1) relaxed agent-scope stores, the storing wave drains (s_waitcnt vmcnt(0)), __syncthreads, one
// lane takes a ticket with an agent-scope atomic; the workgroup that draws the last ticket reads all rows with sc1
// (relaxed agent-scope) loads.  No release fence: an agent-scope release writes back the XCD's whole L2, which
// this kernel has just dirtied with 28 KB of Jacobian rows per workgroup (measured: 7 us on the critical path).
// The ticket counters (kTicketWords unsigned words) are reset by their last arrivers, so they are zero at every launch.
// A point's Jacobian row and flag go to memory AFTER the workgroup has handed its partial row over (in the workgroup that runs the tail: after
// the tail): __syncthreads() waits for every store a wave has issued, and 28 KB of rows per workgroup in front of the hand-off's barriers sat on
// the last workgroup's critical path (round 5: -0.3 us per launch here, -1.7 us per Match on a 5.8 k-point scan; same registers, same bits:
// profiles/r05_ll_ab_late_stores_x_fanin.log).  Nothing inside the launch reads them back.
// Where the time of the tail workgroup goes (profiles/r05_ll_fanin_stamps.log, -DFLS_TIMING, ~2.3 ticks per ns): its own fit 4.2 us, waiting for
// the slowest of its eight waves + row store + drain 3.2 us, two ticket levels 1.0 us, row read + reduction 1.6 us, LDL^T 1.45 us, pose update
// + state + mailbox 1.9 us.
// ---------------------------------------------------------------------------------------------
constexpr int kFitThreads = 512;
// The body of workgroup blockIdx.x of ONE registration whose fit grid has `nrows` workgroups: p2plane_fit_solve_kernel is that registration alone
// (nrows = LaunchBlocksX, the launch's gridDim.x), p2plane_fit_solve_jobs_kernel runs one per blockIdx.y (nrows = the job's own count).  The LDS
// is the calling kernel's, as in icp_knn_fit_body.
#if FLS_FIT_MFMA
#define FLS_P2P_FIT_SMEM_PARAMS LoamTailSmem& sm, double (&wsum)[NT / 64][32], unsigned& s_ticket, double (&mfma_tile)[NT / 64][512]
#define FLS_P2P_FIT_SMEM_DECL                                                      \
    __shared__ LoamTailSmem sm;                                                    \
    __shared__ double wsum[NT / 64][32];                                           \
    __shared__ unsigned s_ticket;                                                  \
    __shared__ __attribute__((aligned(64))) double mfma_tile[NT / 64][512]
#define FLS_P2P_FIT_SMEM_ARGS sm, wsum, s_ticket, mfma_tile
#else
#define FLS_P2P_FIT_SMEM_PARAMS LoamTailSmem& sm, double (&wsum)[NT / 64][32], unsigned& s_ticket
#define FLS_P2P_FIT_SMEM_DECL                                                      \
    __shared__ LoamTailSmem sm;                                                    \
    __shared__ double wsum[NT / 64][32];                                           \
    __shared__ unsigned s_ticket
#define FLS_P2P_FIT_SMEM_ARGS sm, wsum, s_ticket
#endif
template <bool FIRST, int NT, class N, class P>
__device__ __forceinline__ void
p2plane_fit_solve_body(FLS_P2P_FIT_SMEM_PARAMS, const N nrows, const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
                       const int n, GnState* __restrict__ st, const P& T0p /* Pose16, or Pose16Ref */, const float4* __restrict__ nn_pts,
                       const unsigned char* __restrict__ nn_cnt, double* __restrict__ Jst /* [7][n] */, unsigned char* __restrict__ flag,
                       double* __restrict__ partials, unsigned* __restrict__ ticket, Mailbox* __restrict__ mb, const unsigned match_id,
                       const double plane_thres, const double rot_thr, const double pos_thr, const int shards,
                       const unsigned* __restrict__ nn_ids /* may be null */, const float4* __restrict__ map_pts, const unsigned n_slots) {
    const Pose16& T0 = T0p;
    const int i = blockIdx.x * NT + threadIdx.x;
    const int done = FIRST ? 0 : st->done;
    double T44[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) T44[k] = FIRST ? T0.m[k] : st->T[k];
    const double last_rot = FIRST ? 0.0 : st->last_rot, last_pos = FIRST ? 0.0 : st->last_pos;
    const int it = FIRST ? 0 : st->iter;
    // every per-point input is loaded up front on a clamped index (one memory round trip; the neighbour points
    // are fetched whether or not all five exist, the stale flag whether or not it is needed)
    const int ii = i < n ? i : 0;
    const int cb = nn_cnt[ii];
    const int cnt = cb & 7;
    const float px = sx[ii], py = sy[ii], pz = sz[ii];
    const unsigned char stale = FIRST ? (unsigned char)0 : flag[ii];  // the first kNN launch of a Match cleared the flags
    float4 nn[5];
    // A neighbour's load stays where it is written, beside its address: left alone, the compiler merges the loads of the forms below into one load
    // of a merged address and moves it into the fit's block, away from the address arithmetic, where the three words of a point then take three
    // 64-bit addresses of their own (13 loads and 12 additions for 5 loads).  An empty statement that reads and writes the fetched words holds it.
    // (after the five loads of a form, so that they are in flight together; a point as the four registers its load fills, so that no word is moved)
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    auto hold = [&]() {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            f32x4 v = {nn[j].x, nn[j].y, nn[j].z, nn[j].w};
            asm volatile("" : "+v"(v));
            nn[j] = make_float4(v.x, v.y, v.z, v.w);
        }
    };
    if (nn_ids) {  // uniform: lists in ids form unless a point's count byte says rows (bit 7)
        const uint4 i4 = *reinterpret_cast<const uint4*>(nn_ids + (size_t)ii * 8);
        const unsigned i5 = nn_ids[(size_t)ii * 8 + 4];
        const unsigned sl[5] = {i4.x, i4.y, i4.z, i4.w, i5};
        const bool rows_form = (cb & 0x80) != 0;
        if (__ballot(rows_form) == 0ull) {  // the wave's lists are all ids (every wave of a Match that moves no map slot): no per-lane choice of address
#pragma unroll
            for (int j = 0; j < 5; ++j) nn[j] = map_pts[sl[j] < n_slots ? sl[j] : 0u];
            hold();
        } else {
#pragma unroll
            for (int j = 0; j < 5; ++j) nn[j] = *(rows_form ? nn_pts + (size_t)ii * 5 + j : map_pts + (sl[j] < n_slots ? sl[j] : 0u));
            hold();
        }
    } else {
#pragma unroll
        for (int j = 0; j < 5; ++j) nn[j] = nn_pts[(size_t)ii * 5 + j];
        hold();
    }
    if (done) return;
#ifdef FLS_TIMING
    const long long t_begin = (long long)__builtin_readcyclecounter();
#endif
    bool contrib = false, fresh = false;
    double J[6] = {0, 0, 0, 0, 0, 0}, res = 0.0;
    auto store_point = [&]() {  // (called once, after the hand-off)
        if (!fresh) return;
#pragma unroll
        for (int a = 0; a < 6; ++a) Jst[(size_t)a * n + i] = J[a];
        Jst[(size_t)6 * n + i] = res;
        flag[i] = 1;
    };
    {
        // One straight path through the fit for the whole wave: a lane past the scan's end or with a short list computes on what its clamped loads
        // brought and its result is dropped (nothing below traps, and no lane's arithmetic depends on another's); only a wave with no point to fit at all
        // -- the waves past the end of the last workgroup -- skips it.
        const bool want = i < n && cnt == 5;
        bool valid_now = false;
        if (__ballot(want) != 0ull) {
            const double x = px, y = py, z = pz;
            const float ptx = (float)(((T44[0] * x + T44[4] * y) + T44[8] * z) + T44[12]);
            const float pty = (float)(((T44[1] * x + T44[5] * y) + T44[9] * z) + T44[13]);
            const float ptz = (float)(((T44[2] * x + T44[6] * y) + T44[10] * z) + T44[14]);
            valid_now = plane_residual_dev(nn, px, py, pz, ptx, pty, ptz, T44, plane_thres, J, res) && want;
        }
        if (valid_now) {
            fresh = true;
            contrib = true;
        } else if (i < n && stale) {  // Q1: stale contribution of an earlier iteration
#pragma unroll
            for (int a = 0; a < 6; ++a) J[a] = Jst[(size_t)a * n + i];
            res = Jst[(size_t)6 * n + i];
            contrib = true;
        }
    }
#ifdef FLS_TIMING
    const long long t_fit = (long long)__builtin_readcyclecounter();
#endif
    // wave sums -> LDS -> one row per workgroup (fixed order: wave 0 + wave 1 + ...)
#if FLS_FIT_MFMA
    reduce_rank1_mfma_and_store(contrib, J, res, &wsum[threadIdx.x >> 6][0], &mfma_tile[threadIdx.x >> 6][0]);
#else
    reduce_rank1_and_store(contrib, J, res, &wsum[threadIdx.x >> 6][0]);
#endif
#ifdef FLS_TIMING
    const long long t_red = (long long)__builtin_readcyclecounter();
#endif
    __syncthreads();
    if (threadIdx.x < 29) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) v += wsum[w][threadIdx.x];
        // write-through (sc1) publish: visible to every XCD once this wave's stores have drained -- no L2 write-back
        __hip_atomic_store((unsigned long long*)partials + (size_t)blockIdx.x * kPartialStride + threadIdx.x,
                           (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains before the ticket
#ifdef FLS_TIMING
    const long long t_drain = (long long)__builtin_readcyclecounter();
#endif
    __syncthreads();
    // sharded fan-in (kernels_p2plane.hpp::fanin_last_arriver): which workgroup arrives last
    if (threadIdx.x == 0) s_ticket = fanin_last_arriver(ticket, shards, nrows);
    __syncthreads();
    if (!s_ticket) { store_point(); return; }
    // ---- last workgroup: Gauss-Newton tail (reads the rows with sc1 loads: no acquire fence either) ----
#ifdef FLS_TIMING
    if (threadIdx.x == 0) { st->dbg[0] = t_begin; st->dbg[13] = t_fit; st->dbg[14] = t_red; st->dbg[15] = t_drain; }
#endif
    FLS_STAMP(1);
    loam_tail<NT, true>(st, sm, nullptr, 0, partials, (int)(unsigned)nrows, rot_thr, pos_thr, T44, last_rot, last_pos, it, mb, match_id);
    store_point();  // (every thread comes back from the tail: waves 1.. at once, wave 0 after it has published)
}

template <bool FIRST, int NT = kFitThreads>
__global__ void __launch_bounds__(NT)
p2plane_fit_solve_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, const int n,
                         GnState* __restrict__ st, const Pose16 T0, const float4* __restrict__ nn_pts,
                         const unsigned char* __restrict__ nn_cnt, double* __restrict__ Jst, unsigned char* __restrict__ flag,
                         double* __restrict__ partials, unsigned* __restrict__ ticket, Mailbox* __restrict__ mb, const unsigned match_id,
                         const double plane_thres, const double rot_thr, const double pos_thr, const int shards,
                         const unsigned* __restrict__ nn_ids, const float4* __restrict__ map_pts, const unsigned n_slots) {
    FLS_P2P_FIT_SMEM_DECL;
    p2plane_fit_solve_body<FIRST, NT>(FLS_P2P_FIT_SMEM_ARGS, LaunchBlocksX{}, sx, sy, sz, n, st, T0, nn_pts, nn_cnt, Jst, flag, partials, ticket, mb, match_id,
                                      plane_thres, rot_thr, pos_thr, shards, nn_ids, map_pts, n_slots);
}

// The fit launch of a group (IvoxJob above): the jobs of ONE workgroup size -- NT is per job what the single-job path chooses, because another NT
// regroups the wave sums -- as the rows of one grid (nwg_max, jobs).  A workgroup past its job's rows leaves before any barrier, row store or
// ticket; the fan-in and the tail count the job's own nwg, so the job's rows, their order in the sum and the ticket protocol are the single-job
// launch's, and the last arriver OF THE JOB solves and publishes the job's mailbox beside the other jobs' fits.
template <bool FIRST, int NT>
__global__ void __launch_bounds__(NT)
p2plane_fit_solve_jobs_kernel(const IvoxJob* __restrict__ jobs, const double plane_thres, const double rot_thr, const double pos_thr, const int shards,
                              const float4* __restrict__ map_pts, const unsigned n_slots) {
    const IvoxJob& j = jobs[blockIdx.y];
    if ((int)blockIdx.x >= j.nwg) return;
    FLS_P2P_FIT_SMEM_DECL;
    p2plane_fit_solve_body<FIRST, NT>(FLS_P2P_FIT_SMEM_ARGS, (unsigned)j.nwg, job_ptr(j.sx), job_ptr(j.sy), job_ptr(j.sz), j.n, job_ptr(j.st), Pose16Ref{&j.T0},
                                      (const float4*)job_ptr(j.nn_pts), (const unsigned char*)job_ptr(j.nn_cnt), job_ptr(j.Jst), job_ptr(j.flag),
                                      job_ptr(j.partials), job_ptr(j.ticket), job_ptr(j.mb), j.launch_word, plane_thres, rot_thr, pos_thr, shards,
                                      (const unsigned*)job_ptr(j.nn_ids), map_pts, n_slots);
}
#undef FLS_P2P_FIT_SMEM_PARAMS
#undef FLS_P2P_FIT_SMEM_DECL
#undef FLS_P2P_FIT_SMEM_ARGS

// ---------------------------------------------------------------------------------------------
// Map maintenance on the device
//   ivox_apply_updates_kernel   scatter {slot, point} and {cell, begin, count} records into the resident image
//   ivox_add_decide_kernel      the per-point down-sampling decision of LoamPointToPlaneIVOX::AddCloudToLocalMap
//                               (loam_point_to_plane_ivox.h:89-128) on the neighbour lists left by the last
//                               PlanerMatch: code 0 = drop, 1 = points_to_add, 2 = point_no_need_downsample;
//                               pw = pcl::transformPoint(p, T_) (double -> float)
// ---------------------------------------------------------------------------------------------
struct PtUpdDev { unsigned slot; float x, y, z; int id; };
struct CellUpdDev { unsigned long long idx; unsigned begin, count; };

// An image that arrived from another process (fls_map_image_import): every {begin, count} must stay inside the point array and every
// directory entry must name a brick the image holds, or a query kernel would read out of bounds.  bad = number of offending entries.
__global__ void __launch_bounds__(256)
ivox_image_validate_kernel(const uint2* __restrict__ cells, const unsigned long long n_cells, const HashEntry* __restrict__ dir, const unsigned long long n_dir,
                           const unsigned n_bricks_live, const HashEntry* __restrict__ table, const unsigned long long n_table, const unsigned long long used,
                           unsigned* __restrict__ bad) {
    unsigned b = 0u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n_cells; i += stride) {
        const uint2 c = cells[i];
        b += ((unsigned long long)c.x + (unsigned long long)c.y > used) ? 1u : 0u;
    }
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n_dir; i += stride) {
        const HashEntry e = dir[i];
        b += (e.key != kEmptyKey && e.begin >= n_bricks_live) ? 1u : 0u;
    }
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n_table; i += stride) {
        const HashEntry e = table[i];
        b += (e.key != kEmptyKey && (unsigned long long)e.begin + (unsigned long long)e.count > used) ? 1u : 0u;
    }
    if (b) atomicAdd(bad, b);
}

__global__ void __launch_bounds__(256)
ivox_apply_updates_kernel(const PtUpdDev* __restrict__ pu, const int npu, const CellUpdDev* __restrict__ cu, const int ncu,
                          float4* __restrict__ pts, uint2* __restrict__ cells) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < npu) {
        const PtUpdDev u = pu[i];
        pts[u.slot] = make_float4(u.x, u.y, u.z, __int_as_float(u.id));
    }
    if (i < ncu) {
        const CellUpdDev u = cu[i];
        cells[u.idx] = make_uint2(u.begin, u.count);
    }
}

// neighbour lists: ids form -> rows form (before map slots move, and for the host-side readers)
__global__ void __launch_bounds__(256)
ivox_nn_materialize_kernel(const unsigned* __restrict__ nn_ids, unsigned char* __restrict__ nn_cnt, const int n, const float4* __restrict__ map_pts,
                           const unsigned n_slots, float4* __restrict__ nn_pts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned char cb = nn_cnt[i];
    if (cb & 0x80) return;
    if (cb & 7) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const unsigned sl = nn_ids[(size_t)i * 8 + j];
            nn_pts[(size_t)i * 5 + j] = sl < n_slots ? map_pts[sl] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        }
    }
    nn_cnt[i] = (unsigned char)(cb | 0x80);
}

// MATERIALIZE (round 3): the launch also turns the ids-form lists into rows (what ivox_nn_materialize_kernel does) -- the map update that
// follows moves slots, and this kernel gathers the same five points anyway: one launch and one gather less per mapping-mode scan.
// The grid then covers max(n, nn_n) points (lists beyond the points that are decided on still become rows).
// COUNT (round 4): the launch also does what ivox_upd_count did -- block-local exclusive counts of the two insertion codes (lx) and the
// block totals (bt) for the device-side AddPoints -- and resets the batch status words: one dependent launch less in front of the update.
template <bool MATERIALIZE>
__global__ void __launch_bounds__(256)
ivox_add_decide_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, const int n,
                       const Pose16 Tw, float4* __restrict__ nn_pts, unsigned char* __restrict__ nn_cnt, const int nn_n,
                       const double fs /* filter_size_map_min */, unsigned char* __restrict__ code, float4* __restrict__ pw_out,
                       const unsigned* __restrict__ nn_ids /* may be null */, const float4* __restrict__ map_pts, const unsigned n_slots,
                       uint2* __restrict__ lx /* may be null: no counting */, uint2* __restrict__ bt, unsigned* __restrict__ st_status,
                       unsigned* __restrict__ st_apply, const GnState* __restrict__ gn /* non-null: SPECULATIVE launch, see below */, const int max_it) {
    // SPECULATIVE form (round 4): the host queues the decision + update chain right behind the iterations it expects the Match to need,
    // without waiting for the result (14 us of mailbox turnaround + launch latency in front of the map update).  The launch then decides
    // ON THE DEVICE whether LoamPointToPlaneIVOX::Match would reach AddCloudToLocalMap here (:197-206): the Gauss-Newton loop has ended
    // (stop rule or max_iterations) and n_valid >= 50.  If not, the whole chain marks itself skipped (kUpdSkipped = 16) and does nothing;
    // the host queues another chain behind the iterations it adds.  The pose is the device's (GnState::T), not a launch argument.
    Pose16 Tl = Tw;
    if (gn != nullptr) {
        const bool go = (gn->done != 0 || gn->iter >= max_it) && gn->n_valid >= 50;
        if (!go) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { *st_status = 16u; *st_apply = 0u; }
            return;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) Tl.m[q] = gn->T[q];
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned char c = 0;  // this point's code (0 also for the threads beyond n)
    if (i < n || (MATERIALIZE && i < nn_n)) {
        const int cb = i < nn_n ? nn_cnt[i] : 0;
        const int cnt = cb & 7;
        const bool ids_form = nn_ids != nullptr && !(cb & 0x80);
        float4 nb[5];
        if (MATERIALIZE) {
            // all five rows now (whatever the decision below needs), written back in rows form
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                if (ids_form) {
                    const unsigned sl = nn_ids[(size_t)i * 8 + k];
                    nb[k] = (cnt && sl < n_slots) ? map_pts[sl] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
                } else {
                    nb[k] = (i < nn_n && cnt) ? nn_pts[(size_t)i * 5 + k] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
                }
            }
            if (i < nn_n && ids_form) {
                if (cnt) {
#pragma unroll
                    for (int k = 0; k < 5; ++k) nn_pts[(size_t)i * 5 + k] = nb[k];
                }
                nn_cnt[i] = (unsigned char)(cb | 0x80);
            }
        }
        if (i < n) {
            const double x = sx[i], y = sy[i], z = sz[i];
            const float wx = (float)(((Tl.m[0] * x + Tl.m[4] * y) + Tl.m[8] * z) + Tl.m[12]);
            const float wy = (float)(((Tl.m[1] * x + Tl.m[5] * y) + Tl.m[9] * z) + Tl.m[13]);
            const float wz = (float)(((Tl.m[2] * x + Tl.m[6] * y) + Tl.m[10] * z) + Tl.m[14]);
            pw_out[i] = make_float4(wx, wy, wz, 0.f);
            auto neighbour = [&](const int k) -> float4 {
                if (MATERIALIZE) return nb[k];
                if (!ids_form) return nn_pts[(size_t)i * 5 + k];
                const unsigned sl = nn_ids[(size_t)i * 8 + k];
                return map_pts[sl < n_slots ? sl : 0u];
            };
            c = 1;  // no neighbours: add (:126)
            if (cnt > 0) {
                const double half = 0.5 * fs;
                const double c0 = (floor((double)wx / fs) + 0.5) * fs, c1 = (floor((double)wy / fs) + 0.5) * fs, c2 = (floor((double)wz / fs) + 0.5) * fs;
                const float4 n0 = neighbour(0);
                const double d0 = (double)n0.x - c0, d1 = (double)n0.y - c1, d2 = (double)n0.z - c2;
                if (fabs(d0) > half && fabs(d1) > half && fabs(d2) > half) {
                    c = 2;  // :103-108
                } else {
                    const double e0 = (double)wx - c0, e1 = (double)wy - c1, e2 = (double)wz - c2;
                    const double dist = (e0 * e0 + e1 * e1) + e2 * e2;
                    bool need_add = true;
                    if (cnt >= 5) {
#pragma unroll
                        for (int k = 0; k < 5; ++k) {
                            if (!need_add) break;
                            const float4 q = neighbour(k);
                            const double f0 = (double)q.x - c0, f1 = (double)q.y - c1, f2 = (double)q.z - c2;
                            if ((f0 * f0 + f1 * f1) + f2 * f2 < dist + 1.0e-6) need_add = false;
                        }
                    }
                    c = need_add ? 1 : 0;
                }
            }
            code[i] = c;
        }
    }
    if (lx != nullptr) {  // (uniform)
        __shared__ unsigned wsum[256 / 64][2];
        unsigned v[2] = {c == 1 ? 1u : 0u, c == 2 ? 1u : 0u}, tot[2];
        block_excl_scan<2>(v, tot, wsum);
        if (i < n) lx[i] = make_uint2(v[0], v[1]);
        if (threadIdx.x == 0 && blockIdx.x * 256 < n) bt[blockIdx.x] = make_uint2(tot[0], tot[1]);
        if (threadIdx.x == 0 && blockIdx.x == 0) { *st_status = 0u; *st_apply = 0u; }  // kUpdOk; the batch's verdict is open
    }
}

}  // namespace fls
