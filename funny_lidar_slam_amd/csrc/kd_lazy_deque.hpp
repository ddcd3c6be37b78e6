// kd_lazy_deque.hpp -- the bookkeeping of the kd-tree kinds' host deque once a keyframe can be pushed on the device (kernels_kd_push.hpp):
// the LOGICAL deque is what the reference's deque of clouds would be; the DeviceCloudRing (kd_map.hpp) holds all of it whenever
// the handle is on the device path, the host holds a subset of whole clouds.  A cloud pushed on the device has no host copy until something
// reads the host deque (a rebuild the device declined, an export through the host); what is missing is then copied out of the ring's four
// planes, run by run, and is bit for bit what a host push would have stored.  This header knows which clouds are present, which ring floats
// a fetch must copy, and what trim / reset / import do to that; it makes no HIP call (tests/host/kd_push_model_test.cpp runs it with host
// arrays standing in for the ring).
#pragma once
#include "kd_image.hpp"
#include <cstring>
#include <deque>
#include <vector>

namespace fls {

struct KdLazyDeque {
    KdDeque clouds;                    // clouds[k]: the host copy of cloud k if have[k], empty otherwise
    std::deque<unsigned char> have;
    std::deque<size_t> sizes;          // points of every cloud, present or not (== DeviceCloudRing::sizes on the device path)
    size_t n_missing = 0;

    size_t size() const { return sizes.size(); }
    size_t points() const { size_t n = 0; for (const size_t s : sizes) n += s; return n; }
    bool complete() const { return n_missing == 0; }

    void push_host(const std::vector<PtI>& cloud) {
        clouds.push_back(cloud);
        have.push_back(1);
        sizes.push_back(cloud.size());
    }
    // a cloud of n points that exists in the ring alone
    void push_device(const size_t n) {
        clouds.emplace_back();
        have.push_back(0);
        sizes.push_back(n);
        ++n_missing;
    }
    void pop_front() {  // whether or not the cloud was ever fetched
        if (sizes.empty()) return;
        if (!have.front()) --n_missing;
        clouds.pop_front();
        have.pop_front();
        sizes.pop_front();
    }
    // the reference's `if (deque.size() > max) deque.pop_front()`; true: a cloud left
    bool trim(const size_t max_clouds) {
        if (sizes.size() <= max_clouds) return false;
        pop_front();
        return true;
    }
    void clear() {
        clouds.clear();
        have.clear();
        sizes.clear();
        n_missing = 0;
    }
    // an import: everything present on the host
    void assign(KdDeque&& all) {
        clear();
        clouds = std::move(all);
        for (const auto& c : clouds) { have.push_back(1); sizes.push_back(c.size()); }
    }

    // A maximal run of consecutive missing clouds: clouds first .. first + n_clouds, ring floats offset .. offset + n_points of every plane,
    // counted from the ring's head (the deque's first cloud starts there, the clouds lie back to back)
    struct Run { size_t first = 0, n_clouds = 0, offset = 0, n_points = 0; };
    std::vector<Run> missing_runs() const {
        std::vector<Run> runs;
        size_t at = 0;
        for (size_t k = 0; k < sizes.size(); ++k) {
            if (!have[k]) {
                if (!runs.empty() && runs.back().first + runs.back().n_clouds == k) { ++runs.back().n_clouds; runs.back().n_points += sizes[k]; }
                else runs.push_back(Run{k, 1, at, sizes[k]});
            }
            at += sizes[k];
        }
        return runs;
    }
    // the planes of one run (r.n_points floats each, as 32-bit words: the rows carry NaN payloads) become the host copies of its clouds
    void fill(const Run& r, const unsigned* x, const unsigned* y, const unsigned* z, const unsigned* in) {
        size_t at = 0;
        for (size_t k = r.first; k < r.first + r.n_clouds; ++k) {
            std::vector<PtI>& c = clouds[k];
            c.resize(sizes[k]);
            for (size_t j = 0; j < sizes[k]; ++j) {
                const unsigned row[4] = {x[at + j], y[at + j], z[at + j], in[at + j]};
                std::memcpy(static_cast<void*>(&c[j]), row, sizeof(PtI));
            }
            at += sizes[k];
            if (!have[k]) { have[k] = 1; --n_missing; }
        }
    }
};

}  // namespace fls
