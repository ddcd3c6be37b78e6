// fls_hip_keyframes.h -- header-only C++ adapter of include/fls_keyframes.h for the places where the reference assembles a map from
// its keyframes: LoopClosure::GetSubMap (src/slam/loop_closure.cpp:179-231), the loop of System::SaveMap
// (src/slam/system.cpp:310-316) and of the global-map publisher (:884-892).  The keyframes' ordered clouds live in device memory from
// Add() on -- KeyFrame::LoadOrderedCloud and its PCD read per keyframe and sub-map go away --, VoxelGridCloud(keyframe, leaf) runs
// once per keyframe and leaf, and a sub-map is one launch.
// The store keeps no poses: every call takes the keyframes' current poses (they move with every pose-graph optimisation).
// ref_pose.inverse() * pose is evaluated HERE, with the caller's Mat4d: in the reference's tree that is Eigen's own inverse and
// product, exactly as loop_closure.cpp:211-214 evaluates them.
// Templates over the cloud and pose types; needs only fls_keyframes.h (no Eigen, no PCL).  A pose type offers data() (16 doubles,
// column-major), inverse() and operator* (Eigen::Matrix4d).
#pragma once
#include "fls_hip_preprocess.h"
#include "fls_keyframes.h"
#include "fls_loop_device.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

namespace fls_hip {

class HipKeyframeStore {
public:
    // the keyframes a sub-map is made of and the pose each is placed with (column-major, 16 doubles each)
    struct Selection {
        std::vector<int32_t> ids;
        std::vector<double> poses;
        template <class Mat4>
        void push(int32_t id, const Mat4& pose) {
            ids.push_back(id);
            poses.insert(poses.end(), pose.data(), pose.data() + 16);
        }
    };

    explicit HipKeyframeStore(int device = 0) {
        const fls_status rc = fls_keyframes_create(device, &h_);
        if (rc != FLS_OK) {
            std::fprintf(stderr, "HipKeyframeStore: fls_keyframes_create failed: %s\n", fls_status_string(rc));
            std::abort();
        }
    }
    ~HipKeyframeStore() { fls_keyframes_destroy(h_); }
    HipKeyframeStore(const HipKeyframeStore&) = delete;
    HipKeyframeStore& operator=(const HipKeyframeStore&) = delete;

    // where the reference saves the keyframe's ordered cloud: returns KeyFrame::ID-like 0, 1, 2, ...; -1: failed
    template <class Cloud>
    int32_t Add(const Cloud& ordered_cloud) {
        using P = typename std::remove_const<typename std::remove_reference<decltype(ordered_cloud.points[0])>::type>::type;
        static_assert(sizeof(P) % sizeof(float) == 0, "point rows of whole floats");
        int32_t id = -1;
        const float* rows = ordered_cloud.points.empty() ? nullptr : &ordered_cloud.points[0].x;
        return Check(fls_keyframes_add(h_, rows, ordered_cloud.points.size(), int(sizeof(P) / sizeof(float)), &id), "Add") ? id : -1;
    }
    // the ordered cloud of the scan `pre` has just run (Run / RunOnDevice), device to device
    int32_t Add(HipScanPreprocessor& pre) {
        int32_t id = -1;
        return Check(fls_keyframes_add_preprocessed(h_, pre.handle(), FLS_PRE_ORDERED, &id), "Add(preprocessor)") ? id : -1;
    }
    size_t size() const { return fls_keyframes_count(h_); }

    // loop_closure.cpp:186-215: the keyframes of [keyframe_id - left_range, keyframe_id + right_range] that exist, each with its pose,
    // or with ref_pose.inverse() * pose when use_local_pose
    template <class Mat4>
    Selection Select(int32_t keyframe_id, int32_t left_range, int32_t right_range, bool use_local_pose, const std::vector<Mat4>& keyframe_poses) const {
        Selection s;
        std::vector<Mat4> poses;
        const Mat4 ref_pose = keyframe_poses[static_cast<size_t>(keyframe_id)];
        for (int i = -left_range; i <= right_range; ++i) {
            const int32_t keyframe_id_temp = keyframe_id + i;
            if (keyframe_id_temp < 0 || keyframe_id_temp >= static_cast<int32_t>(keyframe_poses.size())) {
                continue;
            }
            s.ids.push_back(keyframe_id_temp);
            poses.push_back(keyframe_poses[static_cast<size_t>(keyframe_id_temp)]);
        }
        if (use_local_pose) {
            const Mat4 ref_pose_inv = ref_pose.inverse();
            for (auto& pose : poses) {
                pose = ref_pose_inv * pose;
            }
        }
        for (const auto& pose : poses) s.poses.insert(s.poses.end(), pose.data(), pose.data() + 16);
        return s;
    }

    // LoopClosure::GetSubMap(keyframe_id, left_range, right_range, use_local_pose): every keyframe VoxelGrid-ed at 0.2, transformed, appended
    template <class Cloud, class Mat4>
    void GetSubMap(Cloud& out, int32_t keyframe_id, int32_t left_range, int32_t right_range, bool use_local_pose,
                   const std::vector<Mat4>& keyframe_poses) {
        Merge(out, Select(keyframe_id, left_range, right_range, use_local_pose, keyframe_poses), 0.2f, 0.f);
    }
    // SaveMap's loop over all keyframes (system.cpp:310-316: leaf, then leaf again on the merged cloud); the publisher's loop
    // (:884-892) is MergeMap(out, poses, 0.3f, 0.f)
    template <class Cloud, class Mat4>
    void MergeMap(Cloud& out, const std::vector<Mat4>& keyframe_poses, float leaf = 0.3f, float leaf_final = 0.3f) {
        Selection s;
        for (size_t k = 0; k < keyframe_poses.size(); ++k) s.push(static_cast<int32_t>(k), keyframe_poses[k]);
        Merge(out, s, leaf, leaf_final);
    }
    template <class Cloud>
    void Merge(Cloud& out, const Selection& s, float leaf_each, float leaf_final) {
        size_t n = 0, cap = 0;
        for (int32_t id : s.ids) {  // no result is longer than the stored clouds
            size_t m = 0;
            (void)fls_keyframes_get(h_, id, 0.f, nullptr, 0, &m);
            cap += m;
        }
        rows_.resize(4 * cap);
        if (!Check(fls_keyframes_merge(h_, s.ids.data(), s.poses.data(), s.ids.size(), leaf_each, leaf_final, rows_.data(), cap, &n), "Merge")) n = 0;
        out.points.resize(n);
        for (size_t k = 0; k < n; ++k) {
            auto& p = out.points[k];
            p.x = rows_[4 * k];
            p.y = rows_[4 * k + 1];
            p.z = rows_[4 * k + 2];
            p.intensity = rows_[4 * k + 3];
        }
    }

    // loop_closure.cpp:75-86: GetSubMap for the source (the loop-closure keyframe, local poses) and the target (the candidate), then
    // LoopClosure::Match(source, target, pose); returns the fitness score
    template <class Mat4>
    float Match(const Selection& source, const Selection& target, Mat4& pose, fls_loop_stats* stats = nullptr) {
        float fitness = std::numeric_limits<float>::max();
        (void)Check(fls_keyframes_loop_match(h_, source.ids.data(), source.poses.data(), source.ids.size(), target.ids.data(), target.poses.data(),
                                             target.ids.size(), pose.data(), &fitness, stats), "Match");
        return fitness;
    }

    // The same with both sub-maps left on the device and the Match started from them there (include/fls_loop_device.h): the same pose,
    // fitness and stats, bit for bit, without the two downloads, the ten host filters and the host leaf builds
    template <class Mat4>
    float LoopMatchOnDevice(const Selection& source, const Selection& target, Mat4& pose, fls_loop_stats* stats = nullptr) {
        float fitness = std::numeric_limits<float>::max();
        (void)Check(fls_keyframes_loop_match_device(h_, source.ids.data(), source.poses.data(), source.ids.size(), target.ids.data(), target.poses.data(),
                                                    target.ids.size(), pose.data(), &fitness, stats), "LoopMatchOnDevice");
        return fitness;
    }

    size_t stat(int slot) const { return fls_keyframes_stat(h_, slot); }
    fls_keyframes_handle handle() const { return h_; }

private:
    static bool Check(fls_status rc, const char* where) {
        if (rc == FLS_OK) return true;
        std::fprintf(stderr, "HipKeyframeStore::%s: %s\n", where, fls_status_string(rc));
        return false;
    }
    fls_keyframes_handle h_ = nullptr;
    std::vector<float> rows_;
};

}  // namespace fls_hip
