// fls_hip_preprocess.h -- header-only C++ adapter of include/fls_preprocess.h for the non-LOAM branch of PreProcessing::Run()
// (src/slam/preprocessing.cpp:86-223): from the raw PointXYZIRT cloud, its header stamp and the IMU
// samples, fill a PointcloudCluster's ordered_cloud_ and planar_cloud_ (VoxelGrid-filtered when a leaf size is set) with the points
// de-skewed on the device.  The caller keeps the queue logic of Run(): Run() below returns what the reference would do.
// Templates over the cluster / cloud / IMU types; needs only fls_preprocess.h (no Eigen, no PCL).  IMU samples expose timestamp_ (us)
// and orientation_.x() .y() .z() .w() (IMUData with an Eigen::Quaterniond).
// RunDriver / RunDriverOnDevice take the driver message's bytes and an fls_driver_cloud instead of a
// converted cloud: they replace ConvertMessageToCloud as well.
#pragma once
#include "fls_ingest.h"

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace fls_hip {

class HipScanPreprocessor {
public:
    // T_lidar_to_imu: Mat4d::data() (column-major)
    HipScanPreprocessor(float min_distance, float max_distance, int lidar_point_jump_span, float planar_voxel_filter_size, const double* T_lidar_to_imu,
                        int device = 0) {
        fls_preprocess_params p{};
        p.struct_size = sizeof(p);
        p.lidar_point_jump_span = lidar_point_jump_span;
        p.min_distance = min_distance;
        p.max_distance = max_distance;
        p.planar_voxel_filter_size = planar_voxel_filter_size;
        for (int k = 0; k < 16; ++k) p.T_lidar_to_imu[k] = T_lidar_to_imu[k];
        leaf_ = planar_voxel_filter_size;
        const fls_status rc = fls_preprocess_create(&p, device, &h_);
        if (rc != FLS_OK) {
            std::fprintf(stderr, "HipScanPreprocessor: fls_preprocess_create failed: %s\n", fls_status_string(rc));
            std::abort();
        }
    }
    ~HipScanPreprocessor() { fls_preprocess_destroy(h_); }
    HipScanPreprocessor(const HipScanPreprocessor&) = delete;
    HipScanPreprocessor& operator=(const HipScanPreprocessor&) = delete;

    // FLS_IMU_OK / FLS_IMU_EMPTY_SEGMENT / FLS_IMU_EMPTY_CLOUD: the clouds are filled (possibly empty); FLS_IMU_DROP: drop the raw cloud;
    // FLS_IMU_WAIT: keep it and retry when more IMU data has arrived; -1: invalid input (the reference would CHECK-abort)
    template <class Cluster, class RawCloud, class ImuVec>
    int Run(Cluster& c, const RawCloud& raw, uint64_t stamp_us, const ImuVec& imu) {
        const int st = Scan(raw, stamp_us, imu, /*on_device=*/false);
        if (st >= 0 && st != FLS_IMU_DROP && st != FLS_IMU_WAIT) FillCluster(c);
        return st;
    }
    // Run() with the clouds left in device memory for HipRegistration::MatchPreprocessed (fls_hip_registration.h): no cluster is
    // filled, the host learns the counts only.  Same return values.
    template <class RawCloud, class ImuVec>
    int RunOnDevice(uint64_t stamp_us, const RawCloud& raw, const ImuVec& imu) {
        return Scan(raw, stamp_us, imu, /*on_device=*/true);
    }
    // Run() / RunOnDevice() from the driver message itself (sensor_msgs::PointCloud2: data.data(), width * height, and a descriptor
    // made from point_step, is_dense and the offsets of the message's fields): ConvertMessageToCloud runs on the device.
    // *stamp_out_us: the header stamp the reference goes on with (RoboSense: the first kept point's time).
    template <class Cluster, class ImuVec>
    int RunDriver(Cluster& c, const void* msg_points, size_t n, const fls_driver_cloud& cloud, const fls_ingest_params& ingest, uint64_t stamp_us,
                  const ImuVec& imu, uint64_t* stamp_out_us = nullptr) {
        const int st = ScanDriver(msg_points, n, cloud, ingest, stamp_us, imu, /*on_device=*/false, stamp_out_us);
        if (st >= 0 && st != FLS_IMU_DROP && st != FLS_IMU_WAIT) FillCluster(c);
        return st;
    }
    template <class ImuVec>
    int RunDriverOnDevice(const void* msg_points, size_t n, const fls_driver_cloud& cloud, const fls_ingest_params& ingest, uint64_t stamp_us,
                          const ImuVec& imu, uint64_t* stamp_out_us = nullptr) {
        return ScanDriver(msg_points, n, cloud, ingest, stamp_us, imu, /*on_device=*/true, stamp_out_us);
    }
    const fls_ingest_info& last_ingest() const { return info_; }
    // the PCL clouds of the last scan, for callers that still need them on the host (visualisation, keyframes): after RunOnDevice
    // each cloud is downloaded here, on its first request
    template <class Cluster>
    void FillCluster(Cluster& c) {
        FetchCloud(FLS_PRE_ORDERED, c.ordered_cloud_);
        FetchCloud(planar_what(), c.planar_cloud_);
    }
    fls_preprocess_handle handle() const { return h_; }
    // the array PreProcessing::Run() puts into planar_cloud_: filtered when a leaf size is set
    int planar_what() const { return leaf_ > 0.f ? FLS_PRE_PLANAR_FILTERED : FLS_PRE_PLANAR; }
    const fls_preprocess_result& last_result() const { return r_; }

private:
    template <class ImuVec>
    void PackImu(const ImuVec& imu) {
        t_.resize(imu.size());
        q_.resize(4 * imu.size());
        for (size_t k = 0; k < imu.size(); ++k) {
            t_[k] = imu[k].timestamp_;
            q_[4 * k] = imu[k].orientation_.x();
            q_[4 * k + 1] = imu[k].orientation_.y();
            q_[4 * k + 2] = imu[k].orientation_.z();
            q_[4 * k + 3] = imu[k].orientation_.w();
        }
    }
    template <class ImuVec>
    int ScanDriver(const void* msg, size_t n, const fls_driver_cloud& cloud, const fls_ingest_params& ingest, uint64_t stamp_us, const ImuVec& imu,
                   bool on_device, uint64_t* stamp_out_us) {
        PackImu(imu);
        r_ = fls_preprocess_result{};
        r_.struct_size = sizeof(r_);
        info_ = fls_ingest_info{};
        info_.struct_size = sizeof(info_);
        const fls_status rc = fls_preprocess_scan_driver(h_, msg, n, &cloud, &ingest, stamp_us, t_.data(), q_.data(), t_.size(), on_device ? 1 : 0, &r_,
                                                         stamp_out_us, &info_);
        if (rc != FLS_OK && rc != FLS_ERR_STATE) { std::fprintf(stderr, "HipScanPreprocessor::RunDriver: %s\n", fls_status_string(rc)); return -1; }
        return r_.imu_status;
    }
    template <class RawCloud, class ImuVec>
    int Scan(const RawCloud& raw, uint64_t stamp_us, const ImuVec& imu, bool on_device) {
        using P = typename std::remove_const<typename std::remove_reference<decltype(raw.points[0])>::type>::type;
        static const fls_raw_layout lay{static_cast<uint32_t>(sizeof(P)), static_cast<uint32_t>(offsetof(P, x)), static_cast<uint32_t>(offsetof(P, intensity)),
                                        static_cast<uint32_t>(offsetof(P, ring)), static_cast<uint32_t>(sizeof(P::ring)),
                                        static_cast<uint32_t>(offsetof(P, time))};
        PackImu(imu);
        r_ = fls_preprocess_result{};
        r_.struct_size = sizeof(r_);
        const fls_status rc = (on_device ? fls_preprocess_scan_device : fls_preprocess_scan)(h_, raw.points.data(), raw.points.size(), &lay, stamp_us,
                                                                                            t_.data(), q_.data(), t_.size(), &r_);
        if (rc != FLS_OK && rc != FLS_ERR_STATE) { std::fprintf(stderr, "HipScanPreprocessor::Run: %s\n", fls_status_string(rc)); return -1; }
        return r_.imu_status;
    }
    template <class Cloud>
    void FetchCloud(int what, Cloud& out) {
        const size_t n = fls_preprocess_get(h_, what, nullptr, 0);
        rows_.resize(4 * n);
        fls_preprocess_get(h_, what, rows_.data(), n);
        out.points.resize(n);
        for (size_t k = 0; k < n; ++k) {
            auto& p = out.points[k];
            p.x = rows_[4 * k];
            p.y = rows_[4 * k + 1];
            p.z = rows_[4 * k + 2];
            p.intensity = rows_[4 * k + 3];
        }
    }
    fls_preprocess_handle h_ = nullptr;
    float leaf_ = 0.f;
    fls_preprocess_result r_{};
    fls_ingest_info info_{};
    std::vector<uint64_t> t_;
    std::vector<double> q_;
    std::vector<float> rows_;
};

}  // namespace fls_hip
