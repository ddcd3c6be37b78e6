// Stand-ins for the reference's types the preprocessing adapter reads (tests only): PointXYZIRT (lidar_point_type.h:121-136),
// pcl::PointXYZI / PointCloud, IMUData with an xyzw quaternion, and the two PointcloudCluster clouds.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct PointXYZIRT {
    float x, y, z, pad;
    float intensity;
    std::uint8_t ring;
    float time;
};
struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };
template <class T>
struct PointCloud {
    std::vector<T> points;
    std::size_t size() const { return points.size(); }
};
struct QuaternionStub {
    double c[4];  // x, y, z, w (Eigen's coeffs() order)
    double x() const { return c[0]; }
    double y() const { return c[1]; }
    double z() const { return c[2]; }
    double w() const { return c[3]; }
};
struct IMUData {
    std::uint64_t timestamp_;
    QuaternionStub orientation_;
};
struct PointcloudCluster {
    PointCloud<PointXYZI> ordered_cloud_, planar_cloud_;
};
