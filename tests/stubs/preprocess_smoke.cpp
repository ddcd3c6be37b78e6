// Builds include/fls_hip_preprocess.h against stub types and links it to libfls_reg.so; with a gfx950 device it also runs one small
// scan through it (a static sensor: the clouds are the gated raw points).
#include "preprocess_stub_types.h"
#include "fls_hip_preprocess.h"
#include <cstdio>

int main() {
    if (fls_device_count() < 1) { std::printf("preprocess adapter ok (compiled and linked; no gfx950 device, not run)\n"); return 0; }
    const double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -0.28, 1};
    fls_hip::HipScanPreprocessor pre(1.0f, 100.0f, 2, 0.f, T);
    PointCloud<PointXYZIRT> raw;
    for (int k = 0; k < 100; ++k) raw.points.push_back(PointXYZIRT{5.f + 0.1f * float(k), 1.f, 0.5f, 0.f, float(k), std::uint8_t(k % 16), 0.001f * float(k)});
    raw.points[3].x = 500.f;  // outside max_distance
    std::vector<IMUData> imu;
    const std::uint64_t stamp = 1000000;
    for (int k = 0; k < 30; ++k) imu.push_back(IMUData{stamp - 20000 + 5000u * std::uint64_t(k), QuaternionStub{{0, 0, 0, 1}}});
    PointcloudCluster c;
    const int st = pre.Run(c, raw, stamp, imu);
    if (st != FLS_IMU_OK || c.ordered_cloud_.size() != 99 || c.planar_cloud_.size() != 50 || c.ordered_cloud_.points[0].z != 0.5f - 0.28f) {
        std::printf("unexpected: status %d ordered %zu planar %zu\n", st, c.ordered_cloud_.size(), c.planar_cloud_.size());
        return 1;
    }
    std::printf("preprocess adapter ok (ran: ordered %zu planar %zu)\n", c.ordered_cloud_.size(), c.planar_cloud_.size());
    return 0;
}
