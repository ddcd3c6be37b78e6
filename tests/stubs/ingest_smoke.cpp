// Builds the driver-message methods of include/fls_hip_preprocess.h against the stub types and links them to libfls_reg.so; with a
// gfx950 device it also runs one packed 22-byte Livox message through them (a static sensor: the clouds are the kept, gated points).
#include "preprocess_stub_types.h"
#include "fls_hip_preprocess.h"
#include <cstdio>
#include <cstring>

int main() {
    fls_driver_cloud dc{};
    if (fls_ingest_revision() != FLS_INGEST_REVISION || fls_ingest_default_layout(FLS_SENSOR_LIVOX_AVIA, &dc) != FLS_OK || dc.point_step != 32) {
        std::printf("unexpected: revision %d\n", fls_ingest_revision());
        return 1;
    }
    if (fls_device_count() < 1) { std::printf("ingest adapter ok (compiled and linked; no gfx950 device, not run)\n"); return 0; }
    // the packed Livox row: x 0, y 4, z 8, intensity 12, time 16 (uint32 ns), line 20, tag 21; step 22
    dc.point_step = 22;
    dc.intensity_offset = 12; dc.time_offset = 16; dc.line_offset = 20; dc.tag_offset = 21;
    const int n = 100;
    std::vector<unsigned char> msg(22 * n);
    for (int k = 0; k < n; ++k) {
        const float xyzi[4] = {5.f + 0.1f * float(k), 1.f, 0.5f, float(k)};
        const std::uint32_t t = 1000000u * std::uint32_t(k);  // 1 ms apart
        unsigned char* q = msg.data() + 22 * k;
        std::memcpy(q, xyzi, 16);
        std::memcpy(q + 16, &t, 4);
        q[20] = static_cast<unsigned char>(k % 8);  // lines 6 and 7 are dropped: 25 of 100
        q[21] = 0x10;
    }
    const double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -0.28, 1};
    fls_hip::HipScanPreprocessor pre(1.0f, 100.0f, 2, 0.f, T);
    fls_ingest_params ip{};
    ip.struct_size = sizeof(ip);
    ip.lidar_point_time_scale = 1e-9;
    std::vector<IMUData> imu;
    const std::uint64_t stamp = 1000000;
    for (int k = 0; k < 30; ++k) imu.push_back(IMUData{stamp - 20000 + 5000u * std::uint64_t(k), QuaternionStub{{0, 0, 0, 1}}});
    PointcloudCluster c;
    std::uint64_t stamp_out = 0;
    const int st = pre.RunDriver(c, msg.data(), n, dc, ip, stamp, imu, &stamp_out);
    if (st != FLS_IMU_OK || stamp_out != stamp || pre.last_ingest().n_message != 100 || pre.last_ingest().n_converted != 75 || c.ordered_cloud_.size() != 75 ||
        c.planar_cloud_.size() != 38 || c.ordered_cloud_.points[0].z != 0.5f - 0.28f) {
        std::printf("unexpected: status %d converted %llu ordered %zu planar %zu\n", st, (unsigned long long)pre.last_ingest().n_converted,
                    c.ordered_cloud_.size(), c.planar_cloud_.size());
        return 1;
    }
    std::printf("ingest adapter ok (ran: converted %llu ordered %zu planar %zu)\n", (unsigned long long)pre.last_ingest().n_converted,
                c.ordered_cloud_.size(), c.planar_cloud_.size());
    return 0;
}
