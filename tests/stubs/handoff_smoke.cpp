// Builds the revision-9 members of include/fls_hip_preprocess.h (RunOnDevice, FillCluster) and include/fls_hip_registration.h
// (MatchPreprocessed) against the stand-in headers of tests/stubs and links them to libfls_reg.so; with a gfx950 device ("run") it
// drives one raw cloud -> pose through them and compares it with the host-cloud path (Run + Match) on a second pair of objects.
#include "fls_hip_registration.h"
#include "fls_hip_preprocess.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

struct QuaternionStub {
    double c[4];  // x, y, z, w
    double x() const { return c[0]; }
    double y() const { return c[1]; }
    double z() const { return c[2]; }
    double w() const { return c[3]; }
};
struct ImuStub {
    unsigned long long timestamp_;
    QuaternionStub orientation_;
};

static PCLPointCloudXYZI map_cloud(int n) {
    std::mt19937 rng(1);
    std::uniform_real_distribution<float> u(-20.f, 20.f), h(-1.8f, 4.f);
    PCLPointCloudXYZI c;
    for (int i = 0; i < n; ++i) {
        PCLPointXYZI p{};
        if (i % 3 == 0) { p.x = 12.f; p.y = u(rng); p.z = h(rng); }
        else if (i % 3 == 1) { p.x = u(rng); p.y = -9.f; p.z = h(rng); }
        else { p.x = u(rng); p.y = u(rng); p.z = -1.8f; }
        c.points.push_back(p);
    }
    return c;
}

int main(int argc, char** argv) {
    if (argc < 2 || fls_device_count() < 1) { std::printf("handoff adapters compiled; no gfx950 device -> not run\n"); return 0; }
    const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    PCLPointCloudXYZIRT raw;  // the map's surfaces seen from 5 cm below, one time stamp per point
    const PCLPointCloudXYZI surf = map_cloud(60000);
    for (size_t k = 0; k < surf.size(); ++k) {
        PointXYZIRT p{};
        p.x = surf.points[k].x; p.y = surf.points[k].y; p.z = surf.points[k].z - 0.05f;
        p.intensity = float(k % 200); p.ring = static_cast<unsigned short>(k % 64); p.time = 1.0e-6f * float(k);
        raw.points.push_back(p);
    }
    std::vector<ImuStub> imu;
    const unsigned long long stamp = 1000000;
    for (int k = 0; k < 40; ++k) imu.push_back(ImuStub{stamp - 20000 + 5000ull * unsigned(k), QuaternionStub{{0, 0, 0, 1}}});
    Mat4d T[2];
    bool ok[2];
    size_t n_planar[2];
    for (int dev = 0; dev < 2; ++dev) {
        fls_hip::HipScanPreprocessor pre(1.0f, 100.0f, 2, 0.5f, I4);
        auto matcher = HipRegistration::PointToPlaneIVOX(0.1, 0.005, 0.001, 10);
        matcher->AddCloudToLocalMap({map_cloud(200000)});
        std::memcpy(T[dev].data(), I4, sizeof(I4));
        auto cluster = std::make_shared<PointcloudCluster>();
        if (dev) {
            if (pre.RunOnDevice(stamp, raw, imu) != FLS_IMU_OK) return 2;
            ok[dev] = matcher->MatchPreprocessed(pre, T[dev]);
            pre.FillCluster(*cluster);  // still available afterwards, fetched here
        } else {
            if (pre.Run(*cluster, raw, stamp, imu) != FLS_IMU_OK) return 2;
            ok[dev] = matcher->Match(cluster, T[dev]);
        }
        n_planar[dev] = cluster->planar_cloud_.size();
    }
    const bool same = ok[0] == ok[1] && n_planar[0] == n_planar[1] && std::memcmp(T[0].data(), T[1].data(), sizeof(I4)) == 0;
    std::printf("ok=%d same=%d planar=%zu tz=%.4f (expect ~ +0.05)\n", int(ok[1]), int(same), n_planar[1], T[1].data()[14]);
    return (ok[1] && same && std::fabs(T[1].data()[14] - 0.05) < 0.01) ? 0 : 1;
}
