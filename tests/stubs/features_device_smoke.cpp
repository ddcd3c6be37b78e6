// Builds the device-resident members of include/fls_hip_features.h (RunOnDevice, FillCluster) and of include/fls_hip_registration.h
// (MatchFeatures) against the stand-in headers of tests/stubs and links them to libfls_reg.so.  Nothing runs without a gfx950 device.
#include "registration/registration_interface.h"
#include "fls_hip_features.h"
#include "fls_hip_registration.h"
#include <cstdio>
#include <cstring>

int main(int argc, char**) {
    if (argc < 2 || fls_device_count() < 1) {
        std::printf("features device adapters compiled; revision %d; no gfx950 device -> not run\n", fls_features_device_revision());
        return 0;
    }
    const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    PointcloudCluster c;
    for (int k = 0; k < 5; ++k) {  // fewer than 12 ordered points: both clouds empty, the attach and the empty Match still answer
        PointXYZIRT p{};
        p.x = 10.0f + float(k);
        c.raw_cloud_.points.push_back(p);
    }
    loam::HipFeatureFrontEnd fe(1800, 64, 0.2f / 180.0f * 3.14159265358979323846f, 4.0f, 100.0f, 1.0f, 0.1f, 0, 0.2f, 0.4f);
    size_t nc = 7, np = 7;
    if (!fe.RunOnDevice(c.raw_cloud_, &nc, &np) || nc != 0 || np != 0 || !fe.filtered()) return 3;
    fe.FillCluster(c);
    auto matcher = HipRegistration::LoamFull(0.2, 1.0, 3.0, 0.01, 0.05, 1.0, 0.2, 50, 40, 0.2f, 0.4f, 5);
    Mat4d T;
    std::memcpy(T.data(), I4, sizeof(I4));
    const bool ok = matcher->MatchFeatures(fe, T);  // (no map yet: the attach succeeds, the Match answers FLS_ERR_STATE = false)
    std::printf("ran=1 corner=%zu planar=%zu match=%d\n", c.corner_cloud_.size(), c.planar_cloud_.size(), int(ok));
    return 0;
}
