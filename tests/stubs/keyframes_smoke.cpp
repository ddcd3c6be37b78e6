// Builds include/fls_hip_keyframes.h (HipKeyframeStore) against the stand-in headers of tests/stubs and links it to libfls_reg.so;
// with a gfx950 device ("run") it stores five keyframes, assembles GetSubMap / MergeMap through the adapter and compares the sub-map
// with the exact filter + a float translation done here.
#include "registration/registration_interface.h"
#include "fls_hip_keyframes.h"
#include <cstdio>
#include <cstring>
#include <random>

// Eigen::Matrix4d's part in GetSubMap: data(), inverse(), operator* (rigid poses only here)
struct PoseStub {
    double m[16];
    double* data() { return m; }
    const double* data() const { return m; }
    PoseStub inverse() const {
        PoseStub o{};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) o.m[i + 4 * j] = m[j + 4 * i];
        for (int i = 0; i < 3; ++i) o.m[12 + i] = -(o.m[i] * m[12] + o.m[i + 4] * m[13] + o.m[i + 8] * m[14]);
        o.m[15] = 1.0;
        return o;
    }
    friend PoseStub operator*(const PoseStub& a, const PoseStub& b) {
        PoseStub o{};
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j)
                for (int k = 0; k < 4; ++k) o.m[i + 4 * j] += a.m[i + 4 * k] * b.m[k + 4 * j];
        return o;
    }
};

static PoseStub translation(double x, double y, double z) {
    PoseStub p{};
    p.m[0] = p.m[5] = p.m[10] = p.m[15] = 1.0;
    p.m[12] = x; p.m[13] = y; p.m[14] = z;
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2 || fls_device_count() < 1) {
        if (fls_keyframes_revision() != FLS_KEYFRAMES_REVISION) return 1;
        std::printf("keyframe adapter compiled; no gfx950 device -> not run\n");
        return 0;
    }
    std::mt19937 rng(3);
    std::uniform_real_distribution<float> u(-10.f, 10.f);
    fls_hip::HipKeyframeStore store;
    std::vector<PCLPointCloudXYZI> clouds(5);
    std::vector<PoseStub> poses;
    size_t stored = 0;
    for (int k = 0; k < 5; ++k) {
        for (int i = 0; i < 2000 + 100 * k; ++i) {
            PCLPointXYZI p{};
            p.x = u(rng); p.y = u(rng); p.z = u(rng); p.intensity = float(i % 100);
            clouds[k].points.push_back(p);
        }
        if (store.Add(clouds[k]) != k) return 2;
        stored += clouds[k].size();
        poses.push_back(translation(1.5 * k, -0.25 * k, 0.125));
    }
    PCLPointCloudXYZI sub, map;
    store.GetSubMap(sub, 2, 1, 5, true, poses);  // keyframes 1..4 (the right range is clipped), relative to keyframe 2
    std::vector<float> want;
    for (int k = 1; k < 5; ++k) {
        std::vector<float> f(4 * clouds[k].size());
        size_t n = 0;
        if (fls_voxel_grid_cloud(0, FLS_VOXELGRID_EXACT, &clouds[k].points[0].x, clouds[k].size(), 8, 0.2f, f.data(), clouds[k].size(), &n) != FLS_OK) return 3;
        const float t[3] = {float(1.5 * (k - 2)), float(-0.25 * (k - 2)), 0.f};
        for (size_t i = 0; i < n; ++i) {
            for (int a = 0; a < 3; ++a) want.push_back((f[4 * i + a] + (0.f + 0.f)) + t[a]);  // R = I: 1 * x + (0 * y + 0 * z)
            want.push_back(f[4 * i + 3]);
        }
    }
    bool same = sub.size() * 4 == want.size();
    for (size_t i = 0; same && i < sub.size(); ++i)
        same = sub.points[i].x == want[4 * i] && sub.points[i].y == want[4 * i + 1] && sub.points[i].z == want[4 * i + 2] && sub.points[i].intensity == want[4 * i + 3];
    store.MergeMap(map, poses);
    const bool ok = same && map.size() > 0 && map.size() <= stored &&  // (a VoxelGrid never adds points)
                    store.stat(5) == 2 && store.size() == 5;
    std::printf("ok=%d same=%d submap=%zu map=%zu\n", int(ok), int(same), sub.size(), map.size());
    return ok ? 0 : 1;
}
