// Builds include/fls_hip_localmap.h (HipLocalMapSource) against the stand-in headers of tests/stubs and links it to libfls_reg.so; with
// a gfx950 device ("run") it stores a global map, walks LoadLocalMap's crop-box branch and its tile branch through the adapter, holds
// the cut against the box test done here, and hands both local maps to a localization matcher.
#include "fls_hip_registration.h"
#include "fls_hip_localmap.h"
#include <cmath>
#include <cstdio>
#include <random>

static Mat4d pose_at(double x, double y, double z) {
    Mat4d T;
    for (int i = 0; i < 16; ++i) T.data()[i] = (i % 5 == 0) ? 1.0 : 0.0;
    T.data()[12] = x; T.data()[13] = y; T.data()[14] = z;
    return T;
}

int main(int argc, char** argv) {
    if (argc < 2 || fls_device_count() < 1) {
        if (fls_localmap_revision() != FLS_LOCALMAP_REVISION) return 1;
        std::printf("localmap adapter compiled; no gfx950 device -> not run\n");
        return 0;
    }
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-200.f, 200.f), h(-2.f, 6.f);
    PCLPointCloudXYZI global;
    for (int i = 0; i < 60000; ++i) {
        PCLPointXYZI p{};
        p.x = u(rng); p.y = u(rng); p.z = (i % 2) ? -1.8f : h(rng); p.intensity = float(i % 100);
        global.points.push_back(p);
    }
    fls_hip::HipLocalMapSource source;
    if (source.SetGlobalMap(global, 0.f) != global.size()) return 2;
    std::shared_ptr<HipRegistration> matcher = HipRegistration::PointToPlaneIVOX(0.1, 0.005, 0.001, 10, /*is_localization_mode=*/true);

    const Mat4d T0 = pose_at(20.3, -31.7, 0.4);
    const bool first = source.LoadLocalMap(T0, true), again = source.LoadLocalMap(pose_at(25.0, -30.0, 0.4));  // 5 m on: inside the margin
    PCLPointCloudXYZI local;
    source.GetLocalMap(local);
    const float mn[3] = {float(20.3 - 100.0), float(-31.7 - 100.0), float(0.4 - 100.0)}, mx[3] = {float(20.3 + 100.0), float(-31.7 + 100.0), float(0.4 + 100.0)};
    size_t k = 0;
    bool same = true;
    for (const auto& p : global.points) {
        if (p.x < mn[0] || p.y < mn[1] || p.z < mn[2] || p.x > mx[0] || p.y > mx[1] || p.z > mx[2]) continue;
        same = same && k < local.size() && local.points[k].x == p.x && local.points[k].y == p.y && local.points[k].z == p.z && local.points[k].intensity == p.intensity;
        ++k;
    }
    same = same && k == local.size() && k > 0;
    const bool added = source.AddTo(*matcher);

    const size_t n_tiles = source.Split(100.0);
    const bool tiles_first = source.LoadTileMap(T0, 0.5f), tiles_again = source.LoadTileMap(pose_at(21.0, -31.0, 0.4), 0.5f);
    const bool added_tiles = source.AddTo(*matcher);
    const bool ok = first && !again && same && added && n_tiles >= 16 && tiles_first && !tiles_again && added_tiles && source.stat(3) == 1 && source.stat(4) == 1 &&
                    source.stat(8) == 1 && source.stat(9) == 2 && source.stat(10) == 0;
    std::printf("ok=%d same=%d local=%zu tiles=%zu\n", int(ok), int(same), local.size(), n_tiles);
    return ok ? 0 : 1;
}
