// ingest_product_shim.cpp -- the product's own host-compilable pieces of kernels_ingest.hpp (A(y, x) and the step-function combine
// operator), exported for tests/test_ingest_model.py.  Compiled with hipcc like tests/host/host_logic_test.cpp; makes no HIP call.
#include "../../funny_lidar_slam_amd/csrc/kernels_ingest.hpp"
#include <vector>

namespace {
// composition of the steps of [a, b) as a balanced tree: another association than the left-to-right one of a sequential loop
fls::IngestStep tree(const std::vector<fls::IngestStep>& f, size_t a, size_t b) {
    if (a == b) return fls::ingest_step_identity();
    if (b - a == 1) return f[a];
    const size_t m = a + (b - a) / 2;
    return fls::ingest_step_compose(tree(f, a, m), tree(f, m, b));
}
}  // namespace

extern "C" {

void ip_atan2_many(const double* y, const double* x, size_t n, double* out) {
    for (size_t k = 0; k < n; ++k) out[k] = fls::ingest_atan2(y[k], x[k]);
}
float ip_base_time(float y_first, float x_first, float y, float x) { return fls::ingest_base_time(fls::ingest_yaw(y_first, x_first), fls::ingest_yaw(y, x)); }

// the period loop of one cloud through the combine operator: per ring, the time of point i = f_i(prefix(i)(0)), the prefix composed as
// a tree over chunks of `chunk` points with the running value carried between chunks (the kernel's structure)
void ip_period_scan(const float* base, const unsigned char* ring, const unsigned char* first, size_t n, int scan_num, size_t chunk, float* time) {
    const float P = fls::ingest_period();
    for (int r = 0; r < scan_num; ++r) {
        float carry = 0.f;
        for (size_t c0 = 0; c0 < n; c0 += chunk) {
            const size_t c1 = std::min(n, c0 + chunk);
            std::vector<fls::IngestStep> f;
            for (size_t i = c0; i < c1; ++i)
                f.push_back(ring[i] != r ? fls::ingest_step_identity() : first[i] ? fls::ingest_step_first() : fls::ingest_step_point(base[i], P));
            for (size_t i = c0; i < c1; ++i) {
                if (ring[i] != r || first[i]) continue;
                const float last = fls::ingest_step_apply(tree(f, 0, i - c0), carry);
                time[i] = fls::ingest_step_apply(f[i - c0], last);
            }
            carry = fls::ingest_step_apply(tree(f, 0, c1 - c0), carry);
        }
    }
}

}  // extern "C"
