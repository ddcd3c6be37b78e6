// fls_reg.hip -- libfls_reg.so: the C ABI (include/*.h) over the gfx950 registration back-end.
// Single translation unit: device kernels (kernels_*.hpp) + host matchers, maps and front ends + the ABI layers below, one header per
// family of public headers.  Built by csrc/Makefile:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// There is no CPU fallback: without a gfx950 device every create call fails with FLS_ERR_DEVICE.
//
// What an integrator links against (host code only; the call plumbing they share is abi_common.hpp):
#include "abi_matcher.hpp"   // fls_reg.h, fls_batch.h, fls_batch_ivox.h, fls_map_ivox.h, fls_map_ndt.h, fls_map_kd.h
#include "abi_frontend.hpp"  // fls_features.h, fls_features_device.h, fls_preprocess.h, fls_ingest.h, the two attach calls
#include "abi_stores.hpp"    // fls_keyframes.h, fls_localmap.h
// What exists for the tests.  These hooks are the first host code to name some kernels, and the code object lists kernels in the order
// of first naming: keep the order of these lines, and of the hooks within each file.
#include "abi_debug_fit.hpp"    // fls_debug_linalg.h, fls_debug_fit.h, fls_debug_ndt.h; fls_debug_fullpiv_qr6, _ldlt6, _last_system
#include "abi_debug_voxel.hpp"  // fls_debug_voxel_grid, _voxel_grid_timed, _exact_sort, _exact_sort_marks
#include "abi_debug_loop.hpp"   // fls_debug_loop.h
#include "abi_debug_knn.hpp"    // fls_debug_knn.h
#include "abi_debug_ivox_update.hpp"  // fls_debug_ivox_update.h (names no kernel of its own)
#include "abi_debug_ivox_decide.hpp"  // fls_debug_ivox_decide.h (names no kernel of its own)
// The reference neighbour order of the iVox kind: its kernel is named here, behind every one above (see the header).
#include "abi_knn_order.hpp"     // fls_knn_order.h
// The loop-closure Match from device clouds: its leaf-build kernels are named here, behind every other one, for the same reason.
#include "abi_loop_device.hpp"   // fls_loop_device.h, fls_debug_loop_leaves.h
// The Gauss-Newton tails on caller-supplied rows: the test kernels are named here, behind every other one, for the same reason.
#include "abi_debug_tail.hpp"    // fls_debug_tail.h
