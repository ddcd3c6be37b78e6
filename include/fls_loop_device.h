/* ============================================================================
 * fls_loop_device.h -- LoopClosure::Match (src/slam/loop_closure.cpp:233-267) from clouds that lie on the device (same shared library as
 * fls_reg.h and fls_keyframes.h; FLS_ABI_REVISION and FLS_KEYFRAMES_REVISION stay, this header has a revision of its own).
 *
 * fls_loop_match starts from host clouds: its ten VoxelGridCloud calls are host filters (or device filters that upload their whole input
 * each), the leaf Gaussians of the four NDT targets are built on one host thread and every filtered cloud is uploaded.  The calls below run
 * the same Match -- the same per-device matcher, under the same mutex, the same optimisers and per-point kernels -- from x | y | z |
 * intensity planes on the device: the ten filters are DeviceVoxelGrid::run straight on the planes, the leaf Gaussians are built on the
 * device (csrc/kernels_loop_leaves.hpp), GICP's clouds, grids, covariances and `output` stay there.
 *
 * CONTRACT: T_colmajor, *fitness and every field of fls_loop_stats equal, bit for bit, what fls_loop_match returns for the same points
 * as host rows.  A filter the device declines (an empty cloud, a non-finite point, "leaf size too small", more than 4,194,304 points, the
 * heap-sort case) is answered by the exact host filter on a host copy of that input, downloaded at most once per call and cloud; a
 * target whose leaf build the device declines (more than 4,194,304 filtered points, a box of INT_MAX cells) goes through the host build on
 * a downloaded copy of the FILTERED cloud.  The sparse leaf table (a box above 32 Mi cells) is built on the device, not declined.
 * Environment: FLS_DEVICE_VOXELGRID=0 makes every filter decline that way (read per call); FLS_LOOP_DEVICE_LEAVES=0, read when the device's
 * matcher is created, sends every leaf build through the host.
 *
 * Plain C; no exception crosses the boundary.  Arguments are validated before the device is looked at: FLS_ERR_INVALID for a NULL
 * T_colmajor or fitness, a NULL x, y or z plane of a cloud with n > 0, a plane that is not 4-byte aligned, n above 4,000,000,000.
 * FLS_ERR_DEVICE: no gfx950 device `device_id`, a HIP error.
 * ==========================================================================*/
#ifndef FLS_LOOP_DEVICE_H
#define FLS_LOOP_DEVICE_H
#include "fls_keyframes.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FLS_LOOP_DEVICE_REVISION 1

int fls_loop_device_revision(void);

/* fls_loop_match from device clouds.  src_* / tgt_*: planes of n_src / n_tgt floats each on device `device_id`, at any 4-byte alignment
 * (what fls_keyframes' merge writes and DeviceVoxelGrid::run reads); the intensity planes may be NULL (intensity 0).  The data must be
 * complete when the call is made (the call does not know the stream that wrote it) and is only read.  T_colmajor is the initial guess on
 * entry; stats may be NULL.  n_src == 0 or n_tgt == 0 answers exactly what fls_loop_match answers for an empty cloud. */
fls_status fls_loop_match_device(int device_id, const float* src_x, const float* src_y, const float* src_z, const float* src_i, size_t n_src,
                                 const float* tgt_x, const float* tgt_y, const float* tgt_z, const float* tgt_i, size_t n_tgt, double T_colmajor[16],
                                 float* fitness, fls_loop_stats* stats);

/* fls_keyframes_loop_match with both sub-maps left on the device: GetSubMap twice (leaf 0.2, no final filter) merged into planes, the
 * matcher's stream ordered behind the merges by an event, then fls_loop_match_device's Match.  Nothing of the sub-maps is downloaded unless
 * a filter declines.  Results equal fls_keyframes_loop_match's, bit for bit; statuses as there. */
fls_status fls_keyframes_loop_match_device(fls_keyframes_handle h, const int32_t* src_ids, const double* src_poses, size_t n_src, const int32_t* tgt_ids,
                                           const double* tgt_poses, size_t n_tgt, double T_colmajor[16], float* fitness, fls_loop_stats* stats);

/* Counters of device `device_id`'s matcher since it was created, over both calls above: 0 matches run from device clouds, 1 filters run on
 * the device, 2 filters declined to the host, 3 leaf grids built on the device, 4 leaf grids built on the host, 5 bytes of input clouds
 * downloaded, 6 bytes of filtered clouds downloaded.  Another slot, or no such gfx950 device: 0 (an unknown slot does not look at the
 * device). */
size_t fls_loop_device_stat(int device_id, int slot);

#ifdef __cplusplus
}
#endif
#endif
