"""Mapping-mode replay scenarios: a short seeded trajectory through the synthetic
scene, driven the way FrontEnd does it (src/slam/frontend.cpp:126-139, 207-210): the first cloud(s) go in through
AddCloudToLocalMap in the world frame, every later scan is Match()-ed with update_map = true from a predicted pose, and
Match itself decides whether / how the local map grows.

A scenario is built so that the reference rules that only show up over several scans all fire:
  * IcpOptimized     deque longer than local_map_size (pop_front), frames that fail IsNeedAddCloud, a frame that does not
                     converge within max_iterations (Q10: returns false, map untouched)        icp_optimized.h:151-189,218-234
  * IncrementalNDT   voxels crossing min_points (first estimate), pooled mean / cov updates + SVD clamp, voxels beyond
                     max_points (frozen), LRU eviction at a shrunk capacity, map update with the INPUT pose (Q11)
                                                                                               incremental_ndt.h:130-227,325-334
  * LoamFull         corner / planar deques, VoxelGrid once a deque holds more than 5 frames, keyframe gate
                                                                                               loam_full_kdtree.h:65-104,374-389
  * LoamPointToPlaneKdtree  mapping-mode deque + pop_front, VoxelGrid of the concatenated deque, keyframe gate
                                                                                               loam_point_to_plane_kdtree.h:56-79,145-149
  * LoamPointToPlaneIVOX  down-sampling insert rule + LRU (already covered by test_gpu_parity._replay; here for _ref)
Used by tests/test_gpu_mapping_replay.py (HIP vs oracle), tests/test_ref_pin.py (oracle vs compiled reference) and
tests/golden/make_golden.py.
"""
from __future__ import annotations

import numpy as np

from funny_lidar_slam_amd import registration as reg, synth


def _xform(cloud: np.ndarray, T: np.ndarray) -> np.ndarray:
    """float world-frame copy of a body-frame cloud (what the frontend hands to the first AddCloudToLocalMap)."""
    return (cloud.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def _step(rng, trans, rot_deg):
    T = np.eye(4)
    T[:3, :3] = synth.so3_exp(np.deg2rad(np.asarray(rot_deg, float)))
    T[:3, 3] = trans
    return T


SCENARIOS = {
    # mode, yaml overrides, n_frames, lidar az steps, sensor range
    "icp": dict(mode="IcpOptimized", y=dict(reg.YAML_NCLT_ICP, local_map_size=3, optimization_iter_num=12), frames=11, n_az=90, rng_job=21,
                max_range=45.0, lidar="v64"),
    "ndt": dict(mode="IncrementalNDT", y=dict(reg.YAML_NCLT_NDT, ndt_capacity=2600), frames=10, n_az=100, rng_job=22, max_range=40.0, lidar="v64"),
    # same frames, capacity far away: the map update runs on the device (kernels_ndt_update.hpp)
    "ndt_dev": dict(mode="IncrementalNDT", y=dict(reg.YAML_NCLT_NDT, ndt_capacity=100000), frames=10, n_az=100, rng_job=22, max_range=40.0, lidar="v64"),
    "loam": dict(mode="LoamFull_KdTree", y=dict(reg.YAML_NCLT_LOAM_FULL), frames=11, n_az=90, rng_job=23, max_range=45.0, lidar="v64"),
    "ivox": dict(mode="PointToPlane_IVOX", y=dict(reg.YAML_NCLT_IVOX), frames=7, n_az=60, rng_job=24, max_range=38.0, lidar="v64"),
    # local_map_size=2: the deque is full after the first accepted frame and pops from the second on.  The localization YAML carries zero
    # keyframe thresholds (the gate is never consulted in that mode; at zero any rounding residue passes it), so the scenario takes the
    # mapping configs' 1.0 m / 0.2 rad: the short steps below must fail the gate
    "p2plane_kd": dict(mode="PointToPlane_KdTree", y=dict(reg.YAML_NCLT_LOC_KDTREE, local_map_size=2, keyframe_delta_distance=1.0, keyframe_delta_rotation=0.2),
                       frames=6, n_az=60, rng_job=25,
                       max_range=40.0, lidar="v64"),
}


def make_replay(name: str, n_frames: int = None, yaw_long_deg: float = 4.0, start=None, max_range: float = None, y_over=None) -> dict:
    """start (4x4) / max_range / y_over (YAML overrides): a straight run with a short sensor range, for the LRU-at-capacity tests.
    n_frames / yaw_long_deg: overrides for the long trajectories of tests/test_gpu_long_replay.py (a 9-degree yaw on the long
    steps bends the path into a circle of ~8.5 m radius that stays inside the 80 x 50 m room for any number of frames).
    returns dict(mode, y, init_clouds=[world clouds for the first AddCloudToLocalMap], frames=[dict(scan, corner, guess_step)])
    Frame k is Match(scan_k, T = T_prev_result @ guess_step_k): guess_step is the nominal motion, the true motion differs a little
    (what an IMU prediction looks like); `big_jump` frames get a poor prediction on purpose."""
    sc = SCENARIOS[name]
    scene = synth.make_scene()
    rng = synth.rng_for(5, sc["rng_job"])
    lid = dict(synth.VELODYNE_64 if sc["lidar"] == "v64" else synth.VELODYNE_16, n_az=sc["n_az"])
    mode = sc["mode"]
    if max_range is not None or y_over is not None:
        sc = dict(sc, max_range=max_range if max_range is not None else sc["max_range"], y=dict(sc["y"], **(y_over or {})))
    T = np.eye(4) if start is None else np.array(start, dtype=np.float64)

    def observe(Tw):
        scan = synth.cast_scan(scene, Tw, rng=rng, max_range=sc["max_range"], **lid)
        corner = None
        if mode == "LoamFull_KdTree":
            corner = synth.cast_edge_scan(scene, Tw, 700, rng)
            scan = scan[::2].copy()
        return scan, corner

    scan0, corner0 = observe(T)
    init = [_xform(scan0, T)] + ([_xform(corner0, T)] if corner0 is not None else [])
    if name == "ivox":  # a prior map around the start (localization.cpp:135 loads one; a single sparse scan makes a poor iVox map)
        init = [synth.sample_map(scene, 60000, synth.rng_for(5, 0, 9), radius=30.0)]
    frames = []
    for k in range(n_frames if n_frames is not None else sc["frames"]):
        # alternate long steps (pass the 1.0 m / 0.2 rad keyframe gate) and short ones (fail it)
        long_step = (k % 3) != 1
        nominal = _step(rng, [1.25 if long_step else 0.25, 0.1 * (k % 2), 0.0], [0.0, 0.0, yaw_long_deg if long_step else 0.5])
        noise = synth.random_pose(rng, 0.4, 0.06)
        guess_step = nominal
        if name == "icp" and k == 6:
            # a prediction that is off by ~0.9 m / 5 deg: 12 iterations are not enough -> Match returns false (Q10)
            noise = _step(rng, [0.8, -0.45, 0.0], [0.0, 0.0, 5.0])
        T = T @ nominal @ noise
        if n_frames is not None:
            # long runs: the per-frame noise must not random-walk the sensor into the ground or onto its side -- keep the
            # accumulated yaw and x / y, draw roll / pitch / z afresh every frame
            yaw = np.arctan2(T[1, 0], T[0, 0])
            tilt = np.deg2rad(rng.uniform(-0.4, 0.4, 2))
            T[:3, :3] = synth.so3_exp(np.array([0.0, 0.0, yaw])) @ synth.so3_exp(np.array([tilt[0], tilt[1], 0.0]))
            T[2, 3] = rng.uniform(-0.06, 0.06)
        scan, corner = observe(T)
        frames.append(dict(scan=scan, corner=corner, guess_step=guess_step, T_gt=T.copy()))
    return dict(name=name, mode=mode, y=sc["y"], init_clouds=init, frames=frames)
