"""The yardstick of the global-localisation tests: cbGlobalLocalization (src/mcl_3dl.cpp:1039-1099) composed from the
reference-backed CPU oracle exactly as the reference composes its own parts, plus the float32 restatement of the particle
set it writes. Shared by tests/test_global_localization_cpu.py and tests/test_gpu_global_localization.py.

  standable_points   pcl::VoxelGrid(grid) over the base map -> a second oracle whose map is the centroid cloud (KdTreeFLANN with
                     the node's point representation) -> radiusSearch(p2, grid) with p2.z = float(double(p.z) + (0.01 + grid))
                     -> the centroids for which nothing is found, in VoxelGrid order
  rotations          (Quat(Vec3(0, 0, 2 pi cnt / div_yaw)) * imu_quat).normalized() in float32, host cosf / sinf
  particles          points x div_yaw states, weights float32(1.0 / float32(points))"""
import numpy as np

import motion_ref as mr
from oracle import pyoracle

F = np.float32


def ref_oracle(**kw):
    """The reference-backed oracle; the composition needs its VoxelGrid, resample and resize, which only it has."""
    assert pyoracle.available("ref"), "oracle/_ref is not built: run __graft_entry__.build() where the reference tree is"
    return pyoracle.Oracle("ref", **kw)


def standable_points(map_xyz, grid, dist_weight):
    """-> (points kept, all centroids, squared distances of the searches, found flags)."""
    grid = float(grid)
    o = ref_oracle(max_search_radius=max(0.4, grid * 1.01))
    c, _ = o.voxel_grid(map_xyz, None, [grid] * 3)
    o.set_map(c, None, stamp=5, dist_weight=dist_weight)
    q = c.copy()
    q[:, 2] = (q[:, 2].astype(np.float64) + (0.01 + grid)).astype(F)
    found, _, sq = o.radius_search(q, grid)
    o.close()
    return c[found == 0], c, sq, found


def quat_from_yaw(yaw, fn):
    """Quat(Vec3(0, 0, yaw)): setRPY (quat.h:202-215) with every product kept, float32."""
    zero = np.zeros_like(yaw)
    t2, t3 = fn["cos"](zero / F(2)), fn["sin"](zero / F(2))
    t4, t5 = fn["cos"](zero / F(2)), fn["sin"](zero / F(2))
    t0, t1 = fn["cos"](yaw / F(2)), fn["sin"](yaw / F(2))
    return np.stack([t0 * t3 * t4 - t1 * t2 * t5,
                     t0 * t2 * t5 + t1 * t3 * t4,
                     t1 * t2 * t4 - t0 * t3 * t5,
                     t0 * t2 * t4 + t1 * t3 * t5], -1).astype(F)


def rotations(div_yaw, imu_quat=None):
    fn = mr.funcs(True)
    imu = np.array([0, 0, 0, 1], F) if imu_quat is None else np.asarray(imu_quat, F)
    yaw = np.array([2.0 * np.pi * k / div_yaw for k in range(div_yaw)], np.float64).astype(F)
    return mr.qnormalized(mr.qmul(quat_from_yaw(yaw, fn), np.broadcast_to(imu, (div_yaw, 4))))


def particles(points, div_yaw, imu_quat=None):
    """-> (state13, weights) of the particle set cbGlobalLocalization leaves."""
    n = len(points) * div_yaw
    st = np.zeros((n, 13), F)
    st[:, :3] = np.repeat(points, div_yaw, 0)
    st[:, 3:7] = np.tile(rotations(div_yaw, imu_quat), (len(points), 1))
    w = np.full(n, F(1.0 / F(len(points))), F)
    return st, w
