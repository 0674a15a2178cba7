"""mcl3dl_hip_global_localization_rotations (a pure host function, no GPU) against the float32 restatement of
(Quat(Vec3(0, 0, 2 pi cnt / div_yaw)) * imu_quat).normalized() in tests/global_loc_ref.py, and the restatement's own sanity."""
import numpy as np
import pytest

import global_loc_ref as glr
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import quat_from_rpy

F = np.float32
IMU = {
    "identity": None,
    "tilted": quat_from_rpy([0.03, -0.05, 0.4]).astype(F),
    "not-normalised": (quat_from_rpy([-0.02, 0.04, -1.1]) * 1.7).astype(F),
}


@pytest.mark.parametrize("imu", list(IMU), ids=list(IMU))
@pytest.mark.parametrize("div_yaw", [1, 4, 12, 13])
def test_rotations_are_the_restatement_bit_for_bit(div_yaw, imu):
    got = capi.global_localization_rotations(div_yaw, IMU[imu])
    want = glr.rotations(div_yaw, IMU[imu])
    assert got.shape == (div_yaw, 4) and got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=2e-7)


@pytest.mark.parametrize("div_yaw", [1, 4, 12, 13])
def test_restated_yaw_is_the_kth_step(div_yaw):
    q = glr.rotations(div_yaw).astype(np.float64)
    np.testing.assert_array_equal(q[:, :2], 0.0)
    yaw = (2.0 * np.arctan2(q[:, 2], q[:, 3])) % (2.0 * np.pi)
    want = 2.0 * np.pi * np.arange(div_yaw) / div_yaw
    err = np.abs((yaw - want + np.pi) % (2.0 * np.pi) - np.pi)
    assert err.max() < 1e-6, err.max()


def test_rotations_reject_bad_arguments():
    with pytest.raises(ValueError):
        capi.global_localization_rotations(0)
    with pytest.raises(ValueError):
        capi.global_localization_rotations(4, [0.0, np.nan, 0.0, 1.0])
    with pytest.raises(ValueError):
        capi.global_localization_rotations(4, [0.0, 0.0, 1.0])


def test_particles_weigh_one_over_the_points():
    pts = np.arange(21, dtype=F).reshape(7, 3)
    st, w = glr.particles(pts, 5)
    assert st.shape == (35, 13) and np.all(w == F(1.0 / F(7)))
    np.testing.assert_array_equal(st[5:10, :3], np.tile(pts[1], (5, 1)))
    np.testing.assert_array_equal(st[:, 7:], 0.0)
    np.testing.assert_array_equal(st[7, 3:7], glr.rotations(5)[2])
