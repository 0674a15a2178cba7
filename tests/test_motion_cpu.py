"""The float32 restatement of the between-scan models (tests/motion_ref.py: what mcl_3dl_amd/csrc/motion_kernels.h computes)
against the reference's own results (tests/golden/motion.npz, tests/golden/make_motion_golden.py). Fields without a
transcendental match bit for bit; the others within the bound DESIGN.md ("Numerics") states for the device's double-evaluated
sinf / cosf / acosf / expf."""
import os

import numpy as np
import pytest

import motion_ref as mr
from pf_measure_ref import pf_measure   # pf::measure (pf.h:252-279): float products, float sequential sum, restore unless sum > 0

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion.npz"))


def steps():
    tc = G["pred_tc"]
    for o in G["pred_steps"]:
        yield mr.motion_step(o[0:7], o[7:14], o[14], tc[0], tc[1])


def test_one_predict_step_device_form():
    m = next(steps())
    got = mr.predict(G["pred_state"], G["pred_noise"], m, host=False)
    want = G["pred_out"][0]
    # no transcendental reaches the position (the rotation from before the step), the odometry-error integrals or the noise
    np.testing.assert_array_equal(got[:, :3], want[:, :3])
    np.testing.assert_array_equal(got[:, 7:13], want[:, 7:13])
    np.testing.assert_array_equal(want[:, 13:], G["pred_noise"])  # predict() leaves the noise as it is
    np.testing.assert_allclose(got[:, 3:7], want[:, 3:7], rtol=0, atol=4e-7)


def test_predict_chain_host_libm_and_device_drift():
    st_h = st_d = G["pred_state"]
    for k, m in enumerate(steps()):
        st_h = mr.predict(st_h, G["pred_noise"], m, host=True)
        st_d = mr.predict(st_d, G["pred_noise"], m, host=False)
        want = G["pred_out"][k]
        # with this box's own sinf / cosf: the reference's arithmetic (bit for bit where this libm is the generator's)
        np.testing.assert_allclose(st_h, want[:, :13], rtol=2e-6, atol=2e-7)
        np.testing.assert_allclose(st_d, want[:, :13], rtol=0, atol=2e-6 * (k + 1))


def test_getaxisang_zero_branch_present():
    angs = [float(m["ang"]) for m in steps()]
    assert 0.0 in angs and any(a != 0.0 for a in angs)


def test_state_plus_is_operator_plus():
    got = mr.state_plus(G["plus_state"], G["plus_noise"])
    want = G["plus_out"]
    np.testing.assert_array_equal(got, want[:, :13])
    np.testing.assert_array_equal(want[:, 13:], 0.0)  # a fresh State6DOF: the noise fields are 0


def test_odom_factor():
    st = np.zeros((len(G["odom_lin"]), 13), np.float32)
    st[:, 7:10] = G["odom_lin"]
    want = G["odom_factor"]
    np.testing.assert_allclose(mr.odom_factor(st, G["odom_sigma"][0], host=True), want, rtol=2.5e-7, atol=0)
    np.testing.assert_allclose(mr.odom_factor(st, G["odom_sigma"][0], host=False), want, rtol=2.5e-7, atol=0)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_imu_gravity_measure(case):
    acc = G["imu%d_acc" % case]
    st, w = G["imu%d_state" % case], G["imu%d_w" % case]
    want_lik, want_w, tail = G["imu%d_lik" % case], G["imu%d_wout" % case], G["imu%d_tail" % case]
    for host in (True, False):
        lik = mr.imu_likelihood(st, acc[:3], acc[3], host=host)
        np.testing.assert_array_equal(np.isnan(lik), np.isnan(want_lik))
        ok = ~np.isnan(want_lik)
        np.testing.assert_allclose(lik[ok], want_lik[ok], rtol=2e-6, atol=0)
    # pf::measure on the reference's own likelihoods: the weights and the restore rule, bit for bit
    got_w, restored = pf_measure(w, want_lik)
    assert restored == bool(tail[1])
    np.testing.assert_array_equal(got_w, want_w)


def test_golden_covers_restore_and_nan():
    assert G["imu1_tail"][1] == 1.0 and np.all(G["imu1_lik"] == 0.0)
    assert np.isnan(G["imu2_lik"]).any() and G["imu2_tail"][1] == 1.0
    assert G["imu0_tail"][1] == 0.0
