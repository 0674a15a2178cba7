"""The float32 restatement of the pose-jump bias and of the landmark model (tests/landmark_ref.py: what
mcl_3dl_amd/csrc/landmark_kernels.h and the host side of mcl3dl_hip_group_measure_landmark compute) against the reference's own
headers (tests/golden/landmark.npz, tests/golden/make_landmark_golden.py). Everything without a transcendental matches bit for
bit; the likelihoods and the biases within the derived bounds of landmark_ref's docstring."""
import os

import numpy as np
import pytest

import landmark_ref as lr
import motion_ref as mr

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landmark.npz"))
CASES = range(int(G["lm_cases"][0]))


def assert_rel(got, want, bound):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.abs(want)
    print("max relative error %.3g, of its bound %.3g" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound), (err.max(), (err / bound).max())


@pytest.mark.parametrize("host", [True, False], ids=["host-libm", "device-form"])
def test_jump_bias(host):
    prev, var, st = G["bias_prev"], G["bias_var"], G["bias_state"]
    want_lin, want_ang, want_bias = G["bias_out"].T
    bias, lin, ang, folded = lr.jump_bias(st, prev, var[0], var[1], host=host, parts=True)
    np.testing.assert_array_equal(lin, want_lin)  # Vec3::norm: no transcendental
    np.testing.assert_array_equal(ang == 0.0, want_ang == 0.0)
    np.testing.assert_array_equal(ang < 0.0, want_ang < 0.0)
    # an angle is acosf's result doubled (and folded): one ulp of the unfolded value
    np.testing.assert_allclose(ang, want_ang, rtol=0, atol=4.8e-7)
    assert_rel(bias, want_bias, lr.jump_bias_bound(ang, var[1]))


def test_golden_covers_the_bias_branches():
    st, prev = G["bias_state"], G["bias_prev"]
    ang = G["bias_out"][:, 1]
    w = mr.qmul(st[:, 3:7], np.broadcast_to(mr.qinv(prev[3:7]), (len(st), 4)))[:, 3]
    assert ang[0] == 0.0 and w[0] > 0 and ang[1] == 0.0 and w[1] < 0  # ang = 0 on both signs of w
    assert np.sum((w < 0) & (ang < 0)) >= 10  # the - 2 pi fold
    assert G["bias_out"][2, 0] == 0.0  # no jump: the largest bias
    assert np.all(G["bias_out"][:, 2] >= np.float32(1e-6))


@pytest.mark.parametrize("case", CASES)
def test_landmark_constants_are_the_constructors(case):
    a, sinv = lr.landmark_constants(G["lm%d_cov" % case])
    assert a == G["lm%d_a" % case][0]
    np.testing.assert_array_equal(sinv, G["lm%d_sinv" % case])


def test_column_major_convention():
    cov = G["lm0_cov"]
    assert cov[6 * 0 + 1] != cov[6 * 1 + 0]  # the fixture's covariance is not symmetric, so the layout shows
    _, sinv_t = lr.landmark_constants(cov.reshape(6, 6).T.reshape(36))
    assert not np.array_equal(sinv_t, G["lm0_sinv"])


@pytest.mark.parametrize("case", CASES)
def test_state_minus_and_rpy(case):
    st, m7, diff = G["lm%d_state" % case], G["lm%d_measured" % case], G["lm%d_diff" % case]
    d, q = lr.state_minus(st, m7)
    np.testing.assert_array_equal(d, diff[:, :3])
    np.testing.assert_array_equal(q, diff[:, 3:7])
    t2d = lr.rpy_terms(q)[5]
    for host in (True, False):
        x = lr.landmark_x(st, m7, host=host)
        np.testing.assert_array_equal(x[:, :3], diff[:, :3])
        # atan2f / asinf: one ulp of the result
        np.testing.assert_array_less(np.abs(x[:, 3:] - diff[:, 7:]), np.spacing(np.abs(diff[:, 7:])) * 1.0001 + 1e-45)
        # where t2 was clamped, asin(+-1) is the same float for every faithful libm
        np.testing.assert_array_equal(x[np.abs(t2d) > 1.0, 4], diff[np.abs(t2d) > 1.0, 8])
    if case == 0:
        assert np.any(t2d > 1.0) and np.any(t2d < -1.0)


def test_landmark_likelihood_within_the_bound():
    st, m7 = G["lm0_state"], G["lm0_measured"]
    a, sinv = lr.landmark_constants(G["lm0_cov"])
    for host in (True, False):
        x = lr.landmark_x(st, m7, host=host)
        lik = lr.normal_nd(a, sinv, x, host=host)
        assert np.all(lik > 1e-30)  # normal floats: the relative bound needs no absolute term
        assert_rel(lik, G["lm0_lik"], lr.landmark_bound(x, sinv))
    # the exponent's structure alone (nd.h:74), on the reference's own diff vector: only expf is left to differ
    x_ref = np.concatenate([G["lm0_diff"][:, :3], G["lm0_diff"][:, 7:]], 1)
    assert_rel(lr.normal_nd(a, sinv, x_ref, host=False), G["lm0_lik"], 2.0 * 2.0 ** -23)


@pytest.mark.parametrize("case", [1, 2])
def test_underflow_and_infinite_determinant_restore(case):
    lik = lr.landmark_likelihood(G["lm%d_state" % case], G["lm%d_measured" % case], G["lm%d_cov" % case], host=False)
    np.testing.assert_array_equal(lik, 0.0)
    np.testing.assert_array_equal(G["lm%d_lik" % case], 0.0)
    assert G["lm%d_tail" % case][1] == 1.0
    assert (G["lm2_a"][0] == 0.0) and (G["lm1_a"][0] > 0.0)


@pytest.mark.parametrize("case", CASES)
def test_pf_measure_on_the_references_likelihoods(case):
    w, tail = G["lm%d_w" % case], G["lm%d_tail" % case]
    got_w, restored = lr.pf_measure(w, G["lm%d_lik" % case])
    assert restored == bool(tail[1])
    np.testing.assert_array_equal(got_w, G["lm%d_wout" % case])


@pytest.mark.parametrize("cov", [np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]), np.ones((6, 6)),
                                 np.diag([1.0, -1.0, 1.0, 1.0, 1.0, 1.0]), np.diag([1.0, np.nan, 1.0, 1.0, 1.0, 1.0]),
                                 np.diag([1.0, np.inf, 1.0, 1.0, 1.0, 1.0]), np.diag([1e-9] * 6)],
                         ids=["zero-axis", "rank-one", "negative-det", "nan", "inf", "det-underflows"])
def test_rejected_covariances(cov):
    with pytest.raises(ValueError):
        lr.landmark_constants(cov)


def test_upstream_kat_seed():
    """test/src/test_landmark.cpp at upstream's numbers: the seed tests/test_gpu_landmark_bias.py relies on meets the condition."""
    st, w0, m7, cov = lr.kat_inputs()
    assert abs(st[:, 1].mean() - 2.0) < 0.1 and abs(st[:, 1].var() - 1.0) < 0.1  # upstream's check of the initial cloud
    w, restored = lr.pf_measure(w0, lr.landmark_likelihood(st, m7, cov, host=False))
    assert not restored
    mean, var = lr.weighted_mean_var(st[:, 1], w)
    assert abs(mean - 2.3) < 0.1 and abs(var - 0.5) < 0.1, (mean, var)
