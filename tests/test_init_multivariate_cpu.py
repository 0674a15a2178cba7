"""The host side of the `initialpose` draw, without a GPU: mcl_3dl_amd/csrc/noise_transform.h through the stand-alone program
tests/cpp/noise_transform_check.cpp (g++) and through the built library (capi.noise_transform6), against the numpy fp64 restatement
of its definition and against T T^T = the float-cast covariance within the bound derived in tests/init_multivariate_ref.py; and the
stream claim behind mcl3dl_hip_group_init_drawn_multivariate — one normal_distribution<float> per particle, called six times, is the
stream of ONE shared distribution — against the standard library itself."""
import numpy as np
import pytest

import init_multivariate_ref as im
import rng_ref
from mcl_3dl_amd import capi

F = np.float32
SPD = im.spd_covariance()
YAW_VAR = (np.pi / 12.0) ** 2  # rviz's 2D Pose Estimate: 0.5 m, 0.5 m, 15 degrees


def rviz_default():
    c = np.zeros((6, 6))
    c[0, 0] = c[1, 1] = 0.25
    c[5, 5] = YAW_VAR
    return c


def rank2():
    a = np.array([[1, 0.5], [-0.25, 2], [0.75, -1], [0.125, 0.25], [-0.5, 0.375], [1.5, 1]])  # dyadic: A A^T is exact in float
    return a @ a.T


def psd_negative_after_cast():
    rng = np.random.default_rng(7)
    b = rng.normal(0.0, 1.0, (6, 3))
    return b @ b.T


def tie_block():
    """Eigenvectors (1, 1) / sqrt 2 and (1, -1) / sqrt 2 in the x-y block: an exact tie for the largest component."""
    c = np.diag([2.0, 2.0, 0.5, 0.25, 0.125, 1.0])
    c[0, 1] = c[1, 0] = -1.0
    return c


GOOD = {
    "rviz": rviz_default(),
    "spd": SPD,
    "rank2": rank2(),
    "degenerate": 0.01 * np.eye(6),
    "spd_1e-12": 1e-12 * SPD,
    "spd_1e6": 1e6 * SPD,
    "psd_negative_after_cast": psd_negative_after_cast(),
    "tie": tie_block(),
}


@pytest.mark.parametrize("name", sorted(GOOD))
def test_transform_reproduces_the_covariance(name):
    cov = GOOD[name]
    rc, T, ev, clamped, msg = im.transform_program(cov)
    assert rc == 0, msg
    T_lib, ev_lib = capi.noise_transform6(cov)
    np.testing.assert_array_equal(T_lib, T)
    np.testing.assert_array_equal(ev_lib, ev)
    T_ref, lam_ref, clamped_ref = im.noise_transform_ref(cov)
    np.testing.assert_array_equal(T, T_ref)
    np.testing.assert_array_equal(ev, lam_ref.astype(F))
    assert clamped == clamped_ref
    # T T^T in double from the float T
    t = T.astype(np.float64)
    err = np.abs(t @ t.T - im.float_cast(cov))
    bound = im.transform_bound(cov, clamped)
    print("%s: clamped %d, max |T T^T - C| / bound = %g" % (name, clamped, np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound), np.argwhere(err > bound)
    # Eigen's order, and the sign rule: the component of largest magnitude is positive
    assert np.all(np.diff(ev) >= 0) and np.all(ev >= 0)
    for k in range(6):
        assert T[:, k].max() >= -T[:, k].min(), k


def test_rviz_default_is_exact():
    _, T, ev, clamped, _ = im.transform_program(rviz_default())
    assert clamped == 0
    yaw = F(np.sqrt(np.float64(F(YAW_VAR))))
    np.testing.assert_array_equal(ev, np.array([0, 0, 0, F(YAW_VAR), 0.25, 0.25], F))
    # diag(0.5, 0.5, 0, 0, 0, sqrt) up to column order: one non-zero per non-zero row, in columns of their own
    np.testing.assert_array_equal(np.sort(np.abs(T), axis=1)[:, -1], np.array([0.5, 0.5, 0, 0, 0, yaw], F))
    assert np.count_nonzero(T) == 3 and np.all(T >= 0)
    assert len({int(np.argmax(T[i])) for i in (0, 1, 5)}) == 3


def test_rounding_sized_negative_eigenvalues_are_clamped():
    cov = psd_negative_after_cast()
    low = np.linalg.eigvalsh(im.float_cast(cov))[0]
    frob = np.sqrt(np.sum(im.float_cast(cov) ** 2))
    assert -2.0 ** -23 * frob <= low < 0, "the case must have a slightly negative eigenvalue once cast to float"
    rc, T, ev, clamped, _ = im.transform_program(cov)
    assert rc == 0 and clamped >= 1 and np.all(ev >= 0) and np.all(np.isfinite(T))


def test_tie_takes_the_lowest_index():
    _, T, ev, _, _ = im.transform_program(tie_block())
    np.testing.assert_array_equal(ev, np.array([0.125, 0.25, 0.5, 1, 1, 3], F))
    # lambda = 3: (1, -1) / sqrt 2, lambda = 1 (twice): (1, 1) / sqrt 2 and the yaw axis; |x| == |y| exactly, x is the positive one
    for k in (3, 4, 5):
        if T[0, k] != 0:
            assert abs(T[0, k]) == abs(T[1, k]) and T[0, k] > 0
    assert T[1, 5] < 0


def test_only_the_lower_triangle_is_read():
    garbage = SPD.copy()
    garbage[np.triu_indices(6, 1)] = np.random.default_rng(3).normal(0, 100, 15)
    np.testing.assert_array_equal(im.transform_program(garbage)[1], im.transform_program(SPD)[1])
    np.testing.assert_array_equal(capi.noise_transform6(garbage)[0], capi.noise_transform6(SPD)[0])


def test_rejections():
    indefinite = SPD - 0.01 * np.eye(6)
    assert np.linalg.eigvalsh(indefinite)[0] < -1e-3
    rc, _, _, _, msg = im.transform_program(indefinite)
    assert rc == -3 and "eigenvalue 0" in msg and "-0.0" in msg
    with pytest.raises(ValueError):
        im.noise_transform_ref(indefinite)
    nan = SPD.copy()
    nan[4, 2] = np.nan
    rc, _, _, _, msg = im.transform_program(nan)
    assert rc == -3 and "cov36[26]" in msg
    huge = SPD.copy()
    huge[5, 5] = 1e300  # infinite as a float
    assert im.transform_program(huge)[0] == -3
    for bad in (indefinite, nan, huge):
        with pytest.raises(ValueError):
            capi.noise_transform6(bad)
    lib = capi.load_library()
    c, t = np.ascontiguousarray(SPD), np.zeros(36, F)
    assert lib.mcl3dl_hip_noise_transform6(None, capi._ptr(t), None) == -3
    assert lib.mcl3dl_hip_noise_transform6(capi._ptr(c), None, None) == -3
    assert lib.mcl3dl_hip_noise_transform6(capi._ptr(c), capi._ptr(t), None) == 0  # eigenvalues6 may be NULL
    np.testing.assert_array_equal(t.reshape(6, 6), capi.noise_transform6(SPD)[0])


@pytest.mark.parametrize("n", [1, 5, 1000])
def test_six_calls_of_one_distribution_per_particle_are_the_shared_stream(n):
    state = rng_ref.minstd_seed(2024)
    z, behind = im.particles_std(state, n)
    shared, shared_behind, _ = rng_ref.stream("std", "shared", state, 6 * n)
    np.testing.assert_array_equal(z, shared)
    assert behind == shared_behind
    fresh, fresh_behind, _ = rng_ref.stream("std", "fresh", state, 6 * n)
    assert behind != fresh_behind and not np.array_equal(z, fresh)
    # ... and the replayed kernels leave the engine where the standard library does
    assert rng_ref.stream("host", "shared", state, 6 * n)[1] == behind


def test_second_round_state():
    state, n_p = im.SECOND_ROUND
    z, behind, rounds = rng_ref.stream("host", "shared", state, 6 * n_p)
    assert rounds == 2
    want, want_behind = im.particles_std(state, n_p)
    np.testing.assert_array_equal(z, want)
    assert behind == want_behind


def test_reference_rows_pass_the_distribution_check():
    """The cap the GPU test applies (6 standard errors at 4096 particles) is one the numpy reference on the standard library's
    stream stays within, with the same covariance and engine state."""
    T, _, _ = im.noise_transform_ref(SPD)
    z, _, _ = rng_ref.stream("std", "shared", im.STAT_STATE, 6 * im.STAT_N)
    rows, _ = im.multivariate_rows(z, im.mean6_of(im.MEAN7), T, im.STAT_N, False)
    worst = im.covariance_within_six_standard_errors(rows, SPD)
    print("largest deviation: %.2f standard errors" % worst)
    assert worst <= 6.0
