"""mcl3dl_hip_group_init_drawn_multivariate (mcl_3dl_amd/csrc/api_rng.inl, rng_kernels.h: rng_multivariate_state_kernel): cbPosition's
pf_->initUsingNoiseGenerator(MultivariateNoiseGenerator<float>(mean, cov)) and the integ_reset_func pass behind it, drawn on the
devices.

Yardsticks: the standard library's own stream through tests/cpp/rng_polar_emul.cpp (`stream std shared`: one shared
normal_distribution is what six calls per particle amount to, tests/test_init_multivariate_cpu.py) with operator() and
generateNoise restated in tests/init_multivariate_ref.py; the CPU replay of the kernels for the engine state (`stream host`) and,
with the device's own logarithm policy (`stream double`), for the values bit for bit. The transform is the numpy restatement's of
the library's definition (the CPU tests show the library returns the same bits)."""
import numpy as np
import pytest

import init_multivariate_ref as im
import resample_cases as rc
import rng_ref
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
F = np.float32
C = capi.C
SPD = im.spd_covariance()
T_SPD = im.noise_transform_ref(SPD)[0]
MEAN7 = im.MEAN7
MEAN6 = im.mean6_of(MEAN7)
LIN = [0, 1, 2, 7, 8, 9, 10, 11, 12]
ROT = [3, 4, 5, 6]
ST = rng_ref.minstd_seed(2024)


@pytest.fixture(scope="module")
def g1():
    g = capi.Group([0])
    yield g
    g.close()


@pytest.fixture(scope="module")
def g1b():
    g = capi.Group([0])
    yield g
    g.close()


def drawn(g, n, state=ST, T=T_SPD, reset=False, mean7=MEAN7):
    behind = g.init_drawn_multivariate(mean7, T, n, state, reset_odom_integ=reset)
    s, w = g.download_state()
    return s, w, behind


def within(got, want, bound):
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound))


@pytest.mark.parametrize("n_p", [1, 2, 63, 64, 65, 256, 257, 1000, 4097])
def test_engine_state_and_install(g1, n_p):
    s, w, behind = drawn(g1, n_p)
    assert behind == rng_ref.stream("host", "shared", ST, 6 * n_p)[1]
    assert g1.resident() == n_p and s.shape == (n_p, 13)
    np.testing.assert_array_equal(w, F(1.0 / n_p))
    np.testing.assert_array_equal(g1.download_odom_noise(), 0)
    assert np.all(np.isfinite(s))


def test_rows_with_the_same_logarithm_policy(g1):
    n = 777
    got, _, behind = drawn(g1, n)
    z, want_behind, _ = rng_ref.stream("double", "shared", ST, 6 * n)
    assert behind == want_behind
    rows, A = im.multivariate_rows(z, MEAN6, T_SPD, n, False)
    np.testing.assert_array_equal(got[:, LIN], rows[:, LIN])
    rng_ref.assert_rows_close(got, rows, im.row_bounds(rows, A, MEAN6, False, same_stream=True))


def test_rows_against_the_reference_stream(g1):
    n = 777
    got, _, behind = drawn(g1, n)
    z, want_behind, _ = rng_ref.stream("std", "shared", ST, 6 * n)
    assert behind == want_behind
    rows, A = im.multivariate_rows(z, MEAN6, T_SPD, n, False)
    rng_ref.assert_rows_close(got, rows, im.row_bounds(rows, A, MEAN6, False))
    same = np.all(got[:, LIN] == rows[:, LIN], axis=1)
    print("rows identical to the standard library's in columns 0-2 and 7-12: %d of %d" % (same.sum(), n))
    assert same.sum() > n // 2


def test_argument_order(g1):
    """T is row-major and applied as T r, and an accepted attempt gives y mult first, x mult second: the transposed matrix and
    the swapped pairs each land outside the bound the right order stays within."""
    n = 777
    got, _, _ = drawn(g1, n)
    z, _, _ = rng_ref.stream("std", "shared", ST, 6 * n)
    rows, A = im.multivariate_rows(z, MEAN6, T_SPD, n, False)
    assert within(got, rows, im.row_bounds(rows, A, MEAN6, False))
    rows_t, A_t = im.multivariate_rows(z, MEAN6, T_SPD.T, n, False)
    assert not within(got, rows_t, im.row_bounds(rows_t, A_t, MEAN6, False))
    z_swapped = z.reshape(3 * n, 2)[:, ::-1].reshape(-1)
    rows_s, A_s = im.multivariate_rows(z_swapped, MEAN6, T_SPD, n, False)
    assert not within(got, rows_s, im.row_bounds(rows_s, A_s, MEAN6, False))


def test_zero_transform_still_draws(g1, g1b):
    n = 1000
    got, w, behind = drawn(g1, n, T=np.zeros((6, 6), F))
    # init_drawn with zero sigmas writes the mean's row through the same generateNoise, and draws nothing
    assert g1b.init_drawn(MEAN7, np.zeros(6, F), n, ST) == ST
    mean_rows = g1b.download_state()[0]
    np.testing.assert_array_equal(got, mean_rows)
    np.testing.assert_array_equal(got[:, LIN], np.tile(np.concatenate([MEAN6[:3], MEAN6[:3], np.zeros(3, F)]), (n, 1)))
    np.testing.assert_array_equal(w, F(1.0 / n))
    # ... while here the engine advances by the calls of 3 n accepted attempts, whatever the matrix holds
    assert behind == rng_ref.stream("host", "shared", ST, 6 * n)[1] and behind != ST


def test_reset_odom_integ(g1, g1b):
    n = 1000
    got, w, behind = drawn(g1, n, reset=True)
    plain, w_b, behind_b = drawn(g1b, n, reset=False)
    assert np.any(plain[:, 7:13] != 0)
    g1b.reset_odom_integ()
    want = g1b.download_state()[0]
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[:, 7:13], 0)
    np.testing.assert_array_equal(got[:, 0:7], plain[:, 0:7])
    np.testing.assert_array_equal(w, w_b)
    assert behind == behind_b
    z, _, _ = rng_ref.stream("std", "shared", ST, 6 * n)
    rows, A = im.multivariate_rows(z, MEAN6, T_SPD, n, True)
    rng_ref.assert_rows_close(got, rows, im.row_bounds(rows, A, MEAN6, True))


def test_second_round(g1):
    """Engine state 318, one particle: the first round's 8 attempts hold fewer than the 3 accepted ones the particle needs
    (tests/test_init_multivariate_cpu.py asserts that the CPU replay takes two rounds there)."""
    state, n_p = im.SECOND_ROUND
    assert rng_ref.stream("host", "shared", state, 6 * n_p)[2] == 2
    got, _, behind = drawn(g1, n_p, state=state)
    z, want_behind, _ = rng_ref.stream("std", "shared", state, 6 * n_p)
    assert behind == want_behind
    rows, A = im.multivariate_rows(z, MEAN6, T_SPD, n_p, False)
    rng_ref.assert_rows_close(got, rows, im.row_bounds(rows, A, MEAN6, False))
    zd, _, _ = rng_ref.stream("double", "shared", state, 6 * n_p)
    np.testing.assert_array_equal(got[:, LIN], im.multivariate_rows(zd, MEAN6, T_SPD, n_p, False)[0][:, LIN])


@pytest.mark.parametrize("devices", [[0, 0, 0], [0, 0]])
def test_shards_match_a_group_of_one(g1, devices):
    g = capi.Group(devices, collective="host")
    try:
        for n_p in (2, 5, 1000):  # 2 particles on three ranks: one shard is empty
            for reset in (False, True):
                one, w_one, behind_one = drawn(g1, n_p, reset=reset)
                many, w_many, behind_many = drawn(g, n_p, reset=reset)
                assert behind_one == behind_many
                np.testing.assert_array_equal(one, many)
                np.testing.assert_array_equal(w_one, w_many)
                assert g.resident() == n_p
    finally:
        g.close()


def test_mixing_with_other_draws_stays_on_the_stream(g1):
    n = 1000
    st1 = g1.init_drawn_multivariate(MEAN7, T_SPD, n, ST)
    st2 = g1.add_noise_drawn(rc.SIGMA6, st1)
    _, st3 = capi.rng_uniform(st2, 0.0, 1.0)
    want1 = rng_ref.stream("std", "shared", ST, 6 * n)[1]
    want2 = rng_ref.stream("std", "fresh", want1, 6 * n)[1]
    assert (st1, st2, st3) == (want1, want2, rng_ref.minstd_next(want2))


def test_distribution(g1):
    """The sample covariance of the drawn noise (position; rpy - mean) at 4096 particles lies within 6 standard errors of the
    covariance in every entry — a cap the numpy reference stays within on the CPU (tests/test_init_multivariate_cpu.py)."""
    got, _, _ = drawn(g1, im.STAT_N, state=im.STAT_STATE)
    worst = im.covariance_within_six_standard_errors(got, SPD)
    print("largest deviation: %.2f standard errors" % worst)
    assert worst <= 6.0


def test_errors_name_the_argument():
    g = capi.Group([0])
    try:
        before = np.random.default_rng(5).normal(0, 1, (8, 13)).astype(F)
        before[:, 3:7] /= np.linalg.norm(before[:, 3:7], axis=1, keepdims=True)
        g.upload_state(before)
        lib = capi.load_library()
        mean, t = np.ascontiguousarray(MEAN7), np.ascontiguousarray(T_SPD)

        def call(mean7=mean, t36=t, n_p=16, reset=0, state=12345, null_state=False):
            st = C.c_uint32(state)
            ref = C.POINTER(C.c_uint32)() if null_state else C.byref(st)
            rc_ = lib.mcl3dl_hip_group_init_drawn_multivariate(g.h, capi._ptr(mean7), capi._ptr(t36), n_p, reset, ref)
            return rc_, lib.mcl3dl_hip_group_last_error(g.h).decode(), int(st.value)

        bad_mean = mean.copy()
        bad_mean[5] = np.nan
        bad_t = t.copy()
        bad_t[2, 5] = np.inf
        cases = [
            (dict(mean7=None), "mean7"),
            (dict(mean7=bad_mean), "mean7[5]"),
            (dict(t36=None), "transform36"),
            (dict(t36=bad_t), "transform36[17]"),
            (dict(n_p=0), "particles"),
            (dict(n_p=0x7fffffff // 16 + 1), "particles"),
            (dict(null_state=True), "engine_state"),
            (dict(state=0), "engine_state"),
            (dict(state=2 ** 31 - 1), "engine_state"),
            (dict(state=2 ** 32 - 1), "engine_state"),
            (dict(reset=2), "reset_odom_integ"),
            (dict(reset=-1), "reset_odom_integ"),
        ]
        for kwargs, word in cases:
            rc_, msg, st_after = call(**kwargs)
            assert rc_ == -3 and word in msg, (kwargs, rc_, msg)
            assert st_after == kwargs.get("state", 12345), kwargs
            assert g.resident() == 8
            np.testing.assert_array_equal(g.download_state()[0], before)
        st = C.c_uint32(12345)
        assert lib.mcl3dl_hip_group_init_drawn_multivariate(None, capi._ptr(mean), capi._ptr(t), 16, 0, C.byref(st)) == -1
        # the Python layer hands the same errors on
        with pytest.raises(capi.EngineError, match=r"-3.*transform36\[17\]"):
            g.init_drawn_multivariate(MEAN7, bad_t, 16, 12345)
        with pytest.raises(capi.EngineError, match="-3.*reset_odom_integ"):
            g.init_drawn_multivariate(MEAN7, T_SPD, 16, 12345, reset_odom_integ=2)
        with pytest.raises(ValueError):
            g.init_drawn_multivariate(MEAN7, np.zeros(35, F), 16, 12345)
        np.testing.assert_array_equal(g.download_state()[0], before)
        # and the same handle still takes a good call
        assert g.init_drawn_multivariate(MEAN7, T_SPD, 16, 12345) == rng_ref.stream("host", "shared", 12345, 96)[1]
        assert g.resident() == 16
    finally:
        g.close()


def test_likelihood_update_is_left_alone():
    """One update on the particles the call installed equals the same update after upload_state of the downloaded rows."""
    sc = make_scene(n=91, n_p=300, n_s=700, n_b=16)
    g = capi.Group([0])
    try:
        g.set_map(sc.map_xyz, sc.map_label, stamp=1, dist_weight=(1.0, 1.0, 1.0))
        g.set_likelihood_params()
        g.set_beam_params(num_points=16)
        T, _ = capi.noise_transform6(np.diag([0.04, 0.04, 0.01, 1e-4, 1e-4, 0.01]) + 1e-3 * SPD)
        g.init_drawn_multivariate(sc.poses[0], T, 300, 4242, reset_odom_integ=True)
        s, w = g.download_state()
        first = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        g.upload_state(s, w)
        second = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        for key in ("weights", "lik", "beam", "quality"):
            np.testing.assert_array_equal(first[key], second[key], err_msg=key)
        assert first["entropy"] == second["entropy"]
        print("particles with a positive likelihood: %d of 300" % np.count_nonzero(first["lik"] > 0))
    finally:
        g.close()
