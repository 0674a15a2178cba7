"""The filter's noise drawn on the devices from the reference's engine (mcl_3dl_amd/csrc/rng_kernels.h, host_rng.h, api_rng.inl):
mcl3dl_hip_rng_seed / _rng_uniform and the group's add_noise_drawn / init_drawn / draw_odom_noise / resample_apply_drawn.

Yardsticks: the reference's own generateNoise rows behind std::default_random_engine(12345) and one uniform draw — committed in
tests/golden/resample.npz, and asked live from oracle/_ref where that is built; the standard library's stream through
tests/cpp/rng_polar_emul.cpp (`stream std`) for other start states, sigmas and means, with generateNoise restated in
tests/rng_ref.py; the CPU replay of the kernels (`stream host`) for the engine state. The device takes the polar method's
logarithm in double, so values are compared within the bound derived in tests/rng_ref.py and bit for bit wherever the device's
noise rows equal the yardstick's; engine states are compared exactly."""
import os
import time

import numpy as np
import pytest

import motion_ref as mr
import resample_cases as rc
import rng_ref
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene
from oracle import pyoracle

pytestmark = pytest.mark.gpu
F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "resample.npz"))
ODOM = np.load(os.path.join(HERE, "golden", "rng_odom_noise.npz"))
ZERO6 = np.zeros(6, F)
IDENTITY7 = np.array([0, 0, 0, 0, 0, 0, 1], F)
ODOM_ERR4 = np.array([0.2, 0.05, 0.1, 0.3], F)  # lin_lin, lin_ang, ang_ang, ang_lin


@pytest.fixture(scope="module")
def g1():
    g = capi.Group([0])
    yield g
    g.close()


@pytest.fixture(scope="module")
def g1b():
    """A second group of one: the host-drawn counterpart of every call."""
    g = capi.Group([0])
    yield g
    g.close()


@pytest.fixture(scope="module")
def g3():
    """Three contexts on the one device, combined through the host: uneven shards at 1000 particles."""
    g = capi.Group([0, 0, 0], collective="host")
    yield g
    g.close()


def states(n, seed=5):
    rng = np.random.default_rng(seed)
    s = rng.normal(0, 1, (n, 13)).astype(F)
    s[:, 3:7] /= np.linalg.norm(s[:, 3:7], axis=1, keepdims=True)
    return s


def after_seed_and_uniform(seed, pstep):
    """The engine state where the reference's rows of tests/golden/resample.npz / pyoracle's resample_draws start."""
    ip, st = capi.rng_uniform(capi.rng_seed(seed), 0.0, pstep)
    return ip, st


def reference_rows(n):
    """n generateNoise rows with SIGMA6 behind engine(12345) and one uniform draw: the live reference where it is built, the
    committed rows of the same stream otherwise."""
    if pyoracle.available("ref"):
        return pyoracle.Oracle("ref").resample_draws(rc.SEED, 1.0, rc.SIGMA6, n)[1]
    rows = GOLD["n2048_d900_noise"]
    assert n <= len(rows)
    return rows[:n]


def std_rows(state, mean6, sigma6, n):
    """Rows from the standard library's stream + tests/rng_ref.py's generateNoise; (rows, z sigma, engine state behind)."""
    d = int(np.count_nonzero(np.asarray(sigma6)))
    z, behind, _ = rng_ref.stream("std", "fresh", state, n * d) if d else (np.zeros(0, F), state, 0)
    rows, zs = rng_ref.noise_rows(z, mean6, sigma6, n)
    return rows, zs, behind


def device_rows(g, state, sigma6, n):
    """The device's own noise rows: pf::init about the identity pose is generateNoise with State6DOF()'s mean."""
    behind = g.init_drawn(IDENTITY7, sigma6, n, state)
    return g.download_state()[0], behind


def zero_mean_zs(rows):
    return np.concatenate([rows[:, 0:3], rows[:, 10:13]], axis=1)


def test_uniform_and_seed_are_the_references():
    assert capi.rng_seed(0) == 1 and capi.rng_seed(2 ** 31 - 1) == 1 and capi.rng_seed(12345) == 12345
    small = F(1.0e-06)
    for name, probs in (("first", [small, 0.2, 0.2, 0.2, F(0.4) - small]), ("last", [0.2, 0.2, 0.2, F(0.4) - small, small])):
        acc = F(0)
        for p in np.array(probs, F):
            acc = F(acc + p)
        ip, st = after_seed_and_uniform(12345, float(F(acc / F(5))))
        assert F(ip) == GOLD["kat_initial_p_" + name]
        assert st == rng_ref.minstd_next(12345)
    # the two edges of generate_canonical: next output 1 (c = 0), next output 2^31 - 2 (c rounds to 1: nextafter(1, 0))
    assert capi.rng_uniform(rng_ref.A_INV, 2.0, 5.0) == (2.0, 1)
    v, st = capi.rng_uniform(rng_ref.BEFORE_MAX, 0.0, 1.0)
    assert F(v) == np.nextafter(F(1), F(0)) and st == rng_ref.M - 1


@pytest.mark.parametrize("n_p", [1, 5, 64, 65, 1000, 4097])
def test_stream_position_behind_add_noise(g1, n_p):
    _, st = after_seed_and_uniform(rc.SEED, 1.0)
    g1.upload_state(states(n_p))
    behind = g1.add_noise_drawn(rc.SIGMA6, st)
    _, want, rounds = rng_ref.stream("host", "fresh", st, 6 * n_p)
    assert behind == want
    assert g1.resident() == n_p


def test_add_noise_values_against_the_reference(g1, g1b):
    n = 1200
    _, st = after_seed_and_uniform(rc.SEED, 1.0)
    rows = reference_rows(n)
    dev, _ = device_rows(g1, st, rc.SIGMA6, n)
    bound = rng_ref.row_bounds(rows, zero_mean_zs(rows), ZERO6)
    equal = np.all(dev == rows, axis=1)
    print("noise rows identical to the reference's: %d of %d" % (equal.sum(), n))
    assert equal.sum() > n // 2
    rng_ref.assert_rows_close(dev, rows, bound)
    s = states(n)
    g1.upload_state(s)
    g1.add_noise_drawn(rc.SIGMA6, st)
    g1b.upload_state(s)
    g1b.add_noise(rows)
    got, want = g1.download_state()[0], g1b.download_state()[0]
    rng_ref.assert_rows_close(got, want, rng_ref.plus_bounds(s, want, bound, False), equal)
    np.testing.assert_array_equal(g1.download_odom_noise(), 0)


@pytest.mark.parametrize("n,dead", rc.CASES)
def test_resample_apply_drawn_against_the_three_call_sequence(g1, g1b, n, dead):
    s, w = rc.make_case(n, dead)
    key = "n%d_d%d" % (n, dead)
    g1.upload_state(s, w)
    pstep = g1.resample_begin()
    ip, st = after_seed_and_uniform(rc.SEED, pstep)
    assert F(ip) == GOLD[key + "_initial_p"]
    src, dup, nd = g1.resample_plan(0, ip)
    np.testing.assert_array_equal(src, GOLD[key + "_source"])
    np.testing.assert_array_equal(dup, GOLD[key + "_dup"])
    rows = GOLD[key + "_noise"]
    assert nd == len(rows)
    behind = g1.resample_apply_drawn(rc.SIGMA6, st)
    assert behind == rng_ref.stream("host", "fresh", st, 6 * nd)[1]
    got, got_w = g1.download_state()
    want = GOLD[key + "_states"]
    np.testing.assert_array_equal(got_w, F(1.0) / F(n))
    copied = dup == 0
    np.testing.assert_array_equal(got[copied], want[copied])
    dev, _ = device_rows(g1b, st, rc.SIGMA6, nd)
    equal = np.all(dev == rows, axis=1)
    bound = rng_ref.plus_bounds(s[src[dup == 1]], want[dup == 1], rng_ref.row_bounds(rows, zero_mean_zs(rows), ZERO6), True)
    rng_ref.assert_rows_close(got[dup == 1], want[dup == 1], bound, equal)


def test_init_drawn_at_a_mean_pose(g1):
    n = 777
    rpy = np.array([[0.3, -0.2, 1.1]], F)
    mean7 = np.concatenate([[1.5, -2.0, 0.25], rng_ref.set_rpy(rpy)[0]]).astype(F)
    import landmark_ref as lr
    t0, t1, t2, t3, t4 = (t.astype(np.float64) for t in lr.rpy_terms(mean7[None, 3:7])[:5])
    mean6 = np.concatenate([mean7[:3], [np.arctan2(t3, t4)[0], np.arcsin(t2)[0], np.arctan2(t1, t0)[0]]]).astype(F)
    np.testing.assert_allclose(mean6[3:], rpy[0], atol=1e-6)
    st = rng_ref.minstd_seed(2024)
    behind = g1.init_drawn(mean7, rc.SIGMA6, n, st)
    rows, zs, want_behind = std_rows(st, mean6, rc.SIGMA6, n)
    assert behind == want_behind
    got, w = g1.download_state()
    np.testing.assert_array_equal(w, F(1.0 / n))
    rng_ref.assert_rows_close(got, rows, rng_ref.row_bounds(rows, zs, mean6))
    assert np.mean(np.all(got[:, [0, 1, 2, 7, 8, 9, 10, 11, 12]] == rows[:, [0, 1, 2, 7, 8, 9, 10, 11, 12]], axis=1)) > 0.5
    np.testing.assert_array_equal(g1.download_odom_noise(), 0)


@pytest.mark.parametrize("sigma6", [(0.1, 0, 0.05, 0, 0, 0.05), (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0.02, 0)])
def test_zero_sigmas_draw_nothing(g1, sigma6):
    n = 1000
    sigma6 = np.array(sigma6, F)
    st = rng_ref.minstd_seed(99)
    rows, zs, want_behind = std_rows(st, ZERO6, sigma6, n)
    s = states(n)
    g1.upload_state(s)
    behind = g1.add_noise_drawn(sigma6, st)
    assert behind == want_behind
    if not sigma6.any():
        assert behind == st
    got = g1.download_state()[0]
    want = mr.state_plus(s, rows)
    bound = rng_ref.plus_bounds(s, want, rng_ref.row_bounds(rows, zs, ZERO6), False)
    rng_ref.assert_rows_close(got, want, bound)
    # a wrong D shifts every later particle: the last one as well as the first, bit for bit where nothing is drawn
    for i in (0, n - 1):
        for k in np.flatnonzero(sigma6[:3] == 0):
            assert got[i, k] == s[i, k] and got[i, 7 + k] == s[i, 7 + k]
        for k in np.flatnonzero(sigma6[3:] == 0):
            assert got[i, 10 + k] == s[i, 10 + k]
    dev, _ = device_rows(g1, st, sigma6, n)
    rng_ref.assert_rows_close(dev[[0, n - 1]], rows[[0, n - 1]], rng_ref.row_bounds(rows, zs, ZERO6)[[0, n - 1]])
    assert np.mean(dev[:, :3] == rows[:, :3]) > 0.9


def test_odometry_noise_stream_and_storage_order(g1):
    z = ODOM["z"]
    n = len(z)
    g1.upload_state(states(n))
    behind = g1.draw_odom_noise(ODOM_ERR4, int(ODOM["state"]))
    assert behind == int(ODOM["state_behind"])
    got = g1.download_odom_noise()
    # draw order ll, la, aa, al; storage order {ll, la, al, aa}
    want = np.stack([z[:, 0] * ODOM_ERR4[0], z[:, 1] * ODOM_ERR4[1], z[:, 3] * ODOM_ERR4[3], z[:, 2] * ODOM_ERR4[2]], axis=1)
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= rng_ref.ODOM_REL * np.abs(want)), np.argwhere(err > rng_ref.ODOM_REL * np.abs(want))[:5]
    assert np.mean(got == want) > 0.9
    swapped = want[:, [0, 1, 3, 2]]
    assert not np.all(np.abs(got - swapped) <= rng_ref.ODOM_REL * np.abs(swapped))


@pytest.mark.parametrize("state,k", [(109, 1), (704, 2)])
def test_second_round(g1, state, k):
    """(state, K) pairs whose first round falls short of K accepted attempts (tests/test_rng_polar_cpu.py asserts that the CPU
    replay takes two rounds on them): the device's result equals the replay's."""
    z, want_behind, rounds = rng_ref.stream("host", "fresh", state, k)
    assert rounds == 2
    sigma6 = np.array([0.1, 0, 0, 0, 0, 0], F)
    dev, behind = device_rows(g1, state, sigma6, k)
    assert behind == want_behind
    rows, zs = rng_ref.noise_rows(z, ZERO6, sigma6, k)
    rng_ref.assert_rows_close(dev, rows, rng_ref.row_bounds(rows, zs, ZERO6))


def run_all_calls(g, s, w):
    """Every drawn call once, on one engine-state word; what there is to compare afterwards."""
    out = {}
    st = rng_ref.minstd_seed(31337)
    st = g.init_drawn(np.concatenate([[0.5, 1.0, -0.25], rng_ref.set_rpy(np.array([[0.1, 0.2, -0.4]], F))[0]]), rc.SIGMA6,
                      len(s), st)
    out["init"], out["init_w"] = g.download_state()
    g.upload_state(s, w)
    st = g.draw_odom_noise(ODOM_ERR4, st)
    out["odom"] = g.download_odom_noise()
    pstep = g.resample_begin()
    ip, st = capi.rng_uniform(st, 0.0, pstep)
    out["plan"] = g.resample_plan(0, ip)
    st = g.resample_apply_drawn(rc.SIGMA6, st)
    out["resampled"], out["resampled_w"] = g.download_state()
    out["odom_resampled"] = g.download_odom_noise()
    st = g.add_noise_drawn(rc.SIGMA6, st)
    out["noised"] = g.download_state()[0]
    out["state"] = st
    return out


def test_shards_match_a_group_of_one(g1, g3):
    s, w = rc.make_case(1000, 300)
    one, three = run_all_calls(g1, s, w), run_all_calls(g3, s, w)
    assert one["state"] == three["state"]
    for key in ("init", "init_w", "odom", "resampled", "resampled_w", "odom_resampled", "noised"):
        np.testing.assert_array_equal(one[key], three[key], err_msg=key)
    for a, b in zip(one["plan"], three["plan"]):
        np.testing.assert_array_equal(a, b)
    dup = one["plan"][1] == 1
    assert dup.any() and not dup.all()
    np.testing.assert_array_equal(one["odom_resampled"][dup], 0)
    assert np.all(one["odom_resampled"][~dup] == one["odom"][one["plan"][0][~dup]])


def test_mixing_with_host_draws_stays_on_the_stream(g1, g1b):
    """draw_odom_noise, a host uniform, resample_apply_drawn, add_noise_drawn on one state word against the same sequence drawn
    by the standard library on one engine and fed to the host-array entry points."""
    n = 1000
    s, w = rc.make_case(n, 300)
    st0 = rng_ref.minstd_seed(777)
    g1.upload_state(s, w)
    g1b.upload_state(s, w)
    st1 = g1.draw_odom_noise(ODOM_ERR4, st0)
    z, want1, _ = rng_ref.stream("std", "shared", st0, 4 * n)
    assert st1 == want1
    z = z.reshape(n, 4)
    g1b.set_odom_noise(np.stack([z[:, 0] * ODOM_ERR4[0], z[:, 1] * ODOM_ERR4[1], z[:, 3] * ODOM_ERR4[3], z[:, 2] * ODOM_ERR4[2]],
                                axis=1))
    pstep = g1.resample_begin()
    assert g1b.resample_begin() == pstep
    ip, st2 = capi.rng_uniform(st1, 0.0, pstep)
    v = rng_ref.minstd_next(st1)
    assert st2 == v and F(ip) == F(F(v - 1) / F(2147483648.0)) * F(pstep)
    src, dup, nd = g1.resample_plan(0, ip)
    g1b.resample_plan(0, ip)
    rows_a, zs_a, want3 = std_rows(st2, ZERO6, rc.SIGMA6, nd)
    st3 = g1.resample_apply_drawn(rc.SIGMA6, st2)
    assert st3 == want3
    g1b.resample_apply(rows_a)
    rows_b, zs_b, want4 = std_rows(st3, ZERO6, rc.SIGMA6, n)
    st4 = g1.add_noise_drawn(rc.SIGMA6, st3)
    assert st4 == want4
    mid = g1b.download_state()[0]
    g1b.add_noise(rows_b)
    got, want = g1.download_state()[0], g1b.download_state()[0]
    # bit for bit where the device's rows of both steps equal the standard library's; within the summed bounds elsewhere
    scratch = capi.Group([0])
    try:
        dev_a, _ = device_rows(scratch, st2, rc.SIGMA6, nd)
        dev_b, _ = device_rows(scratch, st3, rc.SIGMA6, n)
    finally:
        scratch.close()
    eq_a = np.ones(n, bool)
    eq_a[dup == 1] = np.all(dev_a[:, [0, 1, 2, 10, 11, 12]] == rows_a[:, [0, 1, 2, 10, 11, 12]], axis=1)
    eq_b = np.all(dev_b[:, [0, 1, 2, 10, 11, 12]] == rows_b[:, [0, 1, 2, 10, 11, 12]], axis=1)
    lin = [0, 1, 2, 7, 8, 9, 10, 11, 12]
    both = eq_a & eq_b
    assert both.sum() > n // 2
    np.testing.assert_array_equal(got[both][:, lin], want[both][:, lin])
    b1 = np.zeros((n, 13))
    b1[dup == 1] = rng_ref.plus_bounds(s[src[dup == 1]], mid[dup == 1], rng_ref.row_bounds(rows_a, zs_a, ZERO6), True)
    b2 = rng_ref.plus_bounds(mid, want, rng_ref.row_bounds(rows_b, zs_b, ZERO6), False)
    total = b1 + b2
    total[:, 3:7] = b2[:, 3:7] + 2.0 * b1[:, 3:7].max(axis=1)[:, None]  # |noise rot| <= 1 + few u, four products per component
    rng_ref.assert_rows_close(got, want, total)


def test_errors_name_the_argument(g1):
    g = capi.Group([0])
    try:
        with pytest.raises(capi.EngineError, match="-5.*no resident particles"):
            g.add_noise_drawn(rc.SIGMA6, 1)
        with pytest.raises(capi.EngineError, match="-5.*no resident particles"):
            g.draw_odom_noise(ODOM_ERR4, 1)
        with pytest.raises(capi.EngineError, match="-5.*no resident particles"):
            g.resample_apply_drawn(rc.SIGMA6, 1)
        g.upload_state(states(8))
        with pytest.raises(capi.EngineError, match="-5.*before group_resample_plan"):
            g.resample_apply_drawn(rc.SIGMA6, 1)
        bad_sigma = rc.SIGMA6.copy()
        bad_sigma[2] = -0.1
        nan_sigma = rc.SIGMA6.copy()
        nan_sigma[4] = np.nan
        for call in (lambda sg, st: g.add_noise_drawn(sg, st), lambda sg, st: g.resample_apply_drawn(sg, st),
                     lambda sg, st: g.init_drawn(IDENTITY7, sg, 8, st)):
            with pytest.raises(capi.EngineError, match=r"-3.*sigma6\[2\]"):
                call(bad_sigma, 1)
            with pytest.raises(capi.EngineError, match=r"-3.*sigma6\[4\]"):
                call(nan_sigma, 1)
            for st in (0, 2 ** 31 - 1, 2 ** 32 - 1):
                with pytest.raises(capi.EngineError, match="-3.*engine_state"):
                    call(rc.SIGMA6, st)
        for st in (0, 2 ** 31 - 1):
            with pytest.raises(capi.EngineError, match="-3.*engine_state"):
                g.draw_odom_noise(ODOM_ERR4, st)
        with pytest.raises(capi.EngineError, match=r"-3.*odom_err4\[1\]"):
            g.draw_odom_noise(np.array([0.1, np.inf, 0.1, 0.1], F), 1)
        bad_mean = IDENTITY7.copy()
        bad_mean[5] = np.nan
        with pytest.raises(capi.EngineError, match=r"-3.*mean7\[5\]"):
            g.init_drawn(bad_mean, rc.SIGMA6, 8, 1)
        with pytest.raises(capi.EngineError, match="-3.*particles"):
            g.init_drawn(IDENTITY7, rc.SIGMA6, 0, 1)
        lib = capi.load_library()
        null = capi.C.POINTER(capi.C.c_uint32)()
        st = capi.C.c_uint32(1)
        assert lib.mcl3dl_hip_group_add_noise_drawn(g.h, None, capi.C.byref(st)) == -3
        assert b"sigma6" in lib.mcl3dl_hip_group_last_error(g.h)
        assert lib.mcl3dl_hip_group_add_noise_drawn(g.h, capi._ptr(rc.SIGMA6), null) == -3
        assert b"engine_state" in lib.mcl3dl_hip_group_last_error(g.h)
        assert lib.mcl3dl_hip_group_init_drawn(g.h, None, capi._ptr(rc.SIGMA6), 8, capi.C.byref(st)) == -3
        assert b"mean7" in lib.mcl3dl_hip_group_last_error(g.h)
        assert lib.mcl3dl_hip_group_draw_odom_noise(g.h, None, capi.C.byref(st)) == -3
        assert b"odom_err4" in lib.mcl3dl_hip_group_last_error(g.h)
        assert np.isnan(capi.rng_uniform(0, 0.0, 1.0)[0])
        # the failed calls left the resident particles alone
        np.testing.assert_array_equal(g.download_state()[0], states(8))
    finally:
        g.close()


def test_likelihood_update_is_left_alone():
    """The noise buffers are the only shared state touched: the same states weigh the same after the drawn calls."""
    sc = make_scene(n=91, n_p=300, n_s=700, n_b=16)
    s = np.zeros((300, 13), F)
    s[:, :7] = sc.poses
    g = capi.Group([0])
    try:
        g.set_map(sc.map_xyz, sc.map_label, stamp=1, dist_weight=(1.0, 1.0, 1.0))
        g.set_likelihood_params()
        g.set_beam_params(num_points=16)
        g.upload_state(s, sc.weights)
        before = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        st = g.draw_odom_noise(ODOM_ERR4, 4242)
        st = g.add_noise_drawn(rc.SIGMA6, st)
        pstep = g.resample_begin()
        ip, st = capi.rng_uniform(st, 0.0, pstep)
        g.resample_plan(0, ip)
        st = g.resample_apply_drawn(rc.SIGMA6, st)
        st = g.init_drawn(IDENTITY7, rc.SIGMA6, 300, st)
        g.upload_state(s, sc.weights)
        after = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        for key in ("weights", "lik", "beam", "quality"):
            np.testing.assert_array_equal(before[key], after[key], err_msg=key)
        assert before["entropy"] == after["entropy"]
    finally:
        g.close()


def test_speed_gates_against_the_long_way_round(g1):
    """At 262 144 particles neither drawn call is slower than drawing on the host and handing the array over. The host draw is the
    reference's own generateNoise loop where oracle/_ref is built, the standard library's stream through the CPU program otherwise
    (a child process: its start is a millisecond against tens of milliseconds of drawing). Not slower is the whole condition."""
    n = 262144
    g1.upload_state(states(n))
    live = pyoracle.available("ref")
    orc = pyoracle.Oracle("ref") if live else None

    def best(f, reps=3):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return min(ts)

    def noise_long_way():
        if live:
            rows = orc.resample_draws(rc.SEED, 1.0, rc.SIGMA6, n)[1]
        else:
            rows = rng_ref.noise_rows(rng_ref.stream("std", "fresh", 12345, 6 * n)[0], ZERO6, rc.SIGMA6, n)[0]
        g1.add_noise(rows)

    def odom_long_way():
        z = rng_ref.stream("std", "shared", 12345, 4 * n)[0].reshape(n, 4)
        g1.set_odom_noise(z[:, [0, 1, 3, 2]] * ODOM_ERR4[[0, 1, 3, 2]])

    g1.add_noise_drawn(rc.SIGMA6, 12345)
    g1.draw_odom_noise(ODOM_ERR4, 12345)
    t_noise_long, t_odom_long = best(noise_long_way), best(odom_long_way)
    t_noise = best(lambda: g1.add_noise_drawn(rc.SIGMA6, 12345), 5)
    t_odom = best(lambda: g1.draw_odom_noise(ODOM_ERR4, 12345), 5)
    print("add_noise_drawn %.3f ms, host draw + add_noise %.3f ms; draw_odom_noise %.3f ms, host stream + set_odom_noise %.3f ms"
          % (t_noise * 1e3, t_noise_long * 1e3, t_odom * 1e3, t_odom_long * 1e3))
    assert t_noise <= t_noise_long, (t_noise, t_noise_long)
    assert t_odom <= t_odom_long, (t_odom, t_odom_long)
