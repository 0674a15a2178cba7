"""The landmark update, the pose-jump bias inside the moments pass and the single-particle download on RESIDENT particles
(mcl_3dl_amd/csrc/landmark_kernels.h, api_group_motion.inl, api_group_state.inl) against the float32 restatement of the
reference's models (tests/landmark_ref.py, itself checked against the reference's own headers in tests/test_landmark_cpu.py).
Every case runs at N = 1 direct, at N = 1 through the sharded path with RCCL, and at N = 3 contexts on the one device through the
host; at 600 particles (the fused float-order path) and at 4099 (partial + apply; odd, not divisible by three)."""
import math
import time

import numpy as np
import pytest

import landmark_ref as lr
import motion_ref as mr
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
N_P = 4099
SIZES = [600, N_P]
CONFIGS = [([0], None, 1), ([0], None, 0), ([0, 0, 0], "host", 1)]
IDS = ["n1-direct", "n1-rccl", "n3-host"]
VAR_DIST, VAR_ANG = 2.0, 1.57  # the node's defaults for bias_var_dist / bias_var_ang
F = np.float32


def group(cfg):
    devices, collective, direct = cfg
    g = capi.Group(devices, collective=collective)
    g.set_option("direct_single", direct)
    return g


def unit_quats(rng, n, spread):
    q = rng.normal(0.0, spread, (n, 4))
    q[:, 3] += 1.0
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


def rpy_quat(r, p, y):
    t2, t3, t4, t5, t0, t1 = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.array([t0 * t3 * t4 - t1 * t2 * t5, t0 * t2 * t5 + t1 * t3 * t4, t1 * t2 * t4 - t0 * t3 * t5,
                     t0 * t2 * t4 + t1 * t3 * t5])


MEASURED = np.concatenate([[0.5, -1.0, 0.2], rpy_quat(0.05, -0.02, 0.4)]).astype(F)
PREV = np.concatenate([[1.0, -2.0, 0.3], rpy_quat(0.02, -0.03, 0.8)]).astype(F)


def landmark_cov():
    """A full covariance, slightly NON-symmetric so that the column-major convention shows; cov36[6 c + r] = sigma(r, c)."""
    b = np.random.default_rng(40).normal(0, 1, (6, 6))
    cov = np.diag([0.3, 0.25, 0.2, 0.8, 1.2, 0.9]) + 0.02 * (b @ b.T)
    cov[0, 1] += 0.003
    return cov.T.reshape(36).copy()


def landmark_states(n, seed):
    """Particles within about four sigma of MEASURED (normal-float likelihoods); the first 24 pitched to within 1e-3 of +-pi/2
    relative to it with rotations a few ulp longer than 1 (the clamp of t2)."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 13), F)
    s[:, :3] = MEASURED[:3] + rng.normal(0, 0.4, (n, 3))
    s[:, 3:7] = mr.qmul(np.broadcast_to(MEASURED[3:7], (n, 4)), unit_quats(rng, n, 0.25))
    s[:, 7:] = rng.normal(0, 0.05, (n, 6))
    for i in range(24):
        pitch = (1.0 if i % 2 == 0 else -1.0) * (np.pi / 2 - (i // 2) * 8e-5)
        d = rpy_quat(rng.uniform(-0.3, 0.3), pitch, rng.uniform(-0.3, 0.3)) * (1.0 + 2e-7 * (1 + i // 2))
        s[i, 3:7] = mr.qmul(MEASURED[None, 3:7], d.astype(F)[None])[0]
    return s


def bias_states(n, seed):
    """Particles about PREV: rotation == PREV's and == its negation (ang = 0 on both signs of w), ten negated rotations 2 .. 3 rad
    away (w < 0 of the product: the - 2 pi fold), one without any jump."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 13), F)
    s[:, :3] = PREV[:3] + rng.normal(0, 1.0, (n, 3))
    s[:, 3:7] = mr.qmul(unit_quats(rng, n, 0.3), np.broadcast_to(PREV[3:7], (n, 4)))
    s[:, 7:] = rng.normal(0, 0.05, (n, 6))
    s[0, 3:7] = PREV[3:7]
    s[1, 3:7] = -PREV[3:7]
    s[2, :7] = PREV
    for i in range(3, 13):
        ax = rng.normal(0, 1, 3)
        ax /= np.linalg.norm(ax)
        a = rng.uniform(2.0, 3.0)
        d = np.concatenate([ax * np.sin(a / 2), [np.cos(a / 2)]]).astype(F)
        s[i, 3:7] = -mr.qmul(d[None], PREV[None, 3:7])[0]
    return s


def weights(n, seed):
    w = np.random.default_rng(seed).uniform(0.5, 1.5, n).astype(F)
    return (w / w.sum()).astype(F)


def recurrence_error(w0, lik):
    """Relative error of pf::measure's own float recurrence (pf.h:255-260) over the products w0 * lik, against their exact sum."""
    wn = (np.asarray(w0, F) * np.asarray(lik, F)).astype(F)
    s = F(0)
    for v in wn:
        s = F(s + v)
    exact = math.fsum(float(v) for v in wn)
    return abs(float(s) - exact) / exact


def weights_the_recurrence_sums_well(n, lik, seed):
    """Prior weights for the comparison with pyoracle.pf_measure at test_imu_measure's tolerance (rtol 2e-7). Beyond the fused
    float-order path the library adds the products in an fp64 tree, the oracle in the reference's float recurrence, whose own
    rounding error is a random walk of about 4e-7 relative at 600 terms and 1e-6 at 4099 (2.5e-7 and 8.9e-7 on seed 42) —
    common to every weight, and nothing the library computes. The tolerance has room for it only where the recurrence happens to
    land close to the exact sum, as it does on test_imu_measure's data (5e-8 and 7e-8). So the weights are the first seed, counted
    up from `seed`, on which the recurrence over w0 * (the RESTATEMENT's likelihoods) is within 5e-8 of the exact sum: decided on
    the CPU from the reference's arithmetic alone, before the GPU is asked, and asserted."""
    for k in range(64):
        w0 = weights(n, seed + k)
        if recurrence_error(w0, lik) <= 5e-8:
            return w0
    raise AssertionError("no seed on which the reference's float recurrence is within 5e-8 of the exact sum")


def assert_rel(got, want, bound):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.abs(want)
    print("max relative error %.3g, of its bound %.3g" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound), (err.max(), (err / bound).max())


@pytest.fixture(scope="module")
def landmark_ref_results():
    """The restatement's x, likelihoods and bound per particle count: computed once, shared by the configurations."""
    cov = landmark_cov()
    a, sinv = lr.landmark_constants(cov)
    out = {}
    for n in SIZES:
        st = landmark_states(n, 41)
        x = lr.landmark_x(st, MEASURED, host=False)
        t2d = lr.rpy_terms(lr.state_minus(st, MEASURED)[1])[5]
        assert np.any(t2d > 1.0) and np.any(t2d < -1.0)  # the clamp of t2 on both sides
        lik = lr.normal_nd(a, sinv, x, host=False)
        assert np.all(lik > 1e-30)
        out[n] = (st, lik, lr.landmark_bound(x, sinv))
    return cov, out


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("n_p", SIZES)
def test_measure_landmark(cfg, n_p, landmark_ref_results, oracle_kind):
    from oracle import pyoracle
    cov, ref = landmark_ref_results
    st, want_lik, bound = ref[n_p]
    w0 = weights_the_recurrence_sums_well(n_p, want_lik, 42)
    assert recurrence_error(w0, want_lik) <= 5e-8
    g = group(cfg)
    try:
        g.upload_state(st, w0)
        got = g.measure_landmark(MEASURED, cov)
        assert_rel(got["lik"], want_lik, bound)
        assert not got["restored"]
        want_w, want_ent, restored = pyoracle.Oracle(oracle_kind).pf_measure(w0, got["lik"])
        assert not restored
        if n_p <= 1024 and cfg[0] == [0] and cfg[2] == 1:
            np.testing.assert_array_equal(got["weights"], want_w)  # the float recurrence of pf.h:255-260 (default rule)
        else:
            np.testing.assert_allclose(got["weights"], want_w, rtol=2e-7, atol=1e-12)
        np.testing.assert_allclose(got["entropy"], want_ent, rtol=1e-5)
        s_dev, w_dev = g.download_state()
        np.testing.assert_array_equal(w_dev, got["weights"])
        np.testing.assert_array_equal(s_dev, st)  # the update touches nothing but the weights
        # fetch=False leaves the same weights behind
        g.upload_state(st, w0)
        quiet = g.measure_landmark(MEASURED, cov, fetch=False)
        assert quiet["weights"] is None and quiet["entropy"] == got["entropy"]
        np.testing.assert_array_equal(g.download_state()[1], got["weights"])
    finally:
        g.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("n_p", SIZES)
def test_underflow_and_infinite_determinant_restore(cfg, n_p):
    st, w0 = landmark_states(n_p, 43), weights(n_p, 44)
    far = MEASURED.copy()
    far[0] += 50.0
    g = group(cfg)
    try:
        g.upload_state(st, w0)
        # a landmark fifty metres away with a millimetre covariance: every likelihood underflows
        und = g.measure_landmark(far, np.eye(6) * 1e-6)
        assert und["restored"]
        np.testing.assert_array_equal(und["lik"], 0.0)
        np.testing.assert_array_equal(und["weights"], w0)
        np.testing.assert_array_equal(g.download_state()[1], w0)
        # det = 1e42 leaves float range: a_ = 0, every likelihood 0, restored — no error
        inf = g.measure_landmark(MEASURED, np.eye(6) * 1e7)
        assert inf["restored"]
        np.testing.assert_array_equal(inf["lik"], 0.0)
        np.testing.assert_array_equal(inf["weights"], w0)
        np.testing.assert_array_equal(g.download_state()[1], w0)
    finally:
        g.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_rejected_arguments_leave_the_particles_alone(cfg):
    st, w0 = landmark_states(600, 45), weights(600, 46)
    nan_pose = MEASURED.copy()
    nan_pose[4] = np.nan
    bad = {"singular": np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]), "rank-one": np.ones((6, 6)),
           "non-finite": np.diag([1.0, np.nan, 1.0, 1.0, 1.0, 1.0]), "infinite": np.diag([1.0, np.inf, 1.0, 1.0, 1.0, 1.0]),
           "negative-det": np.diag([1.0, -1.0, 1.0, 1.0, 1.0, 1.0])}
    g = group(cfg)
    try:
        for call in (lambda: g.measure_landmark(MEASURED, np.eye(6)), lambda: g.expectation_jump_bias(PREV, VAR_DIST, VAR_ANG),
                     lambda: g.download_particle(0)):
            with pytest.raises(capi.EngineError, match="error -5"):  # nothing resident yet
                call()
        g.upload_state(st, w0)
        for name, cov in bad.items():
            with pytest.raises(capi.EngineError, match="error -3"):
                g.measure_landmark(MEASURED, cov)
        with pytest.raises(capi.EngineError, match="error -3"):
            g.measure_landmark(nan_pose, np.eye(6))
        assert g.lib.mcl3dl_hip_group_measure_landmark(g.h, None, None, None, None, None, None) == -3
        for vd, va in ((0.0, VAR_ANG), (VAR_DIST, -1.0), (np.nan, VAR_ANG), (VAR_DIST, np.inf)):
            with pytest.raises(capi.EngineError, match="error -3"):
                g.expectation_jump_bias(PREV, vd, va)
        with pytest.raises(capi.EngineError, match="error -3"):
            g.expectation_jump_bias(nan_pose, VAR_DIST, VAR_ANG)
        assert g.lib.mcl3dl_hip_group_expectation_jump_bias(g.h, None, 1.0, 1.0, None, None, None, None, None) == -3
        s_dev, w_dev = g.download_state()
        np.testing.assert_array_equal(s_dev, st)
        np.testing.assert_array_equal(w_dev, w0)
    finally:
        g.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_upstream_landmark_kat(cfg):
    """test/src/test_landmark.cpp at upstream's own numbers and tolerances."""
    st, w0, m7, cov = lr.kat_inputs()
    # the seed meets upstream's condition on the CPU, through the restatement, before the GPU is asked
    w_cpu, restored = lr.pf_measure(w0, lr.landmark_likelihood(st, m7, cov, host=False))
    mean, var = lr.weighted_mean_var(st[:, 1], w_cpu)
    assert not restored and abs(mean - 2.3) < 0.1 and abs(var - 0.5) < 0.1, (mean, var)
    g = group(cfg)
    try:
        g.upload_state(st, w0)
        got = g.measure_landmark(m7, cov)
        assert not got["restored"]
        mean, var = lr.weighted_mean_var(st[:, 1], got["weights"])
        assert abs(mean - 2.3) < 0.1, mean
        assert abs(var - 0.5) < 0.1, var
    finally:
        g.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("n_p", SIZES)
def test_jump_bias_inside_the_moments_pass(cfg, n_p):
    st, w0 = bias_states(n_p, 47), weights(n_p, 48)
    want, _, ang, folded = lr.jump_bias(st, PREV, VAR_DIST, VAR_ANG, host=False, parts=True)
    assert ang[0] == 0.0 and ang[1] == 0.0 and folded[3:13].all() and not folded[:3].any()
    g = group(cfg)
    try:
        g.upload_state(st, w0)
        mean, total, imax, ibias, bias = g.expectation_jump_bias(PREV, VAR_DIST, VAR_ANG, fetch_bias=True)
        assert_rel(bias, want, lr.jump_bias_bound(ang, VAR_ANG))
        # the same kernels on the same floats: bit-identical to the expectation over this bias array
        mean2, total2, imax2, ibias2 = g.expectation(bias=bias)
        np.testing.assert_array_equal(mean, mean2)
        assert (total, imax, ibias) == (total2, imax2, ibias2)
        assert imax == int(np.argmax(w0)) and ibias == int(np.argmax((w0 * bias).astype(F)))
        # ... and without fetching the biases
        mean3, total3, imax3, ibias3 = g.expectation_jump_bias(PREV, VAR_DIST, VAR_ANG)
        np.testing.assert_array_equal(mean, mean3)
        assert (total, imax, ibias) == (total3, imax3, ibias3)
        assert not np.array_equal(mean, g.expectation()[0])  # the bias weighs in
    finally:
        g.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_jump_bias_reads_the_resident_particles(cfg):
    """A non-resident update with OTHER poses overwrites the shared pose buffer; the bias still comes from the resident states."""
    sc = make_scene(n=91, n_p=N_P, n_s=64, n_b=0, seed=33)
    st, w0 = bias_states(N_P, 49), weights(N_P, 50)
    g = group(cfg)
    try:
        g.set_map(sc.map_xyz, sc.map_label, stamp=7400, dist_weight=(1.0, 1.0, 5.0))
        g.set_likelihood_params()
        g.upload_state(st, w0)
        g.measure_update(sc.poses, sc.weights, sc.scan_lik)
        mean, total, imax, ibias, bias = g.expectation_jump_bias(PREV, VAR_DIST, VAR_ANG, fetch_bias=True)
        want, _, ang, _ = lr.jump_bias(st, PREV, VAR_DIST, VAR_ANG, host=False, parts=True)
        assert_rel(bias, want, lr.jump_bias_bound(ang, VAR_ANG))
        g.upload_state(st, w0)  # a fresh mirror
        mean2, total2, imax2, ibias2 = g.expectation(bias=bias)
        np.testing.assert_array_equal(mean, mean2)
        assert (total, imax, ibias) == (total2, imax2, ibias2)
    finally:
        g.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_download_particle(cfg):
    st, w0 = bias_states(N_P, 51), weights(N_P, 52)
    g = group(cfg)
    try:
        g.upload_state(st, w0)
        s_all, w_all = g.download_state()
        world = len(cfg[0])
        picks = {0, N_P - 1, g.expectation()[2]}
        for r in range(1, world):
            lo, _ = capi.group_shard(N_P, world, r)
            picks |= {lo - 1, lo}
        for i in sorted(picks):
            s, w = g.download_particle(i)
            np.testing.assert_array_equal(s, s_all[i])
            assert w == w_all[i]
        for i in (N_P, -1, 2 ** 40):
            with pytest.raises(capi.EngineError, match="error -3"):
                g.download_particle(i)
    finally:
        g.close()


def test_speed_gates_against_the_long_way_round():
    """Each long way contains the new call's own device work plus at least 13.6 MB over the bus: not slower, no further margin."""
    n = 262144
    rng = np.random.default_rng(53)
    st = np.zeros((n, 13), F)
    st[:, :3] = rng.uniform(-3, 3, (n, 3))
    st[:, 3:7] = unit_quats(rng, n, 0.2)
    cov = np.diag([9.0, 9.0, 9.0, 1.0, 1.0, 1.0])
    m7 = np.array([0, 0, 0, 0, 0, 0, 1], F)
    host_bias = np.full(n, 0.5, F)  # (the numpy bias itself is not counted)
    g = group(CONFIGS[0])
    try:
        g.upload_state(st)

        def best(f, reps=5):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t0)
            return min(ts)

        def bias_long_way():
            g.download_state()
            g.expectation(bias=host_bias)

        def round_trip():
            s, w = g.download_state()
            g.upload_state(s, w)
        g.expectation_jump_bias(PREV, VAR_DIST, VAR_ANG)
        g.measure_landmark(m7, cov, fetch=False)
        bias_long_way()
        t_long = best(bias_long_way)
        t_bias = best(lambda: g.expectation_jump_bias(PREV, VAR_DIST, VAR_ANG))
        rt = best(round_trip)
        t_lm = best(lambda: g.measure_landmark(m7, cov, fetch=False))
        print("jump bias %.3f ms, download + expectation(bias) %.3f ms; landmark %.3f ms, state round trip %.3f ms"
              % (t_bias * 1e3, t_long * 1e3, t_lm * 1e3, rt * 1e3))
        assert t_bias <= t_long, (t_bias, t_long)
        assert t_lm <= rt, (t_lm, rt)
    finally:
        g.close()
