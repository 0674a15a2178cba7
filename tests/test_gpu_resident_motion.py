"""Motion prediction, IMU measurement, odometry noise and the odometry factor on RESIDENT particles
(mcl_3dl_amd/csrc/api_group_motion.inl, motion_kernels.h) against the float32 restatement of the reference's models
(tests/motion_ref.py, itself checked against the reference's own results in tests/test_motion_cpu.py). Every case runs at N = 1
direct, at N = 1 through the sharded path with RCCL, and at N = 3 contexts on the one device through the host, on a particle
count that does not divide evenly."""
import os
import time

import numpy as np
import pytest

import motion_ref as mr
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
N_P = 4099
CONFIGS = [([0], None, 1), ([0], None, 0), ([0, 0, 0], "host", 1)]
IDS = ["n1-direct", "n1-rccl", "n3-host"]
DW = (1.0, 1.0, 5.0)


def states(n, seed, spread=0.2):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 13), np.float32)
    s[:, :3] = rng.uniform(-3, 3, (n, 3))
    q = rng.normal(0, spread, (n, 4))
    q[:, 3] += 1.0
    s[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    s[:, 7:] = rng.normal(0, 0.05, (n, 6))
    return s


def noise4(n, seed):
    return (np.random.default_rng(seed).normal(0, 1, (n, 4)) * np.array([0.1, 0.05, 0.05, 0.1])).astype(np.float32)


def noise13(n, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 13), np.float32)
    a[:, :3] = rng.normal(0, 0.1, (n, 3))
    q = rng.normal(0, 0.03, (n, 4))
    q[:, 3] = 1.0
    a[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    a[:, 7:] = rng.normal(0, 0.01, (n, 6))
    return a


def odom_path(k, seed):
    rng = np.random.default_rng(seed)
    pos, yaw, out = np.zeros(3), 0.1, []
    for _ in range(k):
        prev = np.concatenate([pos, [0, 0, np.sin(yaw / 2), np.cos(yaw / 2)]]).astype(np.float32)
        pos = pos + np.array([np.cos(yaw), np.sin(yaw), 0.0]) * rng.uniform(0.05, 0.2)
        yaw += rng.uniform(-0.1, 0.1)
        cur = np.concatenate([pos, [0, 0, np.sin(yaw / 2), np.cos(yaw / 2)]]).astype(np.float32)
        out.append((prev, cur, float(rng.uniform(0.06, 0.15))))
    return out


def group(cfg):
    devices, collective, direct = cfg
    g = capi.Group(devices, collective=collective)
    g.set_option("direct_single", direct)
    return g


@pytest.fixture(scope="module")
def scene():
    return make_scene(n=91, n_p=N_P, n_s=600, n_b=32, seed=31)


def configure(obj, sc):
    obj.set_map(sc.map_xyz, sc.map_label, stamp=7300, dist_weight=DW)
    obj.set_likelihood_params()
    obj.set_beam_params(num_points=32)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_one_predict_step_and_noise_roundtrip(cfg):
    st, nz = states(N_P, 1), noise4(N_P, 2)
    g = group(cfg)
    try:
        g.upload_state(st)
        np.testing.assert_array_equal(g.download_odom_noise(), 0.0)  # upload_state installs zeros
        g.set_odom_noise(nz)
        np.testing.assert_array_equal(g.download_odom_noise(), nz)
        prev, cur, dt = odom_path(1, 3)[0]
        g.predict(prev, cur, dt, 10.0, 8.0)
        got, _ = g.download_state()
        want = mr.predict(st, nz, mr.motion_step(prev, cur, dt, 10.0, 8.0), host=False)
        np.testing.assert_array_equal(got[:, :3], want[:, :3])
        np.testing.assert_array_equal(got[:, 7:], want[:, 7:])
        np.testing.assert_allclose(got[:, 3:7], want[:, 3:7], rtol=0, atol=4e-7)
        np.testing.assert_array_equal(g.download_odom_noise(), nz)  # predict() leaves the noise as it is
    finally:
        g.close()


def test_fifty_chained_predictions_drift():
    st, nz = states(N_P, 4), noise4(N_P, 5)
    g = group(CONFIGS[0])
    try:
        g.upload_state(st)
        g.set_odom_noise(nz)
        want = st
        for prev, cur, dt in odom_path(50, 6):
            g.predict(prev, cur, dt, 10.0, 10.0)
            want = mr.predict(want, nz, mr.motion_step(prev, cur, dt, 10.0, 10.0), host=False)
        got, _ = g.download_state()
        # the restatement evaluates the same double transcendentals as the device: the chain stays within a few ulp
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    finally:
        g.close()


def shard_local_run(cfg):
    g = group(cfg)
    try:
        g.upload_state(states(N_P, 7))
        g.set_odom_noise(noise4(N_P, 8))
        for prev, cur, dt in odom_path(3, 9):
            g.predict(prev, cur, dt, 10.0, 10.0)
        a, _ = g.download_state()
        g.reset_odom_integ()
        b, _ = g.download_state()
        g.add_noise(noise13(N_P, 10))
        c, _ = g.download_state()
        return a, b, c, g.download_odom_noise()
    finally:
        g.close()


def test_shard_local_calls_identical_over_shards():
    base = shard_local_run(CONFIGS[0])
    assert np.all(base[1][:, 7:] == 0.0)
    np.testing.assert_array_equal(base[3], 0.0)  # operator+ returns a fresh State6DOF
    st_b = base[1]
    want = mr.state_plus(st_b, noise13(N_P, 10))
    np.testing.assert_array_equal(base[2], want)  # add_noise is operator+ bit for bit (no normalize: pf::noise)
    for cfg in CONFIGS[1:]:
        other = shard_local_run(cfg)
        for x, y in zip(base, other):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_pose_mirror_after_predict_and_add_noise(scene, cfg):
    sc = scene
    st = np.zeros((N_P, 13), np.float32)
    st[:, :7] = sc.poses
    g, h = group(cfg), group(cfg)
    try:
        configure(g, sc)
        configure(h, sc)
        g.upload_state(st)
        g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)  # the mirror holds the old poses now
        g.upload_state(st)
        prev, cur, dt = odom_path(1, 11)[0]
        g.set_odom_noise(noise4(N_P, 12))
        g.predict(prev, cur, dt, 10.0, 10.0)
        g.add_noise(noise13(N_P, 13) * np.float32(0.1) + np.array([0, 0, 0, 0, 0, 0, 0.9] + [0] * 6, np.float32))
        moved, w = g.download_state()
        got = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        h.upload_state(moved, w)
        want = h.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        for k in ("lik", "quality", "beam", "weights"):
            np.testing.assert_array_equal(got[k], want[k])
    finally:
        g.close()
        h.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("n_p", [600, N_P])
def test_imu_measure(cfg, n_p, oracle_kind):
    from oracle import pyoracle
    st = states(n_p, 14, spread=0.15)
    rng = np.random.default_rng(15)
    w0 = rng.uniform(0.5, 1.5, n_p).astype(np.float32)
    w0 /= w0.sum()
    acc = np.array([0.3, -0.2, 9.7], np.float32)
    g = group(cfg)
    try:
        g.upload_state(st, w0)
        got = g.measure_imu(acc, 0.5)
        want_lik = mr.imu_likelihood(st, acc, 0.5, host=False)
        np.testing.assert_allclose(got["lik"], want_lik, rtol=2e-6, atol=0)
        assert not got["restored"]
        orc = pyoracle.Oracle(oracle_kind)
        want_w, want_ent, restored = orc.pf_measure(w0, got["lik"])
        assert not restored
        if n_p <= 1024 and cfg[0] == [0]:
            np.testing.assert_array_equal(got["weights"], want_w)  # the float recurrence of pf.h:255-260 (default rule)
        else:
            np.testing.assert_allclose(got["weights"], want_w, rtol=2e-7, atol=1e-12)
        np.testing.assert_allclose(got["entropy"], want_ent, rtol=1e-5)
        _, w_dev = g.download_state()
        np.testing.assert_array_equal(w_dev, got["weights"])
        # every likelihood underflows: restored, weights untouched
        flat = st.copy()
        flat[:, 3:7] = np.array([0.7071068, 0.0, 0.0, 0.7071068], np.float32)
        g.upload_state(flat, w0)
        und = g.measure_imu(np.array([0.0, 0.0, 9.8], np.float32), 1e-3)
        assert und["restored"]
        np.testing.assert_array_equal(und["lik"], 0.0)
        np.testing.assert_array_equal(und["weights"], w0)
    finally:
        g.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_imu_nan_and_underflow_restore_on_the_device(cfg):
    """A NaN likelihood is a real event: ImuMeasurementModelGravity returns one when rounding pushes the acosf argument above 1.
    The reference's own such case (tests/golden/motion.npz, imu2: 30 particles, NaN at particle 0) and its underflow case (imu1:
    every likelihood 0) through measure_imu: the device forms the same NaN, the float sum is NaN resp. 0, and pf::measure restores
    (pf.h:274-278) — also with that one state among 600 particles, on every shard layout."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion.npz"))
    g = group(cfg)
    try:
        for case in (2, 1):
            acc, st, w = G["imu%d_acc" % case], G["imu%d_state" % case], G["imu%d_w" % case]
            want_lik = G["imu%d_lik" % case]
            assert G["imu%d_tail" % case][1] == 1.0
            g.upload_state(st, w)
            got = g.measure_imu(acc[:3], float(acc[3]))
            np.testing.assert_array_equal(np.isnan(got["lik"]), np.isnan(want_lik))
            ok = ~np.isnan(want_lik)
            np.testing.assert_allclose(got["lik"][ok], want_lik[ok], rtol=2e-6, atol=0)
            assert got["restored"] and np.isnan(got["entropy"])
            np.testing.assert_array_equal(got["weights"], w)
            np.testing.assert_array_equal(got["weights"], G["imu%d_wout" % case])   # the reference's own weights after the call
            np.testing.assert_array_equal(g.download_state()[1], w)
            # 600 particles: one NaN among finite likelihoods (particle 311), resp. every particle underflowing
            big = states(600, 14, spread=0.15)
            if case == 2:
                big[311] = st[int(np.nonzero(np.isnan(want_lik))[0][0])]
            else:
                big = np.tile(st, (30, 1))
            w0 = np.random.default_rng(15).uniform(0.5, 1.5, 600).astype(np.float32)
            w0 /= w0.sum()
            g.upload_state(big, w0)
            got = g.measure_imu(acc[:3], float(acc[3]))
            if case == 2:
                assert np.isnan(got["lik"][311]) and np.count_nonzero(np.isnan(got["lik"])) == 1
                assert np.delete(got["lik"], 311).sum() > 0   # (finite and not all zero: without the NaN the update is alive)
            else:
                np.testing.assert_array_equal(got["lik"], 0.0)
            assert got["restored"] and np.isnan(got["entropy"])
            np.testing.assert_array_equal(got["weights"], w0)
            np.testing.assert_array_equal(g.download_state()[1], w0)
    finally:
        g.close()


@pytest.mark.parametrize("strict_order", [1, 2])
@pytest.mark.parametrize("n_p", [600, 1100])
def test_imu_measure_pf_forms_same_bits(n_p, strict_order):
    """pf::measure behind the resident IMU update on one device, in every form it takes there — the fused work-group (600
    particles, pf_fused 1), partial + self-reducing apply (pf_fused 0 or 1100 particles, fp64 sum), partial / reduce / strict sum
    / apply (the float recurrence: strict_order 1, or 2 up to 1024 particles, with pf_fused 0 or beyond pf_fused_max) — gives
    the bits of the context's own pf::measure on the returned likelihoods under the same two options, and the same bits with
    and without the fused kernel (1100: either side of pf_fused_max = 1024, more than four work-groups of 256)."""
    st = states(n_p, 14, spread=0.15)
    w0 = np.random.default_rng(15).uniform(0.5, 1.5, n_p).astype(np.float32)
    w0 /= w0.sum()
    acc = np.array([0.3, -0.2, 9.7], np.float32)
    got = {}
    for pf_fused in (0, 1):
        g, eng = group(([0], None, 1)), capi.Engine(0)
        try:
            for obj in (g, eng):
                obj.set_option("pf_fused", pf_fused)
                obj.set_option("strict_order", strict_order)
            g.upload_state(st, w0)
            got[pf_fused] = g.measure_imu(acc, 0.5)
            want = eng.pf_measure(w0, got[pf_fused]["lik"])
        finally:
            g.close()
            eng.close()
        np.testing.assert_array_equal(got[pf_fused]["weights"], want["weights"])
        assert got[pf_fused]["entropy"] == want["entropy"]
        assert got[pf_fused]["restored"] == want["restored"] and not want["restored"]
    np.testing.assert_array_equal(got[0]["lik"], got[1]["lik"])
    np.testing.assert_array_equal(got[0]["weights"], got[1]["weights"])
    assert got[0]["entropy"] == got[1]["entropy"]
    assert got[0]["restored"] == got[1]["restored"]


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_device_odometry_factor(scene, cfg):
    sc = scene
    st = np.zeros((N_P, 13), np.float32)
    st[:, :7] = sc.poses
    st[:, 7:] = np.random.default_rng(16).normal(0, 0.1, (N_P, 6))
    g = group(cfg)
    try:
        configure(g, sc)
        g.upload_state(st)
        plain = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        g.upload_state(st)
        g.set_odom_error_sigma(0.0)
        zero = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        for k in plain:
            np.testing.assert_array_equal(np.asarray(plain[k]), np.asarray(zero[k]))  # sigma 0: today's NULL, byte for byte
        g.upload_state(st)
        host = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins,
                                 extra=mr.odom_factor(st, 0.2, host=True))
        g.upload_state(st)
        g.set_odom_error_sigma(0.2)
        dev = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        for k in ("lik", "quality", "beam"):
            np.testing.assert_array_equal(dev[k], host[k])
        np.testing.assert_allclose(dev["weights"], host["weights"], rtol=1e-6, atol=1e-12)
        assert not np.array_equal(dev["weights"], plain["weights"])
    finally:
        g.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_noise_lifecycle_through_resampling(cfg):
    st = states(N_P, 17)
    rng = np.random.default_rng(18)
    w = (rng.uniform(0, 1, N_P) ** 4).astype(np.float32)
    w /= w.sum()
    g, plain = group(cfg), group(cfg)
    try:
        # no noise ever installed: the same collectives and the same new generation as a group that never heard of noise
        for x in (g, plain):
            x.upload_state(st, w)
            x.resample_begin()
            src, dup, nd = x.resample_plan(0, 1e-5)
            x.resample_apply(noise13(nd, 19))
        a, b = g.download_state(), plain.download_state()
        np.testing.assert_array_equal(a[0], b[0])
        assert g.collective_stats() == plain.collective_stats()
        np.testing.assert_array_equal(g.download_odom_noise(), 0.0)
        # installed noise travels with its particle; a duplicate holds zeros
        g.upload_state(st, w)
        nz = noise4(N_P, 20)
        g.set_odom_noise(nz)
        g.resample_begin()
        src, dup, nd = g.resample_plan(0, 1e-5)
        assert 0 < nd < N_P
        g.resample_apply(noise13(nd, 21))
        got = g.download_odom_noise()
        want = nz[src].copy()
        want[dup.astype(bool)] = 0.0
        np.testing.assert_array_equal(got, want)
        g.add_noise(noise13(N_P, 22))
        np.testing.assert_array_equal(g.download_odom_noise(), 0.0)
    finally:
        g.close()
        plain.close()


def test_node_loop_against_cpu(scene, oracle_kind):
    """Ten iterations of the node's loop on the device (predict x3, IMU x5, scan update with the device factor, expectation,
    resample, noise redraw, one expansion reset) and on the CPU (oracle + restatement): mean poses agree."""
    from oracle import pyoracle
    sc = scene
    n = 1024
    st = np.zeros((n, 13), np.float32)
    st[:, :7] = sc.poses[:n]
    w = np.full(n, 1.0 / n, np.float32)
    orc = pyoracle.Oracle(oracle_kind)
    orc.set_map(sc.map_xyz, sc.map_label, dist_weight=DW)
    orc.set_likelihood_params(pyoracle.LikelihoodParams())
    orc.set_beam_params(pyoracle.BeamParams(num_points=32))
    g = group(CONFIGS[0])
    rng = np.random.default_rng(23)
    try:
        configure(g, sc)
        g.upload_state(st, w)
        g.set_odom_error_sigma(0.5)
        path = odom_path(30, 24)
        for it in range(10):
            for prev, cur, dt in path[3 * it:3 * it + 3]:
                g.predict(prev, cur, dt, 10.0, 10.0)
                st = mr.predict(st, nz_cpu if it else None, mr.motion_step(prev, cur, dt, 10.0, 10.0), host=False)
            for _ in range(5):
                acc = np.array([rng.normal(0, 0.05), rng.normal(0, 0.05), 9.8], np.float32)
                g.measure_imu(acc, 0.3, fetch=False)
                w, _, _ = orc.pf_measure(w, mr.imu_likelihood(st, acc, 0.3, host=False))
            g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins, fetch=False)
            upd = orc.measure_update(st[:, :7], w, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins,
                                     odom_err=st[:, 7:10], odom_sigma=0.5)
            w = upd["weights"]
            mean_g = g.expectation()[0]
            mean_c = orc.expectation(st[:, :7], w)[0]
            np.testing.assert_allclose(mean_g[:3], mean_c[:3], atol=1e-3)
            q1, q2 = mean_g[3:7], mean_c[3:7]
            assert 2 * np.arccos(min(1.0, abs(float(np.dot(q1, q2))))) < 1e-3
            # resample with caller-drawn noise: the device's plan, applied on the CPU as pf.h:204-223 does
            g.resample_begin()
            src, dup, nd = g.resample_plan(0, float(rng.uniform(0, 1.0 / n)))
            nzr = noise13(nd, 100 + it)
            g.resample_apply(nzr)
            new = st[src].copy()
            d = np.nonzero(dup)[0]
            new[d] = mr.state_plus(st[src[d]], nzr)
            new[d, 3:7] = mr.qnormalized(new[d, 3:7])
            st, w = new, np.full(n, 1.0 / n, np.float32)
            nz_cpu = noise4(n, 200 + it)
            g.set_odom_noise(nz_cpu)
            if it == 4:  # expansion reset: after the redraw, as the node orders them — the next predictions run without noise
                ex = noise13(n, 300)
                g.add_noise(ex)
                st = mr.state_plus(st, ex)
                nz_cpu = np.zeros((n, 4), np.float32)
        s_dev, _ = g.download_state()
        np.testing.assert_allclose(s_dev[:, :3], st[:, :3], atol=1e-3)
    finally:
        g.close()


def test_speed_gate_against_state_round_trip():
    n = 262144
    st = states(n, 25)
    g = group(CONFIGS[0])
    try:
        g.upload_state(st)
        g.set_odom_noise(noise4(n, 26))
        prev, cur, dt = odom_path(1, 27)[0]
        acc = np.array([0.1, 0.0, 9.8], np.float32)
        g.predict(prev, cur, dt)
        g.measure_imu(acc, 0.3, fetch=False)

        def best(f, reps=5):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t0)
            return min(ts)

        def round_trip():
            s, w = g.download_state()
            g.upload_state(s, w)
        rt = best(round_trip)
        t_pred = best(lambda: g.predict(prev, cur, dt))
        t_imu = best(lambda: g.measure_imu(acc, 0.3, fetch=False))
        assert t_pred <= rt / 5, (t_pred, rt)
        assert t_imu <= rt / 5, (t_imu, rt)
    finally:
        g.close()
