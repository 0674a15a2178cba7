"""pf::covariance(1.0, ratio < 1) on the resident particles of a device group (api_shuffle.inl): mcl3dl_hip_group_covariance_sampled
over caller-drawn indices and mcl3dl_hip_group_covariance_drawn with std::shuffle(iota(n), engine_) made from the engine state — on
the devices from 46341 particles on, by the library's serial loop on the host below. Particles and the exact-sum yardstick are
tests/moments_ref.py's; the shuffle's is libstdc++'s own (tests/cpp/rng_shuffle_emul.cpp)."""
import ctypes as C

import numpy as np
import pytest

import moments_ref as mo
import rng_shuffle_ref as rsr
import test_gpu_scan_prepared as sp
from mcl_3dl_amd import capi
from test_gpu_moments_exact import dev, record, within

pytestmark = pytest.mark.gpu
F, D = mo.F, mo.D
WORLDS = {"n1-direct": ([0], None, 1), "n1-sharded": ([0], None, 0), "n2-host": ([0, 0], "host", 1), "n3-host": ([0, 0, 0], "host", 1)}


def make_group(cfg):
    devices, collective, direct = WORLDS[cfg]
    g = capi.Group(devices, collective=collective)
    g.set_option("direct_single", direct)
    return g


@pytest.fixture(scope="module")
def groups():
    made = {}

    def get(cfg):
        if cfg not in made:
            made[cfg] = make_group(cfg)
        return made[cfg]
    yield get
    for g in made.values():
        g.close()


def shard(n, world, r):
    lo, count = capi.group_shard(n, world, r)
    return lo, lo + count


def states13(pose7):
    s = np.zeros((len(pose7), 13), F)
    s[:, :7] = pose7
    return s


# ---- world 1: the single engine's kernel over the same list ------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["n1-direct", "n1-sharded"])
@pytest.mark.parametrize("n,m", [(1025, 257), (300000, mo.CAP + 1)])
def test_one_device_equals_covariance_device(engine, groups, cfg, n, m):
    case = mo.subset_case(n, m)
    g = groups(cfg)
    g.upload_state(states13(case.pose7), case.w)
    got = g.covariance_sampled(case.mean7, case.subset)
    want = engine.covariance_device(dev(case.pose7), dev(case.w), case.n, case.mean7, dev(case.subset), len(case.subset))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, got.T)


# ---- worlds 2 and 3: lists that leave a shard empty, sit in one shard, straddle a shard edge ---------------------------------------
SHARDED_N = 3001  # shards of 1501 + 1500 and of 1001 + 1000 + 1000


def sharded_lists(world):
    rng = np.random.default_rng(17 + world)
    bounds = [shard(SHARDED_N, world, r) for r in range(world)]
    lo1, hi1 = bounds[1]
    last_lo = bounds[-1][0]
    return {
        "last-shard-empty": rng.permutation(last_lo)[:300],                   # no entry in the last rank's shard
        "first-shard-empty": bounds[0][1] + rng.permutation(SHARDED_N - bounds[0][1])[:300],
        "inside-one-shard": lo1 + rng.permutation(hi1 - lo1)[:257],           # rank 1 alone
        "straddles-an-edge": (lo1 - 40) + rng.permutation(80),                # 40 entries on either side of the edge, mixed
        "everywhere": rng.permutation(SHARDED_N)[:1025],
        "whole-shuffle": rng.permutation(SHARDED_N),
    }


@pytest.mark.parametrize("name", list(sharded_lists(3)))
@pytest.mark.parametrize("cfg", ["n2-host", "n3-host"])
def test_shard_records_against_exact_sums(engine, groups, cfg, name):
    world = len(WORLDS[cfg][0])
    sub = sharded_lists(world)[name].astype(np.uint32)
    marks = mo.sentinels(len(sub))
    case = mo.Case(mo.scene_poses(SHARDED_N), mo.sentinel_weights(SHARDED_N, 5 * SHARDED_N, at=sub[marks].astype(np.int64)),
                   subset=sub, marks=marks)
    case.check(moments=False, covariance=True)
    exact, bound = case.covariance()  # (m - 1) fp64 additions in ANY order — shards and the host's rank-order sum included
    terms = case.cov_bounds()[0]
    d_pose, d_w, d_sub = dev(case.pose7), dev(case.w), dev(sub)
    total = np.zeros(22, D)
    in_shard = []
    for r in range(world):
        lo, hi = shard(SHARDED_N, world, r)
        rec = record(engine, 22, lambda out: engine.covariance_window_partial_device(d_pose[lo:hi], d_w[lo:hi], hi - lo, lo,
                                                                                      case.mean7, out, d_sub, len(sub)))
        inside = (sub >= lo) & (sub < hi)
        in_shard.append(int(inside.sum()))
        if not inside.any():
            np.testing.assert_array_equal(rec, np.zeros(22))
        else:  # the shard's own share, against the exact sum of its terms
            t_r = terms[inside]
            b_r = mo.sum_bound(t_r) + mo.cov_budget(case.pose7, case.w, case.mean7, sub[inside])
            within("%s %s rank %d" % (cfg, name, r), rec, mo.exact_sums(t_r), b_r, t_r)
        total = total + rec  # (rank order, as the group adds)
    print("%s %s: entries per shard %s" % (cfg, name, in_shard))
    if name.endswith("shard-empty") or name == "inside-one-shard":
        assert 0 in in_shard
    if name == "straddles-an-edge":
        assert in_shard[0] == 40 and in_shard[1] == 40
    within("%s %s: position sums and sum w" % (cfg, name), total[mo.POSITION_SUMS], exact[mo.POSITION_SUMS], bound[mo.POSITION_SUMS],
           terms[:, mo.POSITION_SUMS])
    within("%s %s: angle sums" % (cfg, name), total[mo.ANGLE_SUMS], exact[mo.ANGLE_SUMS], bound[mo.ANGLE_SUMS],
           terms[:, mo.ANGLE_SUMS])
    g = groups(cfg)
    g.upload_state(states13(case.pose7), case.w)
    cov = g.covariance_sampled(case.mean7, sub)
    np.testing.assert_array_equal(cov, mo.covariance_finish(total))
    np.testing.assert_array_equal(cov, engine.covariance_finish(total))


# ---- the shuffle made by the call ---------------------------------------------------------------------------------------------------
def node_ratio(n, num_particles=64):
    """src/mcl_3dl.cpp:371-373: std::max(0.1f, static_cast<float>(num_particles) / size)"""
    return float(max(F(0.1), F(num_particles) / F(n)))


FLOAT_PRODUCT = (46341, float(F(9268 / 46341)))  # (float)n * ratio = 9268, the double product 9267.9999...
RATIOS = {46341: [0.1, 0.75, FLOAT_PRODUCT[1]], 200001: [0.1, 0.75], 4096: [0.1, 0.75]}
_particles = {}


def particles(n):
    if n not in _particles:
        pose7 = mo.scene_poses(n)
        w = mo.sentinel_weights(n, n + 11)
        mean7 = mo.moments_finish(mo.moment_terms(pose7, w)[0].astype(D).sum(axis=0))[0]
        _particles[n] = (states13(pose7), w, mean7)
    return _particles[n]


@pytest.mark.parametrize("cfg", ["n1-direct", "n3-host"])
@pytest.mark.parametrize("n", [46341, 200001, 4096])
def test_drawn_equals_sampled_over_the_standard_library_s_shuffle(groups, cfg, n):
    s, w, mean7 = particles(n)
    g = groups(cfg)
    g.upload_state(s, w)
    state = 1  # (rejections on the device path: 1 at 46341, 6 at 200001)
    whole, behind, _ = rsr.emul("std", state, n, n)
    ratios = RATIOS[n] + [node_ratio(n)]
    assert node_ratio(n) == float(F(0.1)) and node_ratio(100) == float(F(0.64))
    seen = {}
    for ratio in ratios:
        m = rsr.sample_count(n, ratio)
        cov, n_sampled, st = g.covariance_drawn(mean7, ratio, state)
        assert n_sampled == m and 0 < m < n and st == behind, (n, ratio)
        if m not in seen:
            seen[m] = g.covariance_sampled(mean7, whole[:m])
        np.testing.assert_array_equal(cov, seen[m])
        assert np.all(np.isfinite(cov)) and np.all(np.diag(cov) > 0)
    if n == FLOAT_PRODUCT[0]:
        assert rsr.sample_count(n, FLOAT_PRODUCT[1]) == 9268 and int(float(n) * FLOAT_PRODUCT[1]) == 9267
        assert not np.array_equal(seen[9268], g.covariance_sampled(mean7, whole[:9267]))
    # the order of the list is the shuffle's: the same set in another order is another summation order, not this call's contract
    assert len(seen) == len({rsr.sample_count(n, r) for r in ratios})


@pytest.mark.parametrize("cfg", ["n1-direct", "n3-host"])
def test_ratio_of_one_or_more_draws_nothing(groups, cfg):
    s, w, mean7 = particles(4096)
    g = groups(cfg)
    g.upload_state(s, w)
    want = g.covariance(mean7)
    for ratio in (1.0, 1.5, float("inf")):
        cov, n_sampled, st = g.covariance_drawn(mean7, ratio, 777)
        np.testing.assert_array_equal(cov, want)
        assert (n_sampled, st) == (4096, 777)


@pytest.mark.parametrize("cfg", ["n1-direct", "n3-host"])
def test_errors_leave_the_state(groups, cfg):
    s, w, mean7 = particles(4096)
    g = groups(cfg)
    g.upload_state(s, w)
    lib = g.lib
    m7 = np.ascontiguousarray(mean7, F)
    for ratio in (float("nan"), -0.5, 1e-5):  # 4096 * 1e-5 truncates to 0: the reference divides by zero
        st, ns = C.c_uint32(4242), C.c_size_t(99)
        cov = np.full((6, 6), 7.0, F)
        assert lib.mcl3dl_hip_group_covariance_drawn(g.h, capi._ptr(m7), ratio, C.byref(st), C.byref(ns), capi._ptr(cov)) == -3
        assert st.value == 4242 and ns.value == 99 and np.all(cov == 7.0)
    for state in (0, 2 ** 31 - 1):
        st = C.c_uint32(state)
        assert lib.mcl3dl_hip_group_covariance_drawn(g.h, capi._ptr(m7), 0.5, C.byref(st), None, capi._ptr(np.zeros((6, 6), F))) == -3
        assert st.value == state
    with pytest.raises(capi.EngineError, match="error -3"):
        g.covariance_sampled(mean7, np.array([5, 4096, 7], np.uint32))
    with pytest.raises(capi.EngineError, match="error -3"):
        g.covariance_sampled(mean7, np.zeros(0, np.uint32))
    g.covariance_sampled(mean7, np.array([5, 4095, 7], np.uint32))  # the last particle is one


def test_without_resident_particles():
    g = make_group("n1-direct")
    try:
        with pytest.raises(capi.EngineError, match="error -5"):
            g.covariance_drawn(np.array([0, 0, 0, 0, 0, 0, 1], F), 0.5, 1)
        with pytest.raises(capi.EngineError, match="error -5"):
            g.covariance_sampled(np.array([0, 0, 0, 0, 0, 0, 1], F), np.arange(3, dtype=np.uint32))
    finally:
        g.close()


# ---- what a call in between leaves alone ------------------------------------------------------------------------------------------
def test_what_is_left_alone():
    """Installed scans, a map update, the resampling plan and the odometry noise: a filter step with both calls thrown in between
    its stages, on the device path of the shuffle, gives the bits of the step without them."""
    sc = sp.make_scene(n=91, n_p=300, n_s=1800, n_b=600, seed=41)
    cloud = np.concatenate([sc.scan_lik, sc.scan_beam, sc.scan_lik[::3] + F(0.004)], 0)
    g = sp.make_group(sc, [0, 0, 0], "host", 1)
    try:
        ctxs = [g.context(r) for r in range(3)]
        for c in ctxs:
            c.map_update(sc.scan_lik[:400] + F(0.3), None)
        n_p = 46342
        s, w = sp.states(sc, n_p)
        mean7 = s[0, :7].copy()
        # (the first update behind a map update compiles the map's indices)
        g.upload_state(s, w)
        sp.begin(g, cloud)
        g.scan_finish_drawn(700, 16, sc.origins, 99)
        g.update_resident_prepared()
        stats = [c.index_stats() for c in ctxs]
        assert all(st["build_ms"] > 0 for st in stats)
        calls = []

        def between(do):
            if not do:
                return
            cov, m, st = g.covariance_drawn(mean7, 0.1, 31)
            assert m == 4634
            calls.append((cov, st))
            np.testing.assert_array_equal(g.covariance_sampled(mean7, rsr.emul("std", 31, n_p, n_p)[0][:m]), cov)

        def sequence(do):
            g.upload_state(s, w)
            sp.begin(g, cloud)
            st0 = g.scan_finish_drawn(700, 16, sc.origins, 99)[2]
            between(do)
            first = g.update_resident_prepared()
            between(do)
            pstep = g.resample_begin()
            ip, st = capi.rng_uniform(st0, 0.0, pstep)
            plan = g.resample_plan(0, ip)
            between(do)
            st = g.resample_apply_drawn(sp.SIGMA6, st)
            between(do)
            second = g.update_resident_prepared()
            return first, plan, st, second, g.download_state()

        a, b = sequence(True), sequence(False)
        sp.assert_same_update(a[0], b[0])
        for x, y in zip(a[1], b[1]):
            np.testing.assert_array_equal(x, y)
        assert a[2] == b[2] and a[1][2] > 0
        sp.assert_same_update(a[3], b[3])
        np.testing.assert_array_equal(a[4][0], b[4][0])
        np.testing.assert_array_equal(a[4][1], b[4][1])
        assert [c.index_stats() for c in ctxs] == stats
        assert len(calls) == 4 and all(c[1] == rsr.emul("std", 31, n_p, 1)[1] for c in calls)
    finally:
        g.close()
