"""Prepared scans on a device group with the uniform sampler drawn on the devices (mcl_3dl_amd/csrc/rng_index.h,
rng_index_kernels.h, api_cloud.inl, api_group_state.inl): mcl3dl_hip_rng_draw_indices, _scan_finish_drawn, the group's scan_begin /
scan_finish / scan_finish_drawn and _group_update_resident_prepared.

Yardsticks: tests/rng_index_ref.py, the integer restatement of std::uniform_int_distribution<size_t> over
std::default_random_engine that tests/test_rng_index_cpu.py holds against the standard library itself; and the parent's own route —
Engine.scan_begin + scan_finish with host-drawn indices + scan_download 3 / 4 + update_resident with host scans. Every comparison is
bit for bit."""
import time

import numpy as np
import pytest

import rng_index_ref as rir
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
F = np.float32
LEAF = (0.05, 0.05, 0.05)
CLIP_LIK = (0.5, 10.0, -2.0, 2.0)
CLIP_BEAM = (0.5, 4.0, -2.0, 2.0)
DW = (1.0, 1.0, 3.0)
SINGLE_MAX = 65536  # rng_index.h: INDEX_SINGLE_MAX, the most draws the one-work-group kernel serves
SIGMA6 = np.array([0.1, 0.1, 0.05, 0.01, 0.01, 0.05], F)
KEYS = ("weights", "lik", "quality", "beam", "entropy", "match_ratio_min", "match_ratio_max", "restored")


def configure(obj, sc):
    obj.set_map(sc.map_xyz, sc.map_label, stamp=8300, dist_weight=DW)
    obj.set_likelihood_params()
    obj.set_beam_params(num_points=64)


@pytest.fixture(scope="module")
def sc():
    return make_scene(n=91, n_p=300, n_s=1800, n_b=600, seed=41)


@pytest.fixture(scope="module")
def cloud(sc):
    """The accumulated cloud, about 3000 points: the scene's scans with duplicates, in the robot frame."""
    return np.concatenate([sc.scan_lik, sc.scan_beam, sc.scan_lik[::3] + F(0.004)], 0)


@pytest.fixture(scope="module")
def eng(sc):
    """One context of its own: the long way round, and the calls on one context."""
    e = capi.Engine(0)
    configure(e, sc)
    yield e
    e.close()


def make_group(sc, devices, collective, direct):
    g = capi.Group(devices, collective=collective)
    g.set_option("direct_single", direct)
    configure(g, sc)
    return g


@pytest.fixture(scope="module")
def g1(sc):
    g = make_group(sc, [0], None, 1)
    yield g
    g.close()


@pytest.fixture(scope="module")
def g3(sc):
    """Three contexts on the one device, combined through the host: uneven shards at 300 + 1 particles."""
    g = make_group(sc, [0, 0, 0], "host", 1)
    yield g
    g.close()


@pytest.fixture(scope="module")
def g1s(sc):
    """One device that takes the sharded path too."""
    g = make_group(sc, [0], None, 0)
    yield g
    g.close()


@pytest.fixture(params=["n1-direct", "n3-host", "n1-sharded"])
def group(request, g1, g3, g1s):
    return {"n1-direct": g1, "n3-host": g3, "n1-sharded": g1s}[request.param]


def states(sc, n=None):
    n = len(sc.poses) if n is None else n
    reps = (n + len(sc.poses) - 1) // len(sc.poses)
    s = np.zeros((n, 13), F)
    s[:, :7] = np.tile(sc.poses, (reps, 1))[:n]
    s[:, 10:13] = np.tile(sc.odom_err, (reps, 1))[:n]
    w = np.full(n, 1.0 / n, F)
    return s, w


def begin(obj, cloud):
    n_full, n_lik, n_beam = obj.scan_begin(cloud, None, leaf=LEAF, clip_lik=CLIP_LIK, clip_beam=CLIP_BEAM)
    assert n_lik > 0 and n_beam > 0 and n_lik != n_beam
    return n_lik, n_beam


def long_way(eng, g, cloud, idx_l, idx_b, origins, extra=None, fetch=True):
    """The parent's route: prepare on one context, fetch the sampled clouds, hand them to the group as host scans."""
    eng.scan_begin(cloud, None, leaf=LEAF, clip_lik=CLIP_LIK, clip_beam=CLIP_BEAM)
    eng.scan_finish(idx_l, idx_b, origins=origins)
    lik_xyz, _ = eng.scan_download(3)
    beam_xyz, beam_label = eng.scan_download(4)
    return g.update_resident(lik_xyz, beam_xyz, beam_label, origins, extra=extra, fetch=fetch)


def assert_same_update(got, want):
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("n", [1, 3, 4089, 1500000000, 2147483646])
def test_draw_indices_against_the_restatement(eng, n):
    """Values and the engine state behind, at counts either side of a wavefront, of a work-group's 2048 attempts and of the
    one-work-group constant."""
    for count, state in ((1, 12345), (64, 1), (257, rir.A_INV), (5000, rir.BEFORE_MAX), (SINGLE_MAX + 4465, 109)):
        got, behind = eng.rng_draw_indices(n, count, state)
        want, want_behind = rir.draw(state, n, count)
        np.testing.assert_array_equal(got, want)
        assert behind == want_behind, (n, count)
    none, behind = capi.rng_draw_indices(eng, n, 0, 777)
    assert len(none) == 0 and behind == 777


def test_second_round(eng):
    """The triples whose first round falls short (tests/test_rng_index_cpu.py asserts that they do)."""
    for state, n, count in rir.SECOND_ROUND:
        got, behind = eng.rng_draw_indices(n, count, state)
        want, want_behind = rir.draw(state, n, count)
        np.testing.assert_array_equal(got, want)
        assert behind == want_behind


def installed(e, n_p_poses):
    """Everything the installed scans decide: downloads 3-6, the order, and an update / a measure on device arrays."""
    import torch
    dev = torch.device("cuda", 0)
    out = [e.scan_download(k) for k in (3, 4, 5, 6)]
    n_s = len(out[2][0])
    out.append(e.scan_order(n_s) if n_s else np.zeros(0, np.uint32))
    n_p = len(n_p_poses)
    d_pose = torch.from_numpy(n_p_poses).to(dev)
    d_lik, d_ratio, d_beam = (torch.empty(n_p, dtype=torch.float32, device=dev) for _ in range(3))
    e.measure_device(d_pose, n_p, d_lik, d_ratio, d_beam)
    e.synchronize()
    out.append((d_lik.cpu().numpy(), d_ratio.cpu().numpy(), d_beam.cpu().numpy()))
    d_w = torch.full((n_p,), 1.0 / n_p, dtype=torch.float32, device=dev)
    d_st = torch.zeros(4, dtype=torch.float32, device=dev)
    e.update_device(d_pose, n_p, d_w, d_st, d_lik=d_lik, d_ratio=d_ratio, d_beam=d_beam)
    e.synchronize()
    out.append((d_w.cpu().numpy(), d_st.cpu().numpy(), d_lik.cpu().numpy(), d_ratio.cpu().numpy(), d_beam.cpu().numpy()))
    return out


def assert_same_installed(got, want):
    for a, b in zip(got, want):
        for x, y in zip(a, b) if isinstance(a, tuple) else ((a, b),):
            np.testing.assert_array_equal(x, y)


# (700, 16) and (96, 3): the one-work-group kernel; (SINGLE_MAX, 16): the first size that takes the rounds per model
@pytest.mark.parametrize("n_s,n_b", [(96, 3), (700, 16), (SINGLE_MAX, 16)])
def test_scan_finish_drawn_equals_scan_finish_with_host_drawn_indices(eng, sc, cloud, n_s, n_b):
    state = 12345
    n_lik, n_beam = begin(eng, cloud)
    idx_l, idx_b, want_behind = rir.scan_draws(state, n_s, n_lik, n_b, n_beam)
    eng.scan_finish(idx_l, idx_b, origins=sc.origins)
    want = installed(eng, sc.poses)
    begin(eng, cloud)
    assert eng.scan_finish_drawn(n_s, n_b, sc.origins, state) == (n_s, n_b, want_behind)
    got = installed(eng, sc.poses)
    assert_same_installed(got, want)
    if n_s == 700:
        # the negative: the likelihood's draws first (the order a std::map does NOT give) is another sample
        wrong_l, st = rir.draw(state, n_lik, n_s)
        wrong_b, _ = rir.draw(st, n_beam, n_b)
        assert not np.array_equal(wrong_l, idx_l) and not np.array_equal(wrong_b, idx_b)
        begin(eng, cloud)
        eng.scan_finish(wrong_l, wrong_b, origins=sc.origins)
        assert not np.array_equal(eng.scan_download(3)[0], got[0][0])


def test_nothing_drawn(eng, sc, cloud):
    state = 4242
    n_lik, n_beam = begin(eng, cloud)
    # n_b = 0: the likelihood's draws alone, from the start state (origins may be absent then)
    want_l, want_behind = rir.draw(state, n_lik, 96)
    assert eng.scan_finish_drawn(96, 0, None, state) == (96, 0, want_behind)
    eng.scan_finish(want_l, None, origins=sc.origins)
    ref_cloud = eng.scan_download(3)[0]
    eng.scan_finish_drawn(96, 0, None, state)
    np.testing.assert_array_equal(eng.scan_download(3)[0], ref_cloud)
    assert len(eng.scan_download(4)[0]) == 0
    # n_s = 0: the beam's alone
    want_b, want_behind = rir.draw(state, n_beam, 16)
    assert eng.scan_finish_drawn(0, 16, sc.origins, state) == (0, 16, want_behind)
    assert len(eng.scan_download(3)[0]) == 0 and len(eng.scan_download(4)[0]) == 16
    # neither: the state does not move
    assert eng.scan_finish_drawn(0, 0, sc.origins, state) == (0, 0, state)
    # a beam clip that keeps no point: sample() returns empty without drawing, the likelihood's draws start at the start state
    n_full, n_lik2, n_beam2 = eng.scan_begin(cloud, None, leaf=LEAF, clip_lik=CLIP_LIK, clip_beam=(0.5, 4.0, 50.0, 60.0))
    assert n_lik2 == n_lik and n_beam2 == 0
    want_l, want_behind = rir.draw(state, n_lik, 96)
    assert eng.scan_finish_drawn(96, 3, sc.origins, state) == (96, 0, want_behind)
    np.testing.assert_array_equal(eng.scan_download(3)[0], ref_cloud)
    # both clips empty
    eng.scan_begin(cloud, None, leaf=LEAF, clip_lik=(0.5, 10.0, 50.0, 60.0), clip_beam=(0.5, 4.0, 50.0, 60.0))
    assert eng.scan_finish_drawn(96, 3, sc.origins, state) == (0, 0, state)


@pytest.mark.parametrize("variant", ["plain", "extra", "odom-sigma"])
def test_prepared_update_equals_the_long_way_round(group, eng, sc, cloud, variant):
    g = group
    n_p = 301 if g.n == 3 else 300  # (uneven shards on three ranks)
    s, w = states(sc, n_p)
    extra = np.random.default_rng(7).uniform(0.2, 1.0, n_p).astype(F) if variant == "extra" else None
    g.set_odom_error_sigma(0.3 if variant == "odom-sigma" else 0.0)
    try:
        state = 2024
        g.upload_state(s, w)
        n_lik, n_beam = begin(g, cloud)
        idx_l, idx_b, want_behind = rir.scan_draws(state, 700, n_lik, 16, n_beam)
        assert g.scan_finish_drawn(700, 16, sc.origins, state) == (700, 16, want_behind)
        got = g.update_resident_prepared(extra=extra)
        # the installed scans stay: a second update on them from the same particles gives the same bits
        g.upload_state(s, w)
        again = g.update_resident_prepared(extra=extra)
        assert_same_update(again, got)
        # caller-drawn indices through the group's scan_finish
        g.upload_state(s, w)
        begin(g, cloud)
        g.scan_finish(idx_l, idx_b, origins=sc.origins)
        assert_same_update(g.update_resident_prepared(extra=extra), got)
        g.upload_state(s, w)
        want = long_way(eng, g, cloud, idx_l, idx_b, sc.origins, extra=extra)
        assert np.count_nonzero(want["lik"]) > n_p // 2 and np.count_nonzero(want["beam"]) > n_p // 2
        assert_same_update(got, want)
    finally:
        g.set_odom_error_sigma(0.0)


def test_prepared_route_across_a_resampling(group, eng, sc, cloud):
    g = group
    s, w = states(sc, 300)
    n_lik, n_beam = begin(eng, cloud)
    idx_l, idx_b, st0 = rir.scan_draws(99, 700, n_lik, 16, n_beam)

    def sequence(prepared):
        g.upload_state(s, w)
        if prepared:
            begin(g, cloud)
            assert g.scan_finish_drawn(700, 16, sc.origins, 99)[2] == st0

        def update():
            return g.update_resident_prepared() if prepared else long_way(eng, g, cloud, idx_l, idx_b, sc.origins)
        first = update()
        pstep = g.resample_begin()
        ip, st = capi.rng_uniform(st0, 0.0, pstep)
        plan = g.resample_plan(0, ip)
        st = g.resample_apply_drawn(SIGMA6, st)
        second = update()
        return first, plan, st, second, g.download_state()

    a, b = sequence(True), sequence(False)
    assert_same_update(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)
    assert a[2] == b[2] and a[1][2] > 0
    assert_same_update(a[3], b[3])
    np.testing.assert_array_equal(a[4][0], b[4][0])
    np.testing.assert_array_equal(a[4][1], b[4][1])


def test_what_is_left_alone(g3, eng, sc, cloud):
    g = g3
    s, w = states(sc, 301)
    host = (sc.scan_lik[:500], sc.scan_beam[:24], sc.scan_beam_label[:24], sc.origins)
    g.upload_state(s, w)
    before = g.update_resident(*host)
    ctx0 = g.context(0)
    stats, footprint = ctx0.index_stats(), ctx0.memory_footprint()
    assert stats["build_ms"] > 0
    n_lik, n_beam = begin(g, cloud)
    # the calls on rank 0's context keep working behind the group's scan_begin: the normal-weighted sampler's weights, and with
    # them caller-drawn indices through the group's scan_finish
    assert len(ctx0.scan_download(1)[0]) == n_lik and len(ctx0.scan_download(2)[0]) == n_beam
    cum, _, _ = ctx0.scan_normal_weights(1, 0.4, np.array([0.0, 0.0, 1.0], F), 5.0)
    # (every weight is at least 1; differencing the running double sum gives it back to within its rounding, ~1e-12 here)
    assert len(cum) == n_lik and np.all(np.diff(cum) >= 1.0 - 1e-9)
    u = np.random.default_rng(3).uniform(0.0, cum[-1], 96)
    g.scan_finish(np.searchsorted(cum, u, "left").astype(np.uint32), np.arange(3, dtype=np.uint32), origins=sc.origins)
    g.upload_state(s, w)
    g.update_resident_prepared()
    g.scan_finish_drawn(700, 16, sc.origins, 5)
    g.upload_state(s, w)
    g.update_resident_prepared()
    # the map's indices were not rebuilt
    assert ctx0.index_stats() == stats and ctx0.memory_footprint() == footprint
    g.upload_state(s, w)
    after = g.update_resident(*host)
    assert_same_update(after, before)
    assert ctx0.index_stats() == stats and ctx0.memory_footprint() == footprint
    # a host-scan update replaced the installed scans, as before
    assert len(ctx0.scan_download(5)[0]) == 500
    ctx0.close()
    assert g.resident() == 301  # (closing the borrowed Engine left the group's context alone)


def test_errors_name_the_argument_and_leave_the_state(eng, sc, cloud):
    import ctypes as C
    lib = eng.lib

    def raw_draw(n, count, state):
        st = C.c_uint32(state)
        out = np.zeros(max(count, 1), np.uint32)
        rc = lib.mcl3dl_hip_rng_draw_indices(eng.h, n, count, C.byref(st), capi._ptr(out))
        return rc, int(st.value), lib.mcl3dl_hip_last_error(eng.h).decode()

    for n in (0, 2 ** 31 - 1):
        rc, st, msg = raw_draw(n, 5, 777)
        assert rc == -3 and st == 777 and "range" in msg, msg
    for bad in (0, 2 ** 31 - 1):
        rc, st, msg = raw_draw(96, 5, bad)
        assert rc == -3 and st == bad and "engine_state" in msg, msg
    assert lib.mcl3dl_hip_rng_draw_indices(eng.h, 96, 5, None, None) == -3
    assert "engine_state" in lib.mcl3dl_hip_last_error(eng.h).decode()
    begin(eng, cloud)
    with pytest.raises(capi.EngineError, match="-3.*engine_state"):
        eng.scan_finish_drawn(96, 3, sc.origins, 0)
    with pytest.raises(capi.EngineError, match="-3.*origins"):
        eng.scan_finish_drawn(96, 3, None, 5)
    st = C.c_uint32(5)
    assert lib.mcl3dl_hip_scan_finish_drawn(eng.h, 96, 3, None, 0, C.byref(st), None, None) == -3 and st.value == 5
    fresh = capi.Engine(0)
    try:
        with pytest.raises(capi.EngineError, match="-5.*scan_begin"):
            fresh.scan_finish_drawn(96, 3, sc.origins, 5)
    finally:
        fresh.close()
    g = make_group(sc, [0, 0, 0], "host", 1)
    try:
        s, w = states(sc, 30)
        with pytest.raises(capi.EngineError, match="-5.*no resident particles"):
            g.update_resident_prepared()
        g.upload_state(s, w)
        with pytest.raises(capi.EngineError, match="-5.*rank 0 holds no installed scan"):
            g.update_resident_prepared()
        with pytest.raises(capi.EngineError, match="-5.*scan_begin"):
            g.scan_finish_drawn(96, 3, sc.origins, 5)
        begin(g, cloud)
        with pytest.raises(capi.EngineError, match="-3.*engine_state"):
            g.scan_finish_drawn(96, 3, sc.origins, 2 ** 31 - 1)
        with pytest.raises(capi.EngineError, match="-3.*origins"):
            g.scan_finish_drawn(96, 3, None, 5)
        g.scan_finish_drawn(96, 3, sc.origins, 5)
        g.update_resident_prepared()
        # rank 1 gets another scan behind the group's back
        r1 = g.context(1)
        r1.upload_scan(sc.scan_lik[:50])
        with pytest.raises(capi.EngineError, match="-5.*rank 1 holds a scan of 50 \\+ 0"):
            g.update_resident_prepared()
        g.scan_finish_drawn(96, 3, sc.origins, 5)
        g.update_resident_prepared()
    finally:
        g.close()


def test_prepared_route_is_not_slower_than_the_long_way_round(sc):
    """4096 particles, 16 384 + 512 points. New: group_scan_finish_drawn + update_resident_prepared. Old, the parent's route on the
    same tree: scan_finish with indices drawn outside the timed region + two scan_downloads + update_resident with the host scans.
    The new route removes two downloads, one upload and two synchronisations and adds one small launch: no margin."""
    big = make_scene(n=91, n_p=300, n_s=20000, n_b=2000, seed=43)
    cloud = np.concatenate([big.scan_lik, big.scan_beam], 0)
    n_s, n_b = 16384, 512
    g = make_group(big, [0], None, 1)
    try:
        s, w = states(big, 4096)
        g.upload_state(s, w)
        ctx = g.context(0)
        n_lik, n_beam = begin(g, cloud)
        idx_l, idx_b, _ = rir.scan_draws(31, n_s, n_lik, n_b, n_beam)

        def best(f, reps):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t0)
            return min(ts)

        def new_route():
            g.scan_finish_drawn(n_s, n_b, big.origins, 31)
            g.update_resident_prepared(fetch=False)

        def old_route():
            ctx.scan_finish(idx_l, idx_b, origins=big.origins)
            lik_xyz, _ = ctx.scan_download(3)
            beam_xyz, beam_label = ctx.scan_download(4)
            g.update_resident(lik_xyz, beam_xyz, beam_label, big.origins, fetch=False)

        new_route()
        old_route()
        t_old = best(old_route, 3)
        t_new = best(new_route, 5)
        print("prepared route %.3f ms, long way round %.3f ms" % (1e3 * t_new, 1e3 * t_old))
        assert t_new <= t_old, (t_new, t_old)
    finally:
        g.close()
