"""The normal-weighted scan sampler drawn on the device (mcl_3dl_amd/csrc/double_chain.h, rng_weighted.h, rng_weighted_kernels.h,
host_weighted.h, api_sampler.inl): mcl3dl_hip_rng_draw_weighted, _scan_finish_drawn_normal and the group form.

Yardstick: tests/cpp/rng_weighted_emul.cpp's standard-library path (tests/rng_weighted_ref.py) — the plain cumulative loop, and
std::default_random_engine + std::uniform_real_distribution<double> + std::lower_bound + std::unordered_set<size_t> in the
sampler's loop — fed the cumulative array the existing mcl3dl_hip_scan_normal_weights returns; and the parent's own route,
scan_finish with those ids. Every comparison is bit for bit (a NaN counts as a NaN: rng_weighted_ref.same_doubles)."""
import ctypes as C
import time

import numpy as np
import pytest

import rng_weighted_ref as rwr
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
F = np.float32
R = 0.4
FPC = np.array([0.8, 0.6, 0.0], F)
MAX_WEIGHT = 5.0
WIDE = (0.0, 1.0e6, -1.0e6, 1.0e6)
BEAM_BAND = (0.0, 1.0e6, -0.4, 0.4)       # the beam model's clip keeps a band of both walls
NOTHING = (0.0, 1.0e6, 50.0, 60.0)
LEAF = (0.05, 0.05, 0.05)
CLIP_LIK = (0.5, 10.0, -2.0, 2.0)
CLIP_BEAM = (0.5, 4.0, -2.0, 2.0)
KEYS = ("weights", "lik", "quality", "beam", "entropy", "match_ratio_min", "match_ratio_max", "restored")
ORIGINS = np.zeros((1, 3), F)


def walls(side=40):
    """The upstream sampler test's geometry (tests/sampler_normal_ref.py:walls) with side x side points per wall: two walls at
    x = 20, the second turned about z by pi / 2. 3200 points."""
    ny, nz = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    base = np.stack([np.full(side * side, 20.0), (ny.ravel() - side // 2) * 0.05, (nz.ravel() - side // 2) * 0.05], axis=1)
    base = base.astype(F).astype(np.float64)
    out = []
    for ang in (0.0, np.pi / 2):
        c, s = np.cos(ang), np.sin(ang)
        out.append(np.stack([c * base[:, 0] - s * base[:, 1], s * base[:, 0] + c * base[:, 1], base[:, 2]], axis=1).astype(F))
    return np.concatenate(out)


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def chain_inputs():
    """(kind, n) -> (weights, the plain loop's cumulative array): computed once."""
    out = {}
    for kind in rwr.KINDS:
        for n in rwr.LENGTHS:
            w = rwr.weights(kind, n)
            out[(kind, n)] = (w, rwr.cumsum(w))
    return out


def test_cumulative_equals_the_serial_loop(eng, chain_inputs):
    """num = 0: the chain alone, on any doubles — all-ones, [1, 5], forced ties, terms of half the sum and more, negative terms,
    +-inf, NaN, -0, a denormal; lengths either side of the serial head, of a pass, and 70 000."""
    for (kind, n), (w, want) in chain_inputs.items():
        ids, cum, state, draws = eng.rng_draw_weighted(w, 0, 777)
        assert len(ids) == 0 and state == 777 and draws == 0
        assert rwr.same_doubles(cum, want), (kind, n, np.flatnonzero(cum.view(np.uint64) != want.view(np.uint64))[:5])
    assert np.isnan(chain_inputs[("special", 70000)][1][-1]) and np.isinf(chain_inputs[("special", 70000)][1][50000])


# (1500, 1110): the first count the rounds serve; (5000, 3000): far beyond
@pytest.mark.parametrize("n,num", [(14, 13), (100, 99), (300, 299), (600, 96), (1500, rwr.SINGLE_MAX), (1500, rwr.SINGLE_MAX + 1),
                                   (5000, 3000)])
def test_draw_weighted_equals_the_standard_library(eng, n, num):
    for kind, state in (("rand", 12345), ("ones", 2 ** 31 - 2)):
        w = rwr.weights(kind, n)
        want_cum = rwr.cumsum(w)
        want_ids, want_behind, want_draws, _ = rwr.draw("std", state, want_cum, num)
        ids, cum, behind, draws = eng.rng_draw_weighted(w, num, state)
        assert rwr.same_doubles(cum, want_cum)
        np.testing.assert_array_equal(ids, want_ids)
        assert (behind, draws) == (want_behind, want_draws), (kind, n, num)


def begin_walls(obj, clip_beam=BEAM_BAND):
    cloud = walls()
    n_full, n_lik, n_beam = obj.scan_begin(cloud, None, leaf=None, clip_lik=WIDE, clip_beam=clip_beam)
    assert n_full == n_lik == len(cloud)
    return n_lik, n_beam


def expected(e, n_s, n_b, state):
    """What sample() installs for both models — beam first — from the cumulative arrays the existing call returns:
    (ids_lik, ids_beam, state behind, clipped likelihood cloud, clipped beam cloud)."""
    lik_cloud, beam_cloud = e.scan_download(1)[0], e.scan_download(2)[0]
    cum_b = e.scan_normal_weights(2, R, FPC, MAX_WEIGHT)[0] if len(beam_cloud) > n_b > 0 else None
    ids_b, state = rwr.sample(state, cum_b, len(beam_cloud), n_b)
    cum_l = e.scan_normal_weights(1, R, FPC, MAX_WEIGHT)[0] if len(lik_cloud) > n_s > 0 else None
    ids_l, state = rwr.sample(state, cum_l, len(lik_cloud), n_s)
    return ids_l, ids_b, state, lik_cloud, beam_cloud


def same_points(a, b):
    np.testing.assert_array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def check_installed(e, n_s, n_b, state, clip_beam=BEAM_BAND):
    begin_walls(e, clip_beam)
    ids_l, ids_b, want_behind, lik_cloud, beam_cloud = expected(e, n_s, n_b, state)
    got = e.scan_finish_drawn_normal(n_s, n_b, ORIGINS, R, FPC, MAX_WEIGHT, state)
    assert got == (len(ids_l), len(ids_b), want_behind)
    # the sampled clouds are the gathers of the expected ids, in the container's order
    same_points(e.scan_download(3)[0], lik_cloud[ids_l])
    same_points(e.scan_download(4)[0], beam_cloud[ids_b])
    drawn = [e.scan_download(k) for k in (5, 6)]
    # ... and the installed scans those of scan_finish with these ids
    begin_walls(e, clip_beam)
    e.scan_finish(ids_l, ids_b, origins=ORIGINS)
    for (a, la), (b, lb) in zip(drawn, [e.scan_download(k) for k in (5, 6)]):
        same_points(a, b)
        np.testing.assert_array_equal(la, lb)
    return ids_l, ids_b, want_behind


# (96, 3), (700, 16): one launch for both models; (1200, 16): the likelihood takes the rounds
@pytest.mark.parametrize("n_s,n_b", [(96, 3), (700, 16), (1200, 16)])
def test_scan_finish_drawn_normal_equals_the_reference_sampler(eng, n_s, n_b):
    state = 12345
    ids_l, ids_b, behind = check_installed(eng, n_s, n_b, state)
    assert len(ids_l) == n_s and len(ids_b) == n_b and behind != state
    assert len(set(ids_l.tolist())) == n_s and len(set(ids_b.tolist())) == n_b
    # the weights matter: the first wall faces fpc_local more squarely than the second and is sampled more often
    if n_s == 700:
        assert np.count_nonzero(ids_l < 1600) > np.count_nonzero(ids_l >= 1600) + 30  # (about 390 against 310)
        # the negative: the likelihood drawn first (the order a std::map does NOT give) is another sample
        cum_l = eng.scan_normal_weights(1, R, FPC, MAX_WEIGHT)[0]
        wrong_l, _, _, _ = rwr.draw("std", state, cum_l, n_s)
        assert not np.array_equal(wrong_l, ids_l)


def test_nothing_drawn_and_whole_clouds(eng):
    state = 4242
    # n_b = 0: the likelihood's draws alone, from the start state (origins may be absent then)
    n_lik, n_beam = begin_walls(eng)
    ids_l, _, behind, lik_cloud, _ = expected(eng, 96, 0, state)
    assert eng.scan_finish_drawn_normal(96, 0, None, R, FPC, MAX_WEIGHT, state) == (96, 0, behind)
    same_points(eng.scan_download(3)[0], lik_cloud[ids_l])
    assert len(eng.scan_download(4)[0]) == 0
    # a beam clip that keeps no point: sample() returns empty without drawing, the likelihood starts at the start state
    begin_walls(eng, NOTHING)
    assert eng.scan_finish_drawn_normal(96, 3, ORIGINS, R, FPC, MAX_WEIGHT, state) == (96, 0, behind)
    same_points(eng.scan_download(3)[0], lik_cloud[ids_l])
    # the likelihood cloud no larger than n_s: copied whole in cloud order, no draw — the state is the one behind the beam's draws
    for n_s in (n_lik, n_lik + 5):
        ids_l2, ids_b2, behind2 = check_installed(eng, n_s, 16, state)
        np.testing.assert_array_equal(ids_l2, np.arange(n_lik))
        assert len(ids_b2) == 16 and behind2 == rwr.draw("std", state, eng.scan_normal_weights(2, R, FPC, MAX_WEIGHT)[0], 16)[1]
    # both whole: nothing drawn at all
    begin_walls(eng)
    assert eng.scan_finish_drawn_normal(n_lik, n_beam, ORIGINS, R, FPC, MAX_WEIGHT, state) == (n_lik, n_beam, state)
    same_points(eng.scan_download(3)[0], lik_cloud)
    # neither asked for
    assert eng.scan_finish_drawn_normal(0, 0, ORIGINS, R, FPC, MAX_WEIGHT, state) == (0, 0, state)
    # max_weight = 1: every weight is exactly 1.0, and the sample is the standard library's over 1, 2, 3, ...
    begin_walls(eng)
    want_ids, want_behind, _, _ = rwr.draw("std", state, np.arange(1, n_lik + 1, dtype=np.float64), 96)
    assert eng.scan_finish_drawn_normal(96, 0, None, R, FPC, 1.0, state) == (96, 0, want_behind)
    same_points(eng.scan_download(3)[0], lik_cloud[want_ids])


def configure(obj, sc):
    obj.set_map(sc.map_xyz, sc.map_label, stamp=8300, dist_weight=(1.0, 1.0, 3.0))
    obj.set_likelihood_params()
    obj.set_beam_params(num_points=64)


def test_the_call_leaves_later_calls_scans_indices_and_global_localisation_alone():
    import torch
    sc = make_scene(n=91, n_p=64, n_s=1000, n_b=200, seed=9)
    raw = np.concatenate([sc.scan_lik, sc.scan_beam, sc.scan_lik[::3] + F(0.004)], 0)
    dev = torch.device("cuda", 0)
    e = capi.Engine(0)
    try:
        configure(e, sc)
        points, _ = e.global_localization_points(0.3)
        count = len(points) * 3
        seeded = torch.zeros(count, 13, dtype=torch.float32, device=dev)
        e.global_localization_seed_device(3, 0, count, d_state13=seeded)
        want_seeded = seeded.cpu().numpy()

        def run(with_call):
            n_full, n_lik, n_beam = e.scan_begin(raw, None, leaf=LEAF)
            assert n_lik > 700 and n_beam > 64
            idx_l = np.random.default_rng(11).integers(0, n_lik, 700).astype(np.uint32)
            idx_b = np.random.default_rng(12).integers(0, n_beam, 64).astype(np.uint32)
            clouds = [e.scan_download(k) for k in (0, 1, 2)]
            if with_call:
                assert e.scan_finish_drawn_normal(700, 64, sc.origins, R, FPC, MAX_WEIGHT, 31)[:2] == (700, 64)
                e.rng_draw_weighted(rwr.weights("rand", 5000), 3000, 31)
                for (a, la), (b, lb) in zip(clouds, [e.scan_download(k) for k in (0, 1, 2)]):
                    same_points(a, b)
                    np.testing.assert_array_equal(la, lb)
            later = [e.scan_normal_weights(which, R, FPC, MAX_WEIGHT, normals=True) for which in (0, 1, 2)]
            e.scan_finish(idx_l, idx_b, origins=sc.origins)
            installed = e.scan_download(5), e.scan_download(6)
            d_pose = torch.from_numpy(sc.poses).to(dev)
            d_lik, d_ratio, d_beam = (torch.empty(len(sc.poses), dtype=torch.float32, device=dev) for _ in range(3))
            e.measure_device(d_pose, len(sc.poses), d_lik, d_ratio, d_beam)
            e.synchronize()
            torch.cuda.synchronize()
            return later, installed, (d_lik.cpu().numpy(), d_ratio.cpu().numpy(), d_beam.cpu().numpy())

        plain = run(False)
        stats = e.index_stats()
        assert stats["build_ms"] > 0
        called = run(True)
        for (cum_a, nrm_a, wo_a), (cum_b, nrm_b, wo_b) in zip(plain[0], called[0]):
            np.testing.assert_array_equal(cum_a.view(np.uint64), cum_b.view(np.uint64))
            np.testing.assert_array_equal(nrm_a.view(np.uint32), nrm_b.view(np.uint32))
            assert wo_a == wo_b
        for (a, la), (b, lb) in zip(plain[1], called[1]):
            same_points(a, b)
            np.testing.assert_array_equal(la, lb)
        for a, b in zip(plain[2], called[2]):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.count_nonzero(plain[2][0]) > 32
        assert e.index_stats() == stats  # the map's indices were not rebuilt
        again = torch.zeros(count, 13, dtype=torch.float32, device=dev)
        e.global_localization_seed_device(3, 0, count, d_state13=again)
        np.testing.assert_array_equal(again.cpu().numpy().view(np.uint32), want_seeded.view(np.uint32))
    finally:
        e.close()


def states(sc, n):
    reps = (n + len(sc.poses) - 1) // len(sc.poses)
    s = np.zeros((n, 13), F)
    s[:, :7] = np.tile(sc.poses, (reps, 1))[:n]
    s[:, 10:13] = np.tile(sc.odom_err, (reps, 1))[:n]
    return s, np.full(n, 1.0 / n, F)


def make_group(sc, devices, collective):
    g = capi.Group(devices, collective=collective)
    g.set_option("direct_single", 1)
    configure(g, sc)
    return g


@pytest.mark.parametrize("devices,collective", [([0], None), ([0, 0], "host")])
def test_group_form(devices, collective):
    sc = make_scene(n=91, n_p=300, n_s=1800, n_b=600, seed=41)
    cloud = np.concatenate([sc.scan_lik, sc.scan_beam, sc.scan_lik[::3] + F(0.004)], 0)
    e = capi.Engine(0)
    g = make_group(sc, devices, collective)
    try:
        configure(e, sc)
        state, n_s, n_b = 2024, 700, 16
        kw = dict(leaf=LEAF, clip_lik=CLIP_LIK, clip_beam=CLIP_BEAM)
        n_full, n_lik, n_beam = e.scan_begin(cloud, None, **kw)
        assert n_lik > n_s and n_beam > n_b
        want = e.scan_finish_drawn_normal(n_s, n_b, sc.origins, R, FPC, MAX_WEIGHT, state)
        want_scans = [e.scan_download(k) for k in (3, 4, 5, 6)]
        assert g.scan_begin(cloud, None, **kw) == (n_full, n_lik, n_beam)
        assert g.scan_finish_drawn_normal(n_s, n_b, sc.origins, R, FPC, MAX_WEIGHT, state) == want
        ranks = [g.context(r) for r in range(g.n)]
        for ctx in ranks:
            for k, (a, la) in zip((3, 4, 5, 6), want_scans):
                b, lb = ctx.scan_download(k)
                same_points(a, b)
                np.testing.assert_array_equal(la, lb)
        # the prepared update behind it against update_resident fed the downloaded scans
        n_p = 301 if g.n == 2 else 300
        s, w = states(sc, n_p)
        g.upload_state(s, w)
        got = g.update_resident_prepared()
        g.upload_state(s, w)
        ref = g.update_resident(want_scans[0][0], want_scans[1][0], want_scans[1][1], sc.origins)
        assert np.count_nonzero(ref["lik"]) > n_p // 2
        for k in KEYS:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        if g.n == 2:
            # rank 1 prepares another cloud of the same sizes behind the group's back: its draws end elsewhere on the stream
            g.scan_begin(cloud, None, **kw)
            other = cloud.copy()
            other[:, 2] = other[:, 2] * F(0.5)
            counts = ranks[1].scan_begin(other, None, **kw)
            e.scan_begin(other, None, **kw)
            elsewhere = e.scan_finish_drawn_normal(n_s, n_b, sc.origins, R, FPC, MAX_WEIGHT, state)
            assert elsewhere != want
            st, a, b = C.c_uint32(state), C.c_size_t(0), C.c_size_t(0)
            og, f = np.ascontiguousarray(sc.origins, F), np.ascontiguousarray(FPC)
            rc = g.lib.mcl3dl_hip_group_scan_finish_drawn_normal(g.h, n_s, n_b, capi._ptr(og), len(og), R, capi._ptr(f), MAX_WEIGHT,
                                                                 C.byref(st), C.byref(a), C.byref(b))
            assert rc == -4 and st.value == state, (rc, counts, elsewhere, want)
            # ... and the group works again once every rank holds the same cloud
            g.scan_begin(cloud, None, **kw)
            assert g.scan_finish_drawn_normal(n_s, n_b, sc.origins, R, FPC, MAX_WEIGHT, state) == want
        for ctx in ranks:
            ctx.close()
    finally:
        g.close()
        e.close()


def test_errors_leave_the_engine_state(eng):
    lib = eng.lib

    def raw_weighted(w, num, state, out=True):
        w = np.ascontiguousarray(w, np.float64)
        st = C.c_uint32(state)
        ids = np.zeros(max(num, 1), np.uint32)
        rc = lib.mcl3dl_hip_rng_draw_weighted(eng.h, capi._ptr(w), len(w), num, C.byref(st), capi._ptr(ids) if out else None, None,
                                              None)
        return rc, int(st.value), lib.mcl3dl_hip_last_error(eng.h).decode()

    ones = np.ones(100)
    for w, num, word in ((ones, 100, "copied"), (ones, 101, "copied"), (np.r_[ones, 0.5], 10, "weight"),
                         (np.r_[ones, np.nan], 10, "weight"), (np.r_[ones, np.inf], 10, "weight"), (np.r_[ones, -1.0], 10, "weight"),
                         (np.full(3, 2.0 ** 49), 1, "2\\^50"), (np.r_[np.ones(10), 2.0 ** 50], 3, "2\\^50")):
        rc, st, msg = raw_weighted(w, num, 777)
        assert rc == -3 and st == 777, (rc, st, msg)
        assert __import__("re").search(word, msg), msg
    for bad in (0, 2 ** 31 - 1):
        rc, st, msg = raw_weighted(ones, 10, bad)
        assert rc == -3 and st == bad and "engine_state" in msg, msg
    rc, st, msg = raw_weighted(ones, 10, 777, out=False)
    assert rc == -3 and st == 777 and "out_idx" in msg
    # the largest admitted total still draws
    ids, _, behind, _ = eng.rng_draw_weighted(np.r_[np.full(3, 2.0 ** 48), 1.0], 2, 777)
    assert len(set(ids.tolist())) == 2 and behind != 777

    def raw_finish(e, n_s, n_b, origins, r, fpc, max_weight, state):
        st = C.c_uint32(state)
        og = None if origins is None else np.ascontiguousarray(origins, F)
        f = np.ascontiguousarray(fpc, F)
        rc = lib.mcl3dl_hip_scan_finish_drawn_normal(e.h, n_s, n_b, capi._ptr(og), 0 if og is None else len(og), r, capi._ptr(f),
                                                     max_weight, C.byref(st), None, None)
        return rc, int(st.value), lib.mcl3dl_hip_last_error(e.h).decode()

    fresh = capi.Engine(0)
    try:
        rc, st, msg = raw_finish(fresh, 96, 3, ORIGINS, R, FPC, MAX_WEIGHT, 5)
        assert rc == -5 and st == 5 and "scan_begin" in msg
    finally:
        fresh.close()
    begin_walls(eng)
    for args, word in (((96, 3, ORIGINS, R, FPC, MAX_WEIGHT, 0), "engine_state"),
                       ((96, 3, ORIGINS, R, FPC, MAX_WEIGHT, 2 ** 31 - 1), "engine_state"),
                       ((96, 3, None, R, FPC, MAX_WEIGHT, 5), "origins"),
                       ((96, 3, ORIGINS, 0.0, FPC, MAX_WEIGHT, 5), "normal_search_range"),
                       ((96, 3, ORIGINS, float("nan"), FPC, MAX_WEIGHT, 5), "normal_search_range"),
                       ((96, 3, ORIGINS, R, (0.8, np.nan, 0.0), MAX_WEIGHT, 5), "fpc_local"),
                       ((96, 3, ORIGINS, R, FPC, float("inf"), 5), "max_weight"),
                       ((96, 3, ORIGINS, R, FPC, 0.999, 5), "max_weight"),
                       ((96, 3, ORIGINS, R, FPC, 2.0 ** 45, 5), "2\\^50")):
        rc, st, msg = raw_finish(eng, *args)
        assert rc == -3 and st == args[-1], (args, rc, st, msg)
        assert __import__("re").search(word, msg), msg
    # the engine is usable afterwards
    assert eng.scan_finish_drawn_normal(96, 3, ORIGINS, R, FPC, MAX_WEIGHT, 5)[:2] == (96, 3)


def test_drawn_route_is_not_slower_than_the_long_way_round():
    """4096 particles, 16 384 + 512 points (the larger shape of test_gpu_scan_prepared.py). New: group_scan_finish_drawn_normal +
    update_resident_prepared. Old, the parent's route on the same tree: scan_normal_weights for both models (8 bytes per point come
    home, the host runs the cumulative recurrence), the host's draw, group_scan_finish with the ids, two scan_downloads,
    update_resident with the host scans. The host's draw is the standard library's loop in C++ (g++ -O2) timed inside
    tests/cpp/rng_weighted_emul.cpp, minimum of ten runs, and added to the minimum of ten timed calls of the rest: Python has no
    such loop to put in the timed region, and a child process per call would charge the old route its start-up. Both figures are
    printed on their own. Minimum of ten calls each, no margin."""
    big = make_scene(n=91, n_p=300, n_s=20000, n_b=2000, seed=43)
    cloud = np.concatenate([big.scan_lik, big.scan_beam], 0)
    n_s, n_b = 16384, 512
    g = make_group(big, [0], None)
    try:
        s, w = states(big, 4096)
        g.upload_state(s, w)
        ctx = g.context(0)
        n_full, n_lik, n_beam = g.scan_begin(cloud, None, leaf=LEAF, clip_lik=CLIP_LIK, clip_beam=CLIP_BEAM)
        assert n_lik > n_s and n_beam > n_b, (n_lik, n_beam)
        ids_l, ids_b, want_behind, _, _ = expected(ctx, n_s, n_b, 31)
        cum_b = ctx.scan_normal_weights(2, R, FPC, MAX_WEIGHT)[0]
        cum_l = ctx.scan_normal_weights(1, R, FPC, MAX_WEIGHT)[0]
        t_draw = 1e-3 * (rwr.host_draw_ms(31, cum_b, n_b) + rwr.host_draw_ms(rwr.draw("std", 31, cum_b, n_b)[1], cum_l, n_s))

        def best(f, reps):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t0)
            return min(ts)

        def new_route():
            assert g.scan_finish_drawn_normal(n_s, n_b, big.origins, R, FPC, MAX_WEIGHT, 31)[2] == want_behind
            g.update_resident_prepared(fetch=False)

        def old_route_without_the_draw():
            ctx.scan_normal_weights(2, R, FPC, MAX_WEIGHT)
            ctx.scan_normal_weights(1, R, FPC, MAX_WEIGHT)
            g.scan_finish(ids_l, ids_b, origins=big.origins)
            lik_xyz, _ = ctx.scan_download(3)
            beam_xyz, beam_label = ctx.scan_download(4)
            g.update_resident(lik_xyz, beam_xyz, beam_label, big.origins, fetch=False)

        new_route()
        old_route_without_the_draw()
        t_rest = best(old_route_without_the_draw, 10)
        t_new = best(new_route, 10)
        t_old = t_rest + t_draw
        print("clipped clouds %d / %d; drawn route %.3f ms; long way round %.3f ms = %.3f ms on the device and the bus + %.3f ms "
              "of host draw" % (n_lik, n_beam, 1e3 * t_new, 1e3 * t_old, 1e3 * t_rest, 1e3 * t_draw))
        assert t_new <= t_old, (t_new, t_old)
    finally:
        g.close()
