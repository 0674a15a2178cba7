"""Resampling the resident particles in one call (mcl_3dl_amd/csrc/float_prefix.h, resample_prefix_kernels.h, api_resample.inl,
api_group_state.inl, api_rng.inl): mcl3dl_hip_float_prefix, _resample_plan_device, _group_resample_drawn, _group_resize_resident.

Yardsticks: a numpy float32 loop for the chain; the three-call sequence group_resample_begin / _plan / _apply[_drawn] on a second
group for everything else — both routes run the same kernels behind the plan and draw the noise with the same device code, so
every comparison is assert_array_equal; the goldens of tests/golden/resample.npz (the reference's own plan and states) for the
tie route; oracle/_ref's pf::resample / resizeParticle where it is built, within tests/rng_ref.py's bounds for drawn rows."""
import os
import time

import numpy as np
import pytest

import resample_cases as rc
import rng_ref
from float_chain_cases import prefix_loop, tie_constant   # the plain float32 loop; 1 / n as a tie on every step of one binade
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene
from oracle import pyoracle

pytestmark = pytest.mark.gpu
F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "resample.npz"))
ZERO6 = np.zeros(6, F)
IDENTITY7 = np.array([0, 0, 0, 0, 0, 0, 1], F)
ODOM_ERR4 = np.array([0.2, 0.05, 0.1, 0.3], F)


@pytest.fixture(scope="module")
def g1():
    """The group under test."""
    g = capi.Group([0])
    yield g
    g.close()


@pytest.fixture(scope="module")
def g1b():
    """A second group of one: the three-call sequence."""
    g = capi.Group([0])
    yield g
    g.close()


@pytest.fixture(scope="module")
def g3():
    """Three contexts on the one device, combined through the host: uneven shards at 1000 particles."""
    g = capi.Group([0, 0, 0], collective="host")
    yield g
    g.close()


@pytest.fixture(scope="module")
def g1r():
    """One rank through the sharded path: RCCL runs ncclAllGather with one rank for the weights, the states and the noise."""
    g = capi.Group([0])
    g.set_option("direct_single", 0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


def states(n, seed=5):
    rng = np.random.default_rng(seed)
    s = rng.normal(0, 1, (n, 13)).astype(F)
    s[:, 3:7] /= np.linalg.norm(s[:, 3:7], axis=1, keepdims=True)
    return s


def tie_free(n):
    """U(0.5, 1.5) / sum, seed = n: every weight is far above half an ulp of the running sum (>= 1 / (3 n) against 2^-25)."""
    w = np.random.default_rng(n).uniform(0.5, 1.5, n)
    return (w / w.sum()).astype(F)


def has_ties(w):
    keys = prefix_loop(w)
    return bool(np.any(~(keys[:-1] < keys[1:])))


def three_call(g, sigma6, st, n_out=0):
    """pf::resample the long way round; what there is to compare afterwards."""
    pstep = g.resample_begin(n_out)
    ip, st = capi.rng_uniform(st, 0.0, pstep)
    src, dup, nd = g.resample_plan(0, ip)
    st = g.resample_apply_drawn(sigma6, st)
    s, w = g.download_state()
    return dict(pstep=F(pstep), ip=F(ip), nd=nd, state=st, src=src, dup=dup, s=s, w=w, odom=g.download_odom_noise())


def one_call(g, sigma6, st):
    pstep, ip, nd, st, route = g.resample_drawn(sigma6, st)
    s, w = g.download_state()
    return dict(pstep=F(pstep), ip=F(ip), nd=nd, state=st, route=route, s=s, w=w, odom=g.download_odom_noise())


def assert_same(one, three):
    for key in ("pstep", "ip", "nd", "state"):
        assert one[key] == three[key], key
    for key in ("s", "w", "odom"):
        np.testing.assert_array_equal(one[key], three[key], err_msg=key)


# ---- the chain on its own ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 3000, 4097])
def test_float_prefix_is_the_serial_loop(eng, n):
    w = tie_free(n)
    np.testing.assert_array_equal(eng.float_prefix(w).view(np.uint32), prefix_loop(w).view(np.uint32))
    c = tie_constant(n, 9) if n == 3000 else F(1.0) / F(n)   # (3000: a rounding tie at every step of one binade)
    want = prefix_loop(np.full(n, c, F))
    np.testing.assert_array_equal(eng.float_prefix(None, c, n).view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(eng.float_prefix(np.full(n, c, F)).view(np.uint32), want.view(np.uint32))
    # a NaN and a negative term: the serial path, wherever they sit
    for pos in sorted({0, n // 2, n - 1}):
        for special in (np.nan, -0.125, 0.0, -0.0, 7.0):
            x = w.copy()
            x[pos] = special
            np.testing.assert_array_equal(eng.float_prefix(x).view(np.uint32), prefix_loop(x).view(np.uint32),
                                          err_msg="%r at %d" % (special, pos))


# ---- pf::resample in one call, tie-free ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 65, 257, 600, 1500, 4097, 70001])
def test_resample_drawn_equals_the_three_calls(g1, g1b, n):
    s, w = states(n), tie_free(n)
    assert not has_ties(w)
    st0 = capi.rng_seed(n)
    with_odom = n in (65, 1500)
    for g in (g1, g1b):
        g.upload_state(s, w)
        if with_odom:
            g.draw_odom_noise(ODOM_ERR4, 4242)
    one, three = one_call(g1, rc.SIGMA6, st0), three_call(g1b, rc.SIGMA6, st0)
    assert one["route"] == 0
    assert_same(one, three)
    np.testing.assert_array_equal(one["w"], F(1.0) / F(n))
    assert one["pstep"] == F(prefix_loop(w)[-1] / F(n))
    src, dup = three["src"], three["dup"]
    copied = dup == 0
    np.testing.assert_array_equal(one["s"][copied], s[src[copied]])
    if with_odom:
        assert one["odom"].any() and np.all(one["odom"][dup == 1] == 0)
    if pyoracle.available("ref") and n <= 4097:
        # the reference itself: engine(seed), one uniform, generateNoise per duplicated slot
        want, want_w = pyoracle.Oracle("ref").resample(s, w, n, rc.SIGMA6)
        np.testing.assert_array_equal(one["w"], want_w)
        np.testing.assert_array_equal(one["s"][copied], want[copied])
        nd = one["nd"]
        if nd:
            _, st1 = capi.rng_uniform(st0, 0.0, float(one["pstep"]))
            z, behind, _ = rng_ref.stream("std", "fresh", st1, 6 * nd)
            assert one["state"] == behind
            rows, zs = rng_ref.noise_rows(z, ZERO6, rc.SIGMA6, nd)
            scratch = capi.Group([0])
            try:
                scratch.init_drawn(IDENTITY7, rc.SIGMA6, nd, st1)
                dev = scratch.download_state()[0]
            finally:
                scratch.close()
            equal = np.all(dev == rows, axis=1)
            bound = rng_ref.plus_bounds(s[src[dup == 1]], want[dup == 1], rng_ref.row_bounds(rows, zs, ZERO6), True)
            rng_ref.assert_rows_close(one["s"][dup == 1], want[dup == 1], bound, equal)


# ---- the tie route --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dead", rc.CASES)
def test_tie_route_against_the_goldens(g1, g1b, n, dead):
    s, w = rc.make_case(n, dead)
    key = "n%d_d%d" % (n, dead)
    st0 = capi.rng_seed(rc.SEED)
    g1.upload_state(s, w)
    g1b.upload_state(s, w)
    one, three = one_call(g1, rc.SIGMA6, st0), three_call(g1b, rc.SIGMA6, st0)
    assert one["route"] == (0 if (n, dead) == (5, 0) else 1)
    assert one["route"] == int(has_ties(w))
    assert_same(one, three)
    assert one["ip"] == GOLD[key + "_initial_p"]
    np.testing.assert_array_equal(three["src"], GOLD[key + "_source"])
    np.testing.assert_array_equal(three["dup"], GOLD[key + "_dup"])
    rows, want = GOLD[key + "_noise"], GOLD[key + "_states"]
    src, dup = GOLD[key + "_source"], GOLD[key + "_dup"]
    assert one["nd"] == len(rows)
    np.testing.assert_array_equal(one["w"], F(1.0) / F(n))
    np.testing.assert_array_equal(one["s"][dup == 0], want[dup == 0])
    _, st1 = capi.rng_uniform(st0, 0.0, float(one["pstep"]))
    assert one["state"] == rng_ref.stream("host", "fresh", st1, 6 * one["nd"])[1]
    g1b.init_drawn(IDENTITY7, rc.SIGMA6, one["nd"], st1)
    dev = g1b.download_state()[0]
    equal = np.all(dev == rows, axis=1)
    zs = np.concatenate([rows[:, 0:3], rows[:, 10:13]], axis=1)
    bound = rng_ref.plus_bounds(s[src[dup == 1]], want[dup == 1], rng_ref.row_bounds(rows, zs, ZERO6), True)
    rng_ref.assert_rows_close(one["s"][dup == 1], want[dup == 1], bound, equal)


# ---- resizeParticle in one call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1000, 4097])
@pytest.mark.parametrize("dead", [False, True])
def test_resize_resident_equals_the_three_calls(g1, g1b, n, dead):
    s = states(n, seed=n)
    w = tie_free(n)
    if dead:
        w[np.random.default_rng(n + 1).integers(0, n, n // 4)] = 0
        w = (w / w.sum(dtype=np.float64)).astype(F)
    for n_out in rc.resize_targets(n):
        for g in (g1, g1b):
            g.upload_state(s, w)
            g.draw_odom_noise(ODOM_ERR4, 99)
        route = g1.resize_resident(n_out)
        assert route == int(has_ties(w)) == int(dead)
        g1b.resample_begin(n_out)
        src, dup, nd = g1b.resample_plan(1)
        assert nd == 0
        g1b.resample_apply()
        assert g1.resident() == g1b.resident() == n_out
        got, got_w = g1.download_state()
        want, want_w = g1b.download_state()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, s[src])
        np.testing.assert_array_equal(got_w, want_w)
        np.testing.assert_array_equal(got_w, F(1.0) / F(n_out))
        np.testing.assert_array_equal(g1.download_odom_noise(), g1b.download_odom_noise())
        if pyoracle.available("ref"):
            ref, ref_w = pyoracle.Oracle("ref").resize(s, w, n_out)
            np.testing.assert_array_equal(got, ref)
            np.testing.assert_array_equal(got_w, ref_w)


# ---- one context, weights in device memory ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_out,mode", [(600, 600, 0), (4097, 4097, 0), (1000, 2005, 1), (1000, 334, 1)])
def test_plan_device_leaves_the_context_where_plan_does(eng, n, n_out, mode):
    import torch
    s, w = states(n), tie_free(n)
    d_w = torch.from_numpy(w).cuda()
    d_in = torch.from_numpy(s).cuda()
    torch.cuda.synchronize()
    st0 = capi.rng_seed(7)
    other = capi.Engine(0)
    try:
        pstep_b = other.resample_begin_device(d_w, n, n_out)
        ip_b, st_b = capi.rng_uniform(st0, 0.0, pstep_b) if mode == 0 else (0.0, None)
        nd_b = other.resample_plan(mode, ip_b, want_plan=False)
        nd_b = nd_b[-1] if isinstance(nd_b, tuple) else nd_b
        pstep, ip, nd, st, route = eng.resample_plan_device(d_w, n, n_out, mode, st0 if mode == 0 else None)
        assert (F(pstep), F(ip), nd, st, route) == (F(pstep_b), F(ip_b), nd_b, st_b, 0)
        noise = states(max(nd, 1), seed=9)[:nd]
        outs = []
        for e in (eng, other):
            d_out = torch.zeros((n_out, 13), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()   # (the fill runs on torch's stream, the engine's kernels on its own)
            e.resample_apply_device(d_in, noise, d_out)
            outs.append(d_out.cpu().numpy())
        np.testing.assert_array_equal(outs[0], outs[1])
    finally:
        other.close()


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_plan_device_takes_weights_at_any_float_alignment(eng, shift):
    """d_weight 4, 8 and 12 bytes off a 16-byte boundary: the chain takes scalar loads there, the plan is the aligned one's."""
    import torch
    n = 1500
    s, w = states(n), tie_free(n)
    buf = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    buf[shift:shift + n] = torch.from_numpy(w).cuda()
    d_w, d_aligned = buf[shift:shift + n], torch.from_numpy(w).cuda()
    d_in = torch.from_numpy(s).cuda()
    torch.cuda.synchronize()
    assert d_w.data_ptr() % 16 == 4 * shift and d_aligned.data_ptr() % 16 == 0
    st0 = capi.rng_seed(11)
    want = eng.resample_plan_device(d_aligned, n, n, 0, st0)
    outs = []
    for d in (d_aligned, d_w):
        got = eng.resample_plan_device(d, n, n, 0, st0)
        assert got == want and got[4] == 0
        noise = states(max(got[2], 1), seed=9)[:got[2]]
        d_out = torch.zeros((n, 13), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.resample_apply_device(d_in, noise, d_out)
        outs.append(d_out.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])


# ---- groups ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dead", [0, 300])
def test_shards_match_a_group_of_one(g1, g3, dead):
    n = 1000
    s, w = (states(n), tie_free(n)) if dead == 0 else rc.make_case(n, dead)
    st0 = capi.rng_seed(31337)
    out = []
    for g in (g1, g3):
        g.upload_state(s, w)
        st = g.draw_odom_noise(ODOM_ERR4, st0)
        out.append(one_call(g, rc.SIGMA6, st))
    assert out[0]["route"] == out[1]["route"] == (1 if dead else 0)
    assert_same(out[1], out[0])
    for n_out in rc.resize_targets(n):
        res = []
        for g in (g1, g3):
            g.upload_state(s, w)
            res.append((g.resize_resident(n_out),) + g.download_state())
        assert res[0][0] == res[1][0]
        np.testing.assert_array_equal(res[0][1], res[1][1])
        np.testing.assert_array_equal(res[0][2], res[1][2])


def odom_noise(n):
    return np.random.default_rng(n + 17).normal(0, 0.1, (n, 4)).astype(F)


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("n,n_out", [(1, 3), (65, 64), (1000, 1500)])
def test_one_rank_over_rccl_equals_the_three_calls(g1r, g1b, n, n_out, with_noise):
    """The gather of the weights, the states and the odometry noise with one rank over RCCL (padded ncclAllGather + unpad): the
    one-call forms on the sharded group against the three-call sequences on a direct group of one."""
    s, w = states(n, seed=n + 1), tie_free(n)
    st0 = capi.rng_seed(n + 3)

    def start():
        for g in (g1r, g1b):
            g.upload_state(s, w)
            if with_noise:
                g.set_odom_noise(odom_noise(n))

    start()
    before = g1r.collective_stats()
    one, three = one_call(g1r, rc.SIGMA6, st0), three_call(g1b, rc.SIGMA6, st0)
    # the weights' all-gather, and the states' (the noise rides in the states' round)
    assert g1r.collective_stats() == dict(rccl=before["rccl"] + 2, host=before["host"])
    assert one["route"] == int(has_ties(w))
    assert_same(one, three)
    assert one["odom"].any() == (with_noise and bool(np.any(three["dup"] == 0)))
    start()
    route = g1r.resize_resident(n_out)
    g1b.resample_begin(n_out)
    src, dup, nd = g1b.resample_plan(1)
    g1b.resample_apply()
    assert route == int(has_ties(w)) and nd == 0
    assert g1r.resident() == g1b.resident() == n_out
    got, want = g1r.download_state(), g1b.download_state()
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[0], s[src])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(g1r.download_odom_noise(), g1b.download_odom_noise())
    if with_noise:
        np.testing.assert_array_equal(g1r.download_odom_noise(), odom_noise(n)[src])


def test_more_ranks_than_particles_through_the_host(g1):
    """Five contexts, three particles: two shards are empty (and every shard is, or is one short of, the largest). Each step
    against a group of one given the same calls."""
    s, w = states(3, seed=8), tie_free(3)
    g5 = capi.Group([0] * 5, collective="host")
    try:
        # (g1 is the module's shared direct group: whatever it held, the first step below is an upload_state, which replaces it)
        def both(call):
            out = [call(g) for g in (g5, g1)]
            assert out[0] == out[1]  # what the call returns: resize's route; resample_drawn's engine state, pstep, initial_p, n_dup
            assert g5.resident() == g1.resident()
            for a, b in zip(g5.download_state() + (g5.download_odom_noise(),), g1.download_state() + (g1.download_odom_noise(),)):
                np.testing.assert_array_equal(a, b)

        both(lambda g: g.upload_state(s, w))
        both(lambda g: g.set_odom_noise(odom_noise(3)))
        assert g5.download_odom_noise().any()
        both(lambda g: g.resize_resident(7))
        assert g5.resident() == 7
        both(lambda g: g.resize_resident(2))
        assert g5.resident() == 2
        both(lambda g: g.resample_drawn(rc.SIGMA6, capi.rng_seed(5)))
    finally:
        g5.close()


# ---- further cases ---------------------------------------------------------------------------------------------------------
def test_second_round_on_the_same_group(g1, g1b):
    """resample, new weights, resample again: the context's plan state carries nothing over."""
    n = 1500
    s, w = states(n), tie_free(n)
    st_a = st_b = capi.rng_seed(2024)
    g1.upload_state(s, w)
    g1b.upload_state(s, w)
    for round_ in range(2):
        one, three = one_call(g1, rc.SIGMA6, st_a), three_call(g1b, rc.SIGMA6, st_b)
        assert_same(one, three)
        assert one["route"] == round_   # (round 1's weights have dead particles)
        st_a, st_b = one["state"], three["state"]
        w2 = tie_free(n + 1)[:n].copy()
        w2[::7] = 0
        w2 = (w2 / w2.sum(dtype=np.float64)).astype(F)
        g1.upload_state(one["s"], w2)
        g1b.upload_state(three["s"], w2)
    # and the three-call sequence still works behind the one-call form on the same group
    assert_same(three_call(g1, rc.SIGMA6, st_a), three_call(g1b, rc.SIGMA6, st_b))


def test_mixing_with_host_draws_stays_on_the_stream(g1, g1b):
    n = 1000
    s, w = states(n), tie_free(n)
    st0 = rng_ref.minstd_seed(777)
    g1.upload_state(s, w)
    g1b.upload_state(s, w)
    st_a = g1.draw_odom_noise(ODOM_ERR4, st0)
    st_b = g1b.draw_odom_noise(ODOM_ERR4, st0)
    u_a, st_a = capi.rng_uniform(st_a, 0.0, 1.0)
    u_b, st_b = capi.rng_uniform(st_b, 0.0, 1.0)
    one, three = one_call(g1, rc.SIGMA6, st_a), three_call(g1b, rc.SIGMA6, st_b)
    assert_same(one, three)
    # the one call made exactly one engine call for initial_p and six per duplicated slot's accepted attempts
    v = rng_ref.minstd_next(st_a)
    assert one["ip"] == F(F(F(v - 1) / F(2147483648.0)) * one["pstep"])
    assert one["state"] == rng_ref.stream("std", "fresh", v, 6 * one["nd"])[1]
    assert g1.add_noise_drawn(rc.SIGMA6, one["state"]) == g1b.add_noise_drawn(rc.SIGMA6, three["state"])
    np.testing.assert_array_equal(g1.download_state()[0], g1b.download_state()[0])


def test_errors_name_the_argument(eng):
    g = capi.Group([0])
    try:
        with pytest.raises(capi.EngineError, match="-5.*no resident particles"):
            g.resample_drawn(rc.SIGMA6, 1)
        with pytest.raises(capi.EngineError, match="-5.*no resident particles"):
            g.resize_resident(8)
        g.upload_state(states(8))
        bad_sigma = rc.SIGMA6.copy()
        bad_sigma[2] = -0.1
        nan_sigma = rc.SIGMA6.copy()
        nan_sigma[4] = np.nan
        with pytest.raises(capi.EngineError, match=r"-3.*sigma6\[2\]"):
            g.resample_drawn(bad_sigma, 1)
        with pytest.raises(capi.EngineError, match=r"-3.*sigma6\[4\]"):
            g.resample_drawn(nan_sigma, 1)
        for st in (0, 2 ** 31 - 1, 2 ** 32 - 1):
            with pytest.raises(capi.EngineError, match="-3.*engine_state"):
                g.resample_drawn(rc.SIGMA6, st)
        for n_out in (0, 2 ** 31):
            with pytest.raises(capi.EngineError, match="-3.*n_out"):
                g.resize_resident(n_out)
        lib = capi.load_library()
        st = capi.C.c_uint32(1)
        null = capi.C.POINTER(capi.C.c_uint32)()
        assert lib.mcl3dl_hip_group_resample_drawn(g.h, None, capi.C.byref(st), None, None, None, None) == -3
        assert b"sigma6" in lib.mcl3dl_hip_group_last_error(g.h)
        assert lib.mcl3dl_hip_group_resample_drawn(g.h, capi._ptr(rc.SIGMA6), null, None, None, None, None) == -3
        assert b"engine_state" in lib.mcl3dl_hip_group_last_error(g.h)
        assert lib.mcl3dl_hip_group_resample_drawn(None, capi._ptr(rc.SIGMA6), capi.C.byref(st), None, None, None, None) == -1
        assert lib.mcl3dl_hip_group_resize_resident(None, 8, None) == -1
        # the failed calls left the resident particles and the engine state alone
        assert st.value == 1
        np.testing.assert_array_equal(g.download_state()[0], states(8))
        # every output pointer is optional
        assert lib.mcl3dl_hip_group_resample_drawn(g.h, capi._ptr(rc.SIGMA6), capi.C.byref(st), None, None, None, None) == 0
        assert lib.mcl3dl_hip_group_resize_resident(g.h, 5, None) == 0 and g.resident() == 5
    finally:
        g.close()
    # the context-level calls
    import torch
    d_w = torch.full((8,), 0.125, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(capi.EngineError, match="-3.*d_weight"):
        eng.resample_plan_device(None, 8, 8, 0, 1)
    with pytest.raises(capi.EngineError, match="-3.*d_weight"):
        eng.resample_plan_device(d_w, 0, 8, 0, 1)
    for n_out in (0, 2 ** 31):
        with pytest.raises(capi.EngineError, match="-3.*n_out"):
            eng.resample_plan_device(d_w, 8, n_out, 0, 1)
    with pytest.raises(capi.EngineError, match="-3.*mode"):
        eng.resample_plan_device(d_w, 8, 8, 2, 1)
    for st in (0, 2 ** 31 - 1):
        with pytest.raises(capi.EngineError, match="-3.*engine_state"):
            eng.resample_plan_device(d_w, 8, 8, 0, st)
    with pytest.raises(capi.EngineError, match="-3.*engine_state"):
        eng.resample_plan_device(d_w, 8, 8, 0, None)
    assert eng.resample_plan_device(d_w, 8, 8, 1, None)[3] is None   # mode 1 needs no engine state
    lib = capi.load_library()
    assert lib.mcl3dl_hip_float_prefix(eng.h, None, 1.0, 4, None) == -3
    assert b"out_prefix" in lib.mcl3dl_hip_last_error(eng.h)
    assert lib.mcl3dl_hip_float_prefix(eng.h, None, 1.0, 2 ** 31, capi._ptr(np.zeros(1, F))) == -3
    assert b"n = " in lib.mcl3dl_hip_last_error(eng.h)
    assert lib.mcl3dl_hip_float_prefix(eng.h, None, 1.0, 0, None) == 0
    assert lib.mcl3dl_hip_float_prefix(None, None, 1.0, 0, None) == -1
    assert lib.mcl3dl_hip_resample_plan_device(None, None, 0, 0, 0, None, None, None, None, None) == -1


def test_likelihood_update_is_left_alone():
    """The same states weigh the same after the one-call forms ran on the group."""
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
        st = g.resample_drawn(rc.SIGMA6, 4242)[3]
        g.resize_resident(450)
        g.resize_resident(300)
        g.resample_drawn(rc.SIGMA6, st)
        g.upload_state(s, sc.weights)
        after = g.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        for key in ("weights", "lik", "beam", "quality"):
            np.testing.assert_array_equal(before[key], after[key], err_msg=key)
        assert before["entropy"] == after["entropy"]
    finally:
        g.close()


# ---- speed ------------------------------------------------------------------------------------------------------------------
def timed(g, s, w, call, reps=5):
    ts = []
    for _ in range(reps):
        g.upload_state(s, w)
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def test_one_call_is_not_slower_than_three(g1):
    """One group, tie-free weights, best of five each. Not slower is the whole condition at 4096 particles: the three-call route
    downloads the weights, runs the recurrence on a host core, uploads the prefixes and synchronises twice more. At 262 144 both
    are printed and recorded (profiles/resample_resident.txt) without a gate: one wavefront against one host core."""
    lib = g1.lib
    st = capi.C.c_uint32(0)
    sig = capi._ptr(rc.SIGMA6)

    def one():
        st.value = 12345
        assert lib.mcl3dl_hip_group_resample_drawn(g1.h, sig, capi.C.byref(st), None, None, None, None) == 0

    def three():
        st.value = 12345
        pstep = capi.C.c_float(0)
        nd = capi.C.c_size_t(0)
        assert lib.mcl3dl_hip_group_resample_begin(g1.h, 0, capi.C.byref(pstep)) == 0
        ip = lib.mcl3dl_hip_rng_uniform(capi.C.byref(st), 0.0, pstep.value)
        assert lib.mcl3dl_hip_group_resample_plan(g1.h, 0, ip, None, None, capi.C.byref(nd)) == 0
        assert lib.mcl3dl_hip_group_resample_apply_drawn(g1.h, sig, capi.C.byref(st)) == 0

    for n in (4096, 262144):
        s, w = states(n), tie_free(n)
        timed(g1, s, w, one, 1)
        timed(g1, s, w, three, 1)
        t_three, t_one = timed(g1, s, w, three), timed(g1, s, w, one)
        print("resample at %d particles: one call %.3f ms, three calls %.3f ms" % (n, t_one * 1e3, t_three * 1e3))
        if n == 4096:
            assert t_one <= t_three, (t_one, t_three)
