"""GPU tests of the beam model's second raycaster: mcl3dl_hip_set_beam_raycast(ctx, 1) = RaycastUsingKDTree, the reference's
default (beam/use_raycast_using_dda = false; include/mcl_3dl/raycasts/raycast_using_kdtree.h:58-109), against the oracle.

Statuses, hit indices and penalty counts are integers and the beam score is pow_table[count], clamped: every comparison with
the oracle is exact (np.testing.assert_array_equal), nothing here has a tolerance. The oracle is built with
max_search_radius = 0.4 >= the caster's second radius (0.271 m on 0.1 m grids), so the reference's chunking hides no point."""
import time

import numpy as np
import pytest
import torch

import beam_kdtree_cases as cases
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu

DW5 = (1.0, 1.0, 5.0)
N_ROUTE, NB_ROUTE, NS_ROUTE = 1100, 32, 1024   # above update_small / pf_fused / beam_prepare (32 768 rays) / 64 beam work-groups
N_SMALL, NB_SMALL = 300, 8                     # below all of them


@pytest.fixture(scope="module")
def eng():
    """A context of this module's own: the caster's mode never leaks into the session's shared engine."""
    e = capi.Engine(0)
    yield e
    e.close()


def configure(obj, sc, dist_weight, stamp, mode, **beam_kw):
    obj.set_map(sc.map_xyz, sc.map_label, stamp=stamp, dist_weight=dist_weight)
    obj.set_likelihood_params()
    obj.set_beam_params(**beam_kw)
    obj.set_beam_raycast(mode)


def oracle_beam(kind, sc, dist_weight, poses, n_b, use_dda=False, threads=16, **beam_kw):
    o = cases.make_oracle(kind, sc.map_xyz, sc.map_label, dist_weight, use_dda=use_dda, **beam_kw)
    return o.beam_measure(poses, sc.scan_beam[:n_b], sc.scan_beam_label[:n_b], sc.origins, threads=threads)[0]


# ---- 1. statuses ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(cases.STATUS_CASES, key=str), ids=str)
def test_statuses_and_hit_indices_equal_the_oracle(eng, oracle_kind, case):
    dist_weight, flm = case
    sc = cases.scene()
    begin, end = cases.rays()
    want_st, want_hit = cases.oracle_statuses(oracle_kind, dist_weight, flm, False)
    dda_st, dda_hit = cases.oracle_statuses(oracle_kind, dist_weight, flm, True)
    # what keeps this from passing vacuously: the oracle's answer holds all four statuses, in the recorded numbers, and the
    # two casters disagree on at least 400 rays
    counts = tuple(int(np.sum(want_st == s)) for s in range(4))
    assert counts == cases.STATUS_CASES[case] and min(counts) > 0
    assert int(np.sum(want_st != dda_st)) >= 400
    configure(eng, sc, dist_weight, 9100, 1, filter_label_max=flm)
    try:
        assert eng.get_beam_raycast() == 1
        st, hit = eng.beam_status(begin, end)
        print("kd-tree caster, %s: engine counts %s, oracle %s" % (case, [int(np.sum(st == s)) for s in range(4)], counts))
        np.testing.assert_array_equal(st, want_st)
        np.testing.assert_array_equal(hit, want_hit)
        # ... and mode 0 still casts with the DDA
        eng.set_beam_raycast(0)
        st0, hit0 = eng.beam_status(begin, end)
        np.testing.assert_array_equal(st0, dda_st)
        np.testing.assert_array_equal(hit0, dda_hit)
    finally:
        eng.set_beam_raycast(0)


# ---- 2. scores --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist_weight", [None, DW5], ids=str)
@pytest.mark.parametrize("short_only", [True, False])
def test_beam_scores_equal_the_oracle(eng, oracle_kind, dist_weight, short_only):
    sc = cases.scene()
    kw = dict(num_points=48, add_penalty_short_only_mode=short_only, filter_label_max=1)
    want = oracle_beam(oracle_kind, sc, dist_weight, sc.poses, 48, threads=4, **kw)
    assert len(np.unique(want)) > 3   # (the scores differ between the particles: equality says something)
    configure(eng, sc, dist_weight, 9200, 1, **kw)
    try:
        _, _, beam = eng.measure_batch(sc.poses, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        np.testing.assert_array_equal(beam, want)
        # the beam model alone (the node asks each model separately), and delivered in slices
        _, _, alone = eng.measure_batch(sc.poses, None, sc.scan_beam, sc.scan_beam_label, sc.origins)
        np.testing.assert_array_equal(alone, want)
        _, _, sliced = eng.measure_batch_begin(sc.poses, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins, slice_particles=8)
        assert eng.measure_batch_wait(len(sc.poses) - 1) == len(sc.poses)
        eng.measure_batch_end()
        np.testing.assert_array_equal(sliced, want)
        # one particle, one ray; no rays at all (beam.cpp:130-133: score 1)
        one = oracle_beam(oracle_kind, sc, dist_weight, sc.poses[:1], 1, threads=1, **kw)
        _, _, got1 = eng.measure_batch(sc.poses[:1], None, sc.scan_beam[:1], sc.scan_beam_label[:1], sc.origins)
        np.testing.assert_array_equal(got1, one)
        _, _, none = eng.measure_batch(sc.poses, sc.scan_lik, None, None, sc.origins)
        np.testing.assert_array_equal(none, np.ones(len(sc.poses), np.float32))
    finally:
        eng.set_beam_raycast(0)


# ---- 3. routes --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def route_scene():
    return make_scene(n=61, n_p=N_ROUTE, n_s=NS_ROUTE, n_b=NB_ROUTE, label_wall=2, seed=2024)


@pytest.fixture(scope="module")
def route_want(oracle_kind, route_scene):
    """The oracle's kd-tree beam scores of both shapes, computed once (read-only)."""
    sc = route_scene
    big = oracle_beam(oracle_kind, sc, DW5, sc.poses, NB_ROUTE, num_points=NB_ROUTE)
    small = oracle_beam(oracle_kind, sc, DW5, sc.poses[:N_SMALL], NB_SMALL, num_points=NB_SMALL)
    for a in (big, small):
        assert len(np.unique(a)) > 3
        a.setflags(write=False)
    return {N_ROUTE: big, N_SMALL: small}


def route_args(sc, n_p, n_b):
    return sc.poses[:n_p], sc.scan_lik, sc.scan_beam[:n_b], sc.scan_beam_label[:n_b], sc.origins


@pytest.mark.parametrize("n_p,n_b", [(N_ROUTE, NB_ROUTE), (N_SMALL, NB_SMALL)])
def test_every_route_of_an_update_casts_with_the_selected_caster(eng, route_scene, route_want, n_p, n_b):
    sc = route_scene
    want = route_want[n_p]
    poses, scan_lik, scan_beam, lab, origins = route_args(sc, n_p, n_b)
    w0 = np.random.default_rng(n_p).uniform(0.1, 1.0, n_p).astype(np.float32)
    configure(eng, sc, DW5, 9300, 0, num_points=n_b)
    dev = torch.device("cuda", 0)
    try:
        res = {}
        for mode in (0, 1):
            eng.set_beam_raycast(mode)
            host = eng.measure_update(poses, w0, scan_lik, scan_beam, lab, origins)
            eng.upload_scan(scan_lik, scan_beam, lab, origins)
            d_pose = torch.from_numpy(np.ascontiguousarray(poses)).to(dev)
            d_w = torch.from_numpy(w0.copy()).to(dev)
            d_lik, d_ratio, d_beam = (torch.empty(n_p, device=dev) for _ in range(3))
            d_stats = torch.zeros(4, device=dev)
            torch.cuda.synchronize()   # the engine runs on its own stream
            eng.update_device(d_pose, n_p, d_w, d_stats, d_lik=d_lik, d_ratio=d_ratio, d_beam=d_beam)
            eng.synchronize()
            device = dict(weights=d_w.cpu().numpy(), lik=d_lik.cpu().numpy(), quality=d_ratio.cpu().numpy(), beam=d_beam.cpu().numpy())
            m_lik, m_ratio, m_beam = (torch.empty(n_p, device=dev) for _ in range(3))
            eng.measure_device(d_pose, n_p, m_lik, m_ratio, m_beam)
            eng.synchronize()
            device["measure_beam"] = m_beam.cpu().numpy()
            res[mode] = (host, device)
        for name, got in (("measure_update", res[1][0]), ("update_device", res[1][1])):
            np.testing.assert_array_equal(got["beam"], want, err_msg=name)
            # pf::measure behind the caster is untouched: the engine's own pf_measure on these scores gives these weights
            apart = eng.pf_measure(w0, got["lik"], got["beam"], None, got["quality"])
            np.testing.assert_array_equal(got["weights"], apart["weights"], err_msg=name)
            # ... and the likelihood model kept its route's bits
            ref0 = res[0][0] if name == "measure_update" else res[0][1]
            np.testing.assert_array_equal(got["lik"], ref0["lik"], err_msg=name)
            np.testing.assert_array_equal(got["quality"], ref0["quality"], err_msg=name)
        np.testing.assert_array_equal(res[1][1]["measure_beam"], want)
        assert np.any(res[0][0]["beam"] != want)   # (mode 0 is the other caster on this scene)
    finally:
        eng.set_beam_raycast(0)


def test_beside_the_likelihood_kernel_on_the_second_stream(eng, oracle_kind):
    """From overlap_min_rays = 262 144 rays the beam kernels run on the second stream beside the likelihood kernel: 1100
    particles x 256 rays = 281 600."""
    sc = make_scene(n=61, n_p=N_ROUTE, n_s=NS_ROUTE, n_b=256, label_wall=2, seed=2025)
    want = oracle_beam(oracle_kind, sc, DW5, sc.poses, 256, num_points=256)
    assert len(np.unique(want)) > 3
    w0 = np.random.default_rng(3).uniform(0.1, 1.0, N_ROUTE).astype(np.float32)
    configure(eng, sc, DW5, 9350, 0, num_points=256)
    try:
        res = {}
        for mode in (0, 1):
            eng.set_beam_raycast(mode)
            res[mode] = eng.measure_update(sc.poses, w0, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        np.testing.assert_array_equal(res[1]["beam"], want)
        np.testing.assert_array_equal(res[1]["lik"], res[0]["lik"])
        np.testing.assert_array_equal(res[1]["quality"], res[0]["quality"])
        apart = eng.pf_measure(w0, res[1]["lik"], res[1]["beam"], None, res[1]["quality"])
        np.testing.assert_array_equal(res[1]["weights"], apart["weights"])
    finally:
        eng.set_beam_raycast(0)


# ---- 4. switching -----------------------------------------------------------------------------------------------------
def test_the_caster_can_be_switched_between_calls(eng, oracle_kind):
    sc = cases.scene()
    kw = dict(num_points=48)
    want = {m: oracle_beam(oracle_kind, sc, DW5, sc.poses, 48, use_dda=(m == 0), threads=4, **kw) for m in (0, 1)}
    assert np.any(want[0] != want[1])
    configure(eng, sc, DW5, 9400, 0, **kw)
    try:
        assert eng.get_beam_raycast() == 0
        for mode in (0, 1, 0, 1):
            eng.set_beam_raycast(mode)
            assert eng.get_beam_raycast() == mode
            _, _, beam = eng.measure_batch(sc.poses, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
            np.testing.assert_array_equal(beam, want[mode], err_msg="mode %d" % mode)
        for bad in (2, -1):
            assert eng.lib.mcl3dl_hip_set_beam_raycast(eng.h, bad) == -3
            assert eng.get_beam_raycast() == 1
        with pytest.raises(capi.EngineError):
            eng.set_beam_raycast(2)
        # parameters set while the kd-tree caster is selected reach it (hit_range is its hit_tolerance_)
        kw2 = dict(num_points=48, hit_range=0.45, map_grid=(0.1, 0.15, 0.1), add_penalty_short_only_mode=False)
        okw2 = dict(num_points=48, hit_range=0.45, map_grid_y=0.15, add_penalty_short_only_mode=False)
        eng.set_beam_params(**kw2)
        _, _, beam = eng.measure_batch(sc.poses, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        np.testing.assert_array_equal(beam, oracle_beam(oracle_kind, sc, DW5, sc.poses, 48, threads=4, **okw2))
    finally:
        eng.set_beam_raycast(0)


# ---- 5. a context that only ever runs the beam model ------------------------------------------------------------------
@pytest.mark.parametrize("dist_weight", [None, DW5], ids=str)
def test_beam_only_context(oracle_kind, dist_weight):
    sc = cases.scene()
    want = oracle_beam(oracle_kind, sc, dist_weight, sc.poses, 48, threads=4, num_points=48)
    e = capi.Engine(0)
    try:
        e.set_map(sc.map_xyz, sc.map_label, stamp=9500, dist_weight=dist_weight)
        e.set_beam_raycast(1)              # before the parameters, before the first ray
        e.set_beam_params(num_points=48)
        _, _, beam = e.measure_batch(sc.poses, None, sc.scan_beam, sc.scan_beam_label, sc.origins)
        np.testing.assert_array_equal(beam, want)
        fp = e.memory_footprint()
        assert fp["dda_bits"] == 0 and fp["dda_voxels"] == 0, "a context on the kd-tree caster built the DDA grid"
        assert fp["lik_cells"] > 0
        # the likelihood model arriving later (its parameters set for the first time) finds a cell grid it can use
        e.set_likelihood_params()
        e.set_option("lik_index", 0)
        lik, ratio, beam2 = e.measure_batch(sc.poses, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        o = cases.make_oracle(oracle_kind, sc.map_xyz, sc.map_label, dist_weight, num_points=48)
        want_lik, want_q = o.likelihood_measure(sc.poses, sc.scan_lik)
        np.testing.assert_array_equal(beam2, want)
        np.testing.assert_array_equal(ratio, want_q)
        np.testing.assert_allclose(lik, want_lik, rtol=1e-5)   # (tests/test_gpu_parity.py: the likelihood score's bound)
    finally:
        e.close()


# ---- 6. map update ----------------------------------------------------------------------------------------------------
def test_a_map_update_is_seen_through_the_merged_cell_grid(eng, oracle_kind):
    sc = cases.scene()
    kw = dict(num_points=48, add_penalty_short_only_mode=False)
    configure(eng, sc, DW5, 9600, 1, **kw)
    try:
        before = oracle_beam(oracle_kind, sc, DW5, sc.poses, 48, threads=4, **kw)
        _, _, got = eng.measure_batch(sc.poses, None, sc.scan_beam, sc.scan_beam_label, sc.origins)
        np.testing.assert_array_equal(got, before)
        # a wall 0.8 m in front of the sensor, across the rays (one point per 0.1 m leaf: VoxelGrid keeps each as it is)
        centre = sc.poses[:, :3].astype(np.float64).mean(0)
        yy, zz = np.meshgrid(np.arange(-15, 16) * 0.1, np.arange(-12, 13) * 0.1, indexing="ij")
        wall = np.stack([np.full(yy.size, centre[0] + 0.8), centre[1] + yy.ravel(), centre[2] + zz.ravel()], 1)
        wall = (np.floor(wall / 0.1) * 0.1 + 0.05).astype(np.float32)
        wall = np.unique(wall, axis=0)
        n_map, _ = eng.map_update(wall, None, leaf=(0.1, 0.1, 0.1), stamp=9601)
        merged_xyz, merged_lab = eng.map_download()
        assert n_map == len(merged_xyz) == len(sc.map_xyz) + len(wall)
        np.testing.assert_array_equal(merged_xyz[:len(sc.map_xyz)], sc.map_xyz)
        o = cases.make_oracle(oracle_kind, merged_xyz, merged_lab, DW5, **kw)
        want = o.beam_measure(sc.poses, sc.scan_beam, sc.scan_beam_label, sc.origins, threads=4)[0]
        assert np.any(want != before)   # (the wall changes the scores)
        _, _, got = eng.measure_batch(sc.poses, None, sc.scan_beam, sc.scan_beam_label, sc.origins)
        np.testing.assert_array_equal(got, want)
        begin, end = cases.rays()
        st, hit = eng.beam_status(begin[:500], end[:500])
        want_st, want_hit = o.beam_status(begin[:500], end[:500])
        np.testing.assert_array_equal(st, want_st)
        np.testing.assert_array_equal(hit, want_hit)
        assert np.any(want_hit >= len(sc.map_xyz))   # (some rays end on the update's points)
    finally:
        eng.set_beam_raycast(0)


# ---- 7. device groups -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices,collective,direct", [((0,), None, 1), ((0,), "host", 0), ((0, 0, 0), "host", 1)],
                         ids=["one-direct", "one-sharded-host", "three-host"])
def test_groups_cast_with_the_selected_caster(eng, route_scene, route_want, devices, collective, direct):
    """The group forms against ONE context on the same inputs, bit for bit: likelihoods, match ratios, beam scores — and, where
    one device holds every particle, weights and entropy. Three shards add their weights in one fp64 all-reduce where one
    context adds 1100 of them in an fp64 tree: 1100 floats within a few binades of each other add up exactly in fp64 either
    way, so the normalised weights are the same bits there too."""
    sc = route_scene
    n_p, n_b = N_ROUTE, NB_ROUTE
    poses, scan_lik, scan_beam, lab, origins = route_args(sc, n_p, n_b)
    rng = np.random.default_rng(77)
    w0 = rng.uniform(0.5, 1.5, n_p).astype(np.float32)
    st = np.zeros((n_p, 13), np.float32)
    st[:, :7] = poses
    configure(eng, sc, DW5, 9700, 1, num_points=n_b)
    g = capi.Group(devices, collective=collective)
    try:
        want = eng.measure_update(poses, w0, scan_lik, scan_beam, lab, origins)
        np.testing.assert_array_equal(want["beam"], route_want[n_p])
        configure(g, sc, DW5, 9700, 1, num_points=n_b)
        assert g.get_beam_raycast() == 1
        g.set_option("direct_single", direct)
        got_u = g.measure_update(poses, w0, scan_lik, scan_beam, lab, origins)
        g.upload_state(st, w0)
        got_r = g.update_resident(scan_lik, scan_beam, lab, origins)
        for name, got in (("group_measure_update", got_u), ("group_update_resident", got_r)):
            for k in ("lik", "quality", "beam", "weights"):
                np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (name, k))
            if len(devices) == 1:
                assert got["entropy"] == want["entropy"], name
            else:
                np.testing.assert_allclose(got["entropy"], want["entropy"], rtol=1e-6)   # (tests/test_gpu_group_state.py: the sum of w ln w is not exact)
        assert g.lib.mcl3dl_hip_group_set_beam_raycast(g.h, 2) == -3 and g.get_beam_raycast() == 1
    finally:
        g.close()
        eng.set_beam_raycast(0)


# ---- 8. rays that must not spin ---------------------------------------------------------------------------------------
def test_degenerate_and_very_long_rays(eng, oracle_kind):
    sc = cases.scene()
    half = 61 * 0.1 / 2.0
    begin = np.array([[0.3, 0.2, 0.1],                 # zero length
                      [half + 0.5, 0.1, 0.2],          # starts behind the map, 10 km away from it
                      [half + 0.5, -0.4, 0.3],         # ... along a diagonal
                      [0.0, 0.0, 0.0],                 # from inside through the wall to 10 km
                      [0.1, 0.1, 0.1]], np.float32)    # NaN end point
    end = np.array([[0.3, 0.2, 0.1],
                    [half + 10000.0, 0.1, 0.2],
                    [half + 7000.0, 7000.0, 1500.0],
                    [10000.0, 0.0, 0.0],
                    [np.nan, 0.0, 0.0]], np.float32)
    o = cases.make_oracle(oracle_kind, sc.map_xyz, sc.map_label, DW5)
    # The zero-length ray marches from a NaN position (0 / 0 in the normalisation): three searches that find nothing, LONG. The
    # reference-backed oracle computes that; the plain-C port's chunk lookup converts the NaN to an index (undefined, it
    # crashes), so where only the port is built the reference's recorded answer stands in for that one ray.
    first = 0 if oracle_kind == "ref" else 1
    want_st, want_hit = o.beam_status(begin[first:4], end[first:4])
    if first:
        want_st, want_hit = np.concatenate([[2], want_st]), np.concatenate([[-1], want_hit])
    assert want_st[0] == 2 and want_st[1] == 2 and want_st[2] == 2 and want_st[3] != 2
    configure(eng, sc, DW5, 9800, 1)
    try:
        eng.beam_status(begin[:1], end[:1])   # (structures built outside the timed call)
        t0 = time.perf_counter()
        st, hit = eng.beam_status(begin, end)
        dt = time.perf_counter() - t0
        print("five degenerate / 10 km rays: %.4f s" % dt)
        np.testing.assert_array_equal(st[:4], want_st)
        np.testing.assert_array_equal(hit[:4], want_hit)
        assert st[4] == 2 and hit[4] == -1   # a non-finite end point: LONG, at once
        assert dt < 0.5, "the early exit behind the map is not taken: %.3f s" % dt
    finally:
        eng.set_beam_raycast(0)
