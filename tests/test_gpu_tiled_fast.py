"""The tiled likelihood kernel's pose loop specialised for the common map (likelihood_kernels.h: eval_coop_first<true>, chosen once
per launch from RecGrid::common_map) against the general loop (switch lik_tiled_fast = 0) and against the oracle.

Every case forces the tiled kernel (lik_tiled_min = 1) and runs the same call with both loops in two summation modes that go
through it at these particle counts:
  * strict_order 0   likelihood_tiled_kernel<G, 2, 8, true, true, false> — the benchmark's instantiation — and the fp64 tree:
                     likelihoods, match ratios and the weights of the update equal between the loops bit for bit; against
                     the oracle the tolerances tests/test_gpu_fuzz.py uses for this mode (the fp64 tree is not the reference's sum)
  * strict_order 3   the same pose loop in the CHAIN instantiation, the reference's float recurrence inside the kernel:
                     equal between the loops AND equal to the oracle on the scan in the engine's order, bit for bit
and once in the default mode (strict_order 2), whose result must be the oracle's bit for bit as in the fuzz (below 2048
particles the default adds a short scan up in the per-particle kernels, so that run alone would not reach the tiled kernel).
Which loop ran is read back (lik_tiled_fast_active)."""
import numpy as np
import pytest

from mcl_3dl_amd.synthetic import make_scene
from oracle import pyoracle

pytestmark = pytest.mark.gpu

OPTIONS = dict(lik_tiled_min=1, cand_packed=1, cand_record_parts=0, lik_defer=1)
DEFAULTS = dict(lik_tiled_min=1024, cand_packed=1, cand_record_parts=0, lik_defer=1, strict_order=2, lik_tiled_fast=-1)


def run_case(engine, oracle_kind, sc, stamp, dist_weight=(1.0, 1.0, 1.0), lik_kw=None, options=None, want_fast=1,
             oracle_scan=None):
    """Both loops in both tiled modes; returns the fast results of strict_order 0. oracle_scan: what the oracle is given
    instead of the scan (a scan with a NaN: the same scan with that point moved far outside the map — no match either way)."""
    lik_kw = lik_kw or {}
    poses, scan = sc.poses, sc.scan_lik
    o = pyoracle.Oracle(oracle_kind)
    o.set_map(sc.map_xyz, sc.map_label, dist_weight=dist_weight)
    o.set_likelihood_params(pyoracle.LikelihoodParams(**lik_kw))
    o_scan = scan if oracle_scan is None else oracle_scan
    want_lik, want_q = o.likelihood_measure(poses, o_scan)
    w0 = np.random.default_rng(stamp).uniform(0.1, 1.0, len(poses)).astype(np.float32)
    w0 /= w0.sum()
    out = {}
    try:
        for k, v in dict(OPTIONS, **(options or {})).items():
            engine.set_option(k, v)
        engine.set_map(sc.map_xyz, sc.map_label, stamp=stamp, dist_weight=dist_weight)
        engine.set_likelihood_params(**lik_kw)
        for strict in (0, 3):
            engine.set_option("strict_order", strict)
            for fast in (-1, 0):
                engine.set_option("lik_tiled_fast", fast)
                lik, ratio, _ = engine.measure_batch(poses, scan)
                active = int(engine.get_option("lik_tiled_fast_active"))
                assert active == (want_fast if fast else 0), (strict, fast, active)
                upd = engine.measure_update(poses, w0, scan) if strict == 0 else None
                out[strict, fast] = (lik.copy(), ratio.copy(), None if upd is None else upd["weights"].copy())
            for a, b in zip(out[strict, -1], out[strict, 0]):
                if a is not None:
                    np.testing.assert_array_equal(a, b)
        if want_fast:
            assert int(engine.get_option("lik_defer_active")) == 1 and int(engine.get_option("cand_packed_active")) == 1
        # the fp64 tree against the reference's float sum: the fuzz's tolerances for strict_order 0
        np.testing.assert_allclose(out[0, -1][0], want_lik, rtol=1e-5 if len(scan) <= 512 else 3e-5, atol=0)
        np.testing.assert_array_equal(out[0, -1][1], want_q)
        # the in-kernel recurrence: the oracle on the scan in the engine's order, bit for bit
        order = engine.scan_order(len(scan))
        want3, want_q3 = o.likelihood_measure(poses, np.ascontiguousarray(o_scan[order]))
        np.testing.assert_array_equal(out[3, -1][0], want3)
        np.testing.assert_array_equal(out[3, -1][1], want_q3)
        # the default mode, as the fuzz compares it
        engine.set_option("strict_order", 2)
        engine.set_option("lik_tiled_fast", -1)
        lik, ratio, _ = engine.measure_batch(poses, scan)
        np.testing.assert_array_equal(lik, want_lik)
        np.testing.assert_array_equal(ratio, want_q)
        assert np.count_nonzero(want_q) > 0   # (a case in which nothing matches would compare zeros)
    finally:
        for k, v in DEFAULTS.items():
            engine.set_option(k, v)
        engine.set_likelihood_params()
    return out[0, -1]


@pytest.mark.parametrize("n_s,n_p", [(300, 21), (1030, 40)])
def test_partial_tile_and_partial_group(engine, oracle_kind, n_s, n_p):
    """300 x 21: two tiles, the second with 44 points, and a last particle group of five (n_valid < G = 16);
    1030 x 40: five tiles, the last with six points."""
    sc = make_scene(n=61, n_p=n_p, n_s=n_s, n_b=0, seed=70 + n_p)
    run_case(engine, oracle_kind, sc, stamp=9400 + n_p)


def test_map_of_centroids_runs_overflow_records_the_skip_bound_and_the_queue(engine, oracle_kind):
    sc = make_scene(n=58, n_p=48, n_s=600, n_b=0, seed=72, map_jitter=0.045)   # 6 x 58^2 = 20 184 map points
    run_case(engine, oracle_kind, sc, stamp=9410)
    engine.set_option("lik_tiled_min", 1)
    try:
        engine.set_map(sc.map_xyz, sc.map_label, stamp=9410, dist_weight=(1.0, 1.0, 1.0))
        engine.measure_batch(sc.poses, sc.scan_lik)
        st = engine.index_stats()
        assert st["voxels_with_overflow"] > 0.05 * st["voxels_with_candidates"] and st["deferred_overflow"] == 1
        assert int(engine.get_option("cand_bound_active")) == 1
    finally:
        engine.set_option("lik_tiled_min", 1024)


def test_dist_weight(engine, oracle_kind):
    sc = make_scene(n=61, n_p=21, n_s=600, n_b=0, seed=73)
    run_case(engine, oracle_kind, sc, stamp=9420, dist_weight=(1.0, 1.0, 5.0))


def test_flat_above_the_radius_falls_back_to_the_compare_form(engine, oracle_kind):
    """match_dist_flat > match_dist_min: dist = r - flat < 0 for every neighbour inside the radius — `matched` does not follow
    from the radius test, the launcher must keep the general loop (and nothing matches: the ratios are all zero)."""
    sc = make_scene(n=61, n_p=21, n_s=600, n_b=0, seed=74)
    kw = dict(match_dist_min=0.2, match_dist_flat=0.3, match_weight=5.0)
    o = pyoracle.Oracle(oracle_kind)
    o.set_map(sc.map_xyz, sc.map_label, dist_weight=(1.0, 1.0, 1.0))
    o.set_likelihood_params(pyoracle.LikelihoodParams(**kw))
    want_lik, want_q = o.likelihood_measure(sc.poses, sc.scan_lik)
    try:
        engine.set_option("lik_tiled_min", 1)
        engine.set_option("strict_order", 0)
        engine.set_map(sc.map_xyz, sc.map_label, stamp=9430, dist_weight=(1.0, 1.0, 1.0))
        engine.set_likelihood_params(**kw)
        lik, ratio, _ = engine.measure_batch(sc.poses, sc.scan_lik)
        assert int(engine.get_option("lik_tiled_fast")) == -1 and int(engine.get_option("lik_tiled_fast_active")) == 0
        assert int(engine.get_option("lik_defer_active")) == 1   # (the map is a common one: the parameters alone decide)
        np.testing.assert_array_equal(lik, want_lik)
        np.testing.assert_array_equal(ratio, want_q)
        assert not ratio.any()
        # flat == r is the last admissible value: matched with dist == +0
        engine.set_likelihood_params(match_dist_min=0.2, match_dist_flat=0.2, match_weight=5.0)
        engine.measure_batch(sc.poses, sc.scan_lik)
        assert int(engine.get_option("lik_tiled_fast_active")) == 1
    finally:
        engine.set_option("lik_tiled_min", 1024)
        engine.set_option("strict_order", 2)
        engine.set_likelihood_params()
    sc2 = make_scene(n=61, n_p=21, n_s=600, n_b=0, seed=74)
    run_case(engine, oracle_kind, sc2, stamp=9431, lik_kw=dict(match_dist_min=0.2, match_dist_flat=0.2, match_weight=5.0))


def test_points_the_grid_never_sees(engine, oracle_kind):
    """Scan points far outside the grid (their voxel coordinates saturate), one NaN coordinate (no match: the oracle gets that
    point moved far away instead, which adds the same zero term) and a particle whose quaternion is not normalised."""
    sc = make_scene(n=61, n_p=21, n_s=600, n_b=0, seed=75)
    scan = sc.scan_lik.copy()
    scan[5] = (4.0e4, -3.0e4, 12.0)
    scan[17] = (1.0e30, 0.0, 0.0)
    scan[300] = (-2.5e9, 2.5e9, -2.5e9)
    sc.scan_lik = scan
    sc.poses = sc.poses.copy()
    sc.poses[3, 3:] *= 1.7
    sc.poses[20, 3:] *= 0.25
    run_case(engine, oracle_kind, sc, stamp=9440)
    with_nan = scan.copy()
    with_nan[44, 1] = np.nan
    moved = scan.copy()
    moved[44] = (7.0e4, 7.0e4, 7.0e4)
    sc.scan_lik = with_nan
    run_case(engine, oracle_kind, sc, stamp=9441, oracle_scan=moved)


@pytest.mark.parametrize("options", [dict(cand_packed=0), dict(cand_record_parts=8)], ids=["plain_words", "records_128"])
def test_a_map_that_is_not_the_common_one_takes_the_general_loop(engine, oracle_kind, options):
    sc = make_scene(n=61, n_p=21, n_s=600, n_b=0, seed=76)
    run_case(engine, oracle_kind, sc, stamp=9450 + len(options), options=options, want_fast=0)
