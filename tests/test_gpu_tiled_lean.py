"""The tiled update's leaner forms against the general loop, the oracle and the launches apart.

  * unit weights: the common-map pose loop is compiled for three forms of the dist_weight (LikParams::unit_form: a weight
    the host has seen to be exactly 1.0f is not multiplied by) and picked once per launch. (1,1,1) is form 2, the reference's
    shipped (1,1,5) form 1, (2,1,1) and (1,3,1) form 0. tests/test_gpu_tiled_fast.py's method (run_case: lik_tiled_min = 1, both
    loops, strict_order 0 and 3, the default mode against the oracle bit for bit) on one scene at the four weights, on the
    map of centroids (the deferred queue's rounds take the same form) and in the merged launch of an update with beam points.
  * term slots: the terms lie in LDS in the order the fp64 sum reads them (term_slots.h) for 4, 8 and 16 particles per
    work-group; the queue's rounds and the strict_order = 1 term writer go through the same mapping.
  * the tail: lik_pf_partial_kernel issues every load before its first add (unrolled up to 64 tiles, the loop beyond) and
    pf_apply_kernel reads its element before the reduction. Same arithmetic in the same association, so one update equals
    measure_batch (lik_finalize_kernel's sums) followed by pf_measure on its results, bit for bit — at 2 tiles, at 64 (the
    unrolled form's last size), at 65 (the loop), for particle counts that take the split form, one of them no multiple of 64.
"""
import numpy as np
import pytest

from mcl_3dl_amd.synthetic import make_scene
from test_gpu_tiled_fast import run_case

pytestmark = pytest.mark.gpu

WEIGHTS = [(1.0, 1.0, 1.0), (1.0, 1.0, 5.0), (2.0, 1.0, 1.0), (1.0, 3.0, 1.0)]
WEIGHT_IDS = ["form2_unit", "form1_z5", "form0_x2", "form0_y3"]


@pytest.mark.parametrize("dist_weight", WEIGHTS, ids=WEIGHT_IDS)
def test_one_scene_at_the_four_weight_forms(engine, oracle_kind, dist_weight):
    """300 x 21: two tiles, the second with 44 points, and a last particle group of five."""
    sc = make_scene(n=61, n_p=21, n_s=300, n_b=0, seed=91)
    run_case(engine, oracle_kind, sc, stamp=9500 + WEIGHTS.index(dist_weight), dist_weight=dist_weight)


@pytest.mark.parametrize("dist_weight", WEIGHTS[:2], ids=WEIGHT_IDS[:2])
def test_five_tiles_and_three_groups(engine, oracle_kind, dist_weight):
    """1030 x 40: five tiles, the last with six points; groups of 16, 16 and 8."""
    sc = make_scene(n=61, n_p=40, n_s=1030, n_b=0, seed=92)
    run_case(engine, oracle_kind, sc, stamp=9510 + WEIGHTS.index(dist_weight), dist_weight=dist_weight)


@pytest.mark.parametrize("dist_weight", WEIGHTS[:3], ids=WEIGHT_IDS[:3])
def test_map_of_centroids_drains_the_queue_in_the_same_form(engine, oracle_kind, dist_weight):
    sc = make_scene(n=58, n_p=48, n_s=600, n_b=0, seed=93, map_jitter=0.045)
    stamp = 9520 + WEIGHTS.index(dist_weight)
    run_case(engine, oracle_kind, sc, stamp=stamp, dist_weight=dist_weight)
    engine.set_option("lik_tiled_min", 1)
    try:
        engine.set_map(sc.map_xyz, sc.map_label, stamp=stamp, dist_weight=dist_weight)
        engine.measure_batch(sc.poses, sc.scan_lik)
        st = engine.index_stats()
        assert st["voxels_with_overflow"] > 0 and st["deferred_overflow"] == 1
    finally:
        engine.set_option("lik_tiled_min", 1024)


@pytest.mark.parametrize("dist_weight", WEIGHTS[:3], ids=WEIGHT_IDS[:3])
def test_update_with_beam_points_runs_the_same_body(engine, dist_weight):
    """600 x 21 with 32 beam points: the merged launch of both models calls the tiled body; weights, likelihoods and beam
    scores equal between the common-map loop and the general one."""
    sc = make_scene(n=61, n_p=21, n_s=600, n_b=32, seed=94)
    w0 = np.random.default_rng(94).uniform(0.1, 1.0, 21).astype(np.float32)
    out = {}
    try:
        engine.set_option("lik_tiled_min", 1)
        engine.set_option("strict_order", 0)
        engine.set_map(sc.map_xyz, sc.map_label, stamp=9530 + WEIGHTS.index(dist_weight), dist_weight=dist_weight)
        engine.set_likelihood_params()
        engine.set_beam_params(num_points=32)
        for fast in (-1, 0):
            engine.set_option("lik_tiled_fast", fast)
            out[fast] = engine.measure_update(sc.poses, w0, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
            assert int(engine.get_option("lik_tiled_fast_active")) == (1 if fast else 0)
    finally:
        engine.set_option("lik_tiled_fast", -1)
        engine.set_option("strict_order", 2)
        engine.set_option("lik_tiled_min", 1024)
    for k in ("weights", "lik", "quality", "beam"):
        np.testing.assert_array_equal(out[-1][k], out[0][k], err_msg=k)
    assert out[-1]["entropy"] == out[0]["entropy"]
    assert np.count_nonzero(out[-1]["quality"]) > 0 and np.ptp(out[-1]["beam"]) > 0


@pytest.mark.parametrize("group", [4, 8, 16, 32])
def test_every_group_size_on_the_map_of_centroids(engine, oracle_kind, group):
    """The particles per work-group decide the slot mapping (4, 8, 16: the reader's order, each with its own swizzle; 32: array
    order). At these shapes a launch would pick 4 on its own, so the size is forced (option lik_group); 600 x 70 leaves a last
    group of 6 (of 14 for 8, of 2 for 4)."""
    sc = make_scene(n=58, n_p=70, n_s=600, n_b=0, seed=97, map_jitter=0.045)
    try:
        run_case(engine, oracle_kind, sc, stamp=9550 + group, options=dict(lik_group=group))
    finally:
        engine.set_option("lik_group", 0)


@pytest.mark.parametrize("group", [0, 8, 16])
@pytest.mark.parametrize("n_s,n_p,jitter", [(300, 21, 0.0), (600, 48, 0.045)], ids=["300x21", "600x48_centroids"])
def test_strict_order_1_reads_the_terms_through_the_slots(engine, oracle_kind, n_s, n_p, jitter, group):
    """strict_order = 1: the kernel's term-array writer copies every float term out of LDS, where the terms now lie in the fp64
    reader's order (term_slots.h), and the rows are added in the reference's order: the oracle's likelihoods in the caller's
    order, bit for bit, from both loops. The map of centroids parks best-so-far values in the slots and replaces them from the
    queue's rounds."""
    from oracle import pyoracle
    sc = make_scene(n=58 if jitter else 61, n_p=n_p, n_s=n_s, n_b=0, seed=96, map_jitter=jitter)
    o = pyoracle.Oracle(oracle_kind)
    o.set_map(sc.map_xyz, sc.map_label, dist_weight=(1.0, 1.0, 1.0))
    o.set_likelihood_params(pyoracle.LikelihoodParams())
    want_lik, want_q = o.likelihood_measure(sc.poses, sc.scan_lik)
    try:
        engine.set_option("lik_tiled_min", 1)
        engine.set_option("strict_order", 1)
        engine.set_option("lik_group", group)   # (0: the launch picks 4 at these shapes)
        engine.set_map(sc.map_xyz, sc.map_label, stamp=9560 + n_p, dist_weight=(1.0, 1.0, 1.0))
        engine.set_likelihood_params()
        for fast in (-1, 0):
            engine.set_option("lik_tiled_fast", fast)
            lik, ratio, _ = engine.measure_batch(sc.poses, sc.scan_lik)
            assert int(engine.get_option("lik_tiled_fast_active")) == (1 if fast else 0)
            np.testing.assert_array_equal(lik, want_lik)
            np.testing.assert_array_equal(ratio, want_q)
        if jitter:
            assert engine.index_stats()["voxels_with_overflow"] > 0
        assert np.count_nonzero(want_q) > 0
    finally:
        engine.set_option("lik_group", 0)
        engine.set_option("lik_tiled_fast", -1)
        engine.set_option("strict_order", 2)
        engine.set_option("lik_tiled_min", 1024)


@pytest.fixture(scope="module")
def tail_scene():
    return make_scene(n=91, n_p=4096, n_s=16640, n_b=0, seed=95)


@pytest.mark.parametrize("n_s", [300, 16384, 16640], ids=["2_tiles", "64_tiles", "65_tiles"])
@pytest.mark.parametrize("n_p", [2049, 2500, 4096])
def test_the_tail_behind_the_tiled_kernel_equals_the_launches_apart(engine, tail_scene, n_p, n_s):
    sc = tail_scene
    poses, scan = sc.poses[:n_p], sc.scan_lik[:n_s]
    rng = np.random.default_rng(n_p + n_s)
    w0 = rng.uniform(0.0, 1.0, n_p).astype(np.float32)
    w0[::7] = 0.0
    extra = rng.uniform(0.1, 0.4, n_p).astype(np.float32)
    try:
        engine.set_option("lik_tiled_min", 1)
        engine.set_option("strict_order", 0)
        engine.set_map(sc.map_xyz, sc.map_label, stamp=9540, dist_weight=(1.0, 1.0, 1.0))
        engine.set_likelihood_params()
        for ex in (None, extra):
            one = engine.measure_update(poses, w0, scan, extra=ex)
            lik, ratio, bscore = engine.measure_batch(poses, scan)
            apart = engine.pf_measure(w0, lik, bscore, ex, ratio)
            np.testing.assert_array_equal(one["lik"], lik)
            np.testing.assert_array_equal(one["quality"], ratio)
            np.testing.assert_array_equal(one["weights"], apart["weights"])
            assert one["entropy"] == apart["entropy"] and one["restored"] == apart["restored"] is False
            assert one["match_ratio_min"] == apart["match_ratio_min"] and one["match_ratio_max"] == apart["match_ratio_max"]
            # what the weights are, from the likelihoods: w * lik (* extra) over the float of their fp64 sum (pf.h:258-272; the
            # sum's last bit depends on the order of the adds, hence one ulp for the quotient)
            wn = w0 * (lik if ex is None else lik * ex)
            want = wn / np.float32(wn.astype(np.float64).sum())
            np.testing.assert_allclose(one["weights"], want, rtol=2.0 ** -22, atol=0)
            assert np.count_nonzero(ratio) > 0 and np.count_nonzero(one["weights"]) > 0
    finally:
        engine.set_option("strict_order", 2)
        engine.set_option("lik_tiled_min", 1024)
