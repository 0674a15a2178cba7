"""The likelihood indices kilometres from their grid's origin (tests/long_map_cases.py): corridors of 2.2 km (r = 0.05 m: 830 m;
far from the coordinate origin: 3.3 km) whose candidate grid has 22 000 to 45 000 voxels along one axis, where the float voxel
index of a query is off by more than the 1e-3 of a voxel that V+ used to allow. Queries on and around voxel faces at the far
stations, constructed (q, p, p') triples at which a candidate list compiled for the wrong box drops the true nearest neighbour,
and points near map points — likelihoods, match ratios and radius searches must be the oracle's, bit for bit (strict_order 1:
the reference's float sums), through the candidate index and the cell grid, the tiled and the per-particle kernel, after map
updates by rebuild and by the incremental path. No tolerance anywhere."""
import numpy as np
import pytest

import long_map_cases as L
from mcl_3dl_amd import capi
from oracle import pyoracle

pytestmark = pytest.mark.gpu

TILED_PARTICLES = 2048   # with exact sums the tiled kernel (and its replay) takes over from this many particles (host_measure.h)


class Reference:
    """One variant's case, its queries and the oracle's answers — computed once, shared by every test of the variant."""

    def __init__(self, name, kind):
        self.case = c = L.make_case(name)
        self.kind = kind
        self.faces = None

    def ready(self, geom):
        if self.faces is not None:
            return self
        c = self.case
        self.faces = L.face_queries(c, geom)
        self.queries = np.concatenate([self.faces, c["triples_q"], L.near_queries(c)], 0)
        self.identity = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
        far_centre = c["map_xyz"][c["n_base"] - 1].astype(np.float64)   # a point of the last station
        self.poses, self.scan_local = L.posed(self.queries, far_centre, 8, c["seed"])
        o = pyoracle.Oracle(self.kind)
        o.set_map(c["map_xyz"], None, dist_weight=c["dist_weight"] or (1.0, 1.0, 1.0))
        o.set_likelihood_params(pyoracle.LikelihoodParams(match_dist_min=c["r"], match_dist_flat=c["r"] / 4))
        self.want_abs = o.likelihood_measure(self.identity, self.queries)
        self.want_triples = o.likelihood_measure(self.identity, c["triples_q"])
        self.want_posed = o.likelihood_measure(self.poses, self.scan_local)
        self.want_search = o.radius_search(self.queries, c["r"])
        o.close()
        return self


_refs = {}
_stamp = [7000]


def reference(name, kind):
    if name not in _refs:
        _refs[name] = Reference(name, kind)
    return _refs[name]


def install(eng, c, stamp, lik_index):
    eng.set_option("strict_order", 1)
    eng.set_option("lik_index", lik_index)
    eng.set_option("cand_voxel_ratio", L.VOXEL_RATIO)
    eng.set_option("cand_phase", L.PHASE)
    eng.set_map(c["map_xyz"], None, stamp=stamp, dist_weight=c["dist_weight"] or (1.0, 1.0, 1.0))
    eng.set_likelihood_params(match_dist_min=c["r"], match_dist_flat=c["r"] / 4)


def restore(eng):
    for k, v in (("strict_order", 2), ("lik_index", 2), ("cand_voxel_ratio", 0.0), ("cand_phase", 0.5), ("lik_tiled", 1),
                 ("lik_group", 0)):
        eng.set_option(k, v)
    eng.set_likelihood_params()


def engine_geometry(eng, c):
    """Builds the candidate index (one query) and reads its geometry back."""
    eng.set_option("lik_index", 2)
    eng.measure_batch(np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32), c["map_xyz"][:4])
    return eng.index_geometry()


def check_search(eng, ref):
    idx, sq = eng.radius_search(ref.queries, ref.case["r"])
    found, w_idx, w_sq = ref.want_search
    np.testing.assert_array_equal(idx >= 0, found > 0)
    f = found > 0
    np.testing.assert_array_equal(idx[f], w_idx[f])
    np.testing.assert_array_equal(sq[f], w_sq[f])
    assert f.sum() > len(f) // 3


@pytest.mark.parametrize("kernel", ["tiled", "per_particle"])
@pytest.mark.parametrize("lik_index", [2, 0])
@pytest.mark.parametrize("variant", list(L.VARIANTS))
def test_long_corridor_is_exact(engine, oracle_kind, variant, lik_index, kernel):
    ref = reference(variant, oracle_kind)
    c = ref.case
    try:
        _stamp[0] += 1
        install(engine, c, _stamp[0], lik_index)
        geom = engine_geometry(engine, c)
        engine.set_option("lik_index", lik_index)
        # the generator's restatement of the geometry is the engine's: the triples were built for this grid
        np.testing.assert_array_equal(geom["origin"], c["geom"]["origin"])
        np.testing.assert_array_equal(geom["edge"], c["geom"]["edge"])
        np.testing.assert_array_equal(geom["voxels"], c["geom"]["voxels"])
        assert geom["grow"] == c["geom"]["grow"] > 2.0 * c["geom"]["grow_fixed"]
        ref.ready(geom)
        assert len(c["triples_q"]) >= L.MIN_TRIPLES and len(ref.queries) >= 4000 + L.MIN_TRIPLES
        rep = TILED_PARTICLES if kernel == "tiled" else 1
        engine.set_option("lik_tiled", 1 if kernel == "tiled" else 0)
        engine.set_option("lik_group", 8 if kernel == "tiled" else 0)
        runs = [("absolute queries, identity pose", np.repeat(ref.identity, rep, 0), ref.queries, ref.want_abs),
                ("triples alone, identity pose", np.repeat(ref.identity, rep, 0), c["triples_q"], ref.want_triples),
                ("posed particles", np.tile(ref.poses, (max(rep // 8, 1), 1)), ref.scan_local, ref.want_posed)]
        for what, poses, scan, (want_lik, want_q) in runs:
            lik, ratio, _ = engine.measure_batch(poses, scan)
            n = len(want_lik)
            print("%s %s: lik %r want %r" % (variant, what, lik[:n], want_lik))
            np.testing.assert_array_equal(ratio, np.tile(want_q, len(poses) // n), err_msg=what)
            np.testing.assert_array_equal(lik, np.tile(want_lik, len(poses) // n), err_msg=what)
            assert np.all(want_lik > 0), what
        # every triple's query has its nearest neighbour within the radius: the oracle matches them all
        assert ref.want_triples[1][0] == 1.0
        if kernel == "per_particle":
            check_search(engine, ref)
    finally:
        restore(engine)


def test_map_update_to_the_far_station_by_rebuild_and_by_increment(oracle_kind):
    """A map that ends at 1 030 m receives the far stations as a map update (outside the grid in place: the index is rebuilt),
    then a second update inside the new bounds replaces it (the incremental path): exact both times."""
    c = L.make_case("along_x")
    xyz = c["map_xyz"]
    base = xyz[(xyz[:, 0] < 1100.0)]
    far = xyz[(xyz[:, 0] >= 1100.0)]
    second = far[(far[:, 0] < 2205.0)]          # without the zone behind the last station: bounds inside the first update's
    leaf = (0.05, 0.05, 0.05)
    eng = capi.Engine(0)
    try:
        eng.set_option("strict_order", 1)
        eng.set_option("cand_voxel_ratio", L.VOXEL_RATIO)
        eng.set_map(base, None, stamp=1)
        eng.set_likelihood_params(match_dist_min=c["r"], match_dist_flat=c["r"] / 4)
        identity = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
        eng.measure_batch(identity, base[:64])   # builds the index of the short map
        assert eng.index_geometry()["voxels"][0] < 11000
        for step, (upd, outcome) in enumerate([(far, 4), (second, 0)]):
            n_map, stats = eng.map_update(upd, None, leaf=leaf, stamp=10 + step)
            assert stats["outcome"] == outcome, stats
            merged, _ = eng.map_download()
            assert n_map == len(merged) > len(base) + 1000
            case = dict(c, map_xyz=merged)
            geom = engine_geometry(eng, case)
            assert geom["voxels"][0] > 22000 and geom["grow"] > 4.0 * 1e-3 * geom["edge"].min()
            queries = np.concatenate([L.face_queries(case, geom), L.near_queries(case)], 0)
            poses, scan_local = L.posed(queries, merged[len(base) + 5].astype(np.float64), 8, step)
            o = pyoracle.Oracle(oracle_kind)
            o.set_map(merged, None)
            o.set_likelihood_params(pyoracle.LikelihoodParams(match_dist_min=c["r"], match_dist_flat=c["r"] / 4))
            for p, s in ((identity, queries), (poses, scan_local)):
                want_lik, want_q = o.likelihood_measure(p, s)
                lik, ratio, _ = eng.measure_batch(p, s)
                print("update %d (%s): lik %r want %r" % (step, stats, lik, want_lik))
                np.testing.assert_array_equal(ratio, want_q)
                np.testing.assert_array_equal(lik, want_lik)
                assert np.all(want_lik > 0)
            found, w_idx, w_sq = o.radius_search(queries, c["r"])
            o.close()
            idx, sq = eng.radius_search(queries, c["r"])
            np.testing.assert_array_equal(idx >= 0, found > 0)
            np.testing.assert_array_equal(idx[found > 0], w_idx[found > 0])
            np.testing.assert_array_equal(sq[found > 0], w_sq[found > 0])
    finally:
        eng.close()


def test_a_map_past_the_slack_limit_is_refused_and_the_context_lives_on(oracle_kind):
    """Two clusters 9 km apart at r = 0.05 m (voxels of 0.025 m: 360 000 along x; the slack would pass 1/16 of a voxel at 322 000)
    and 180 000 cells of the cell grid (the 27-cell scan is exact up to 40 000): both indices refuse with -4; with r = 0.25 m the
    same context answers exactly."""
    rng = np.random.default_rng(5)
    cluster = rng.uniform(0.0, 0.3, (300, 3))
    xyz = np.concatenate([cluster, cluster + [9000.0, 0.0, 0.0]], 0).astype(np.float32)
    queries = (xyz[rng.integers(0, len(xyz), 1500)] + rng.normal(0, 0.02, (1500, 3))).astype(np.float32)
    identity = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
    eng = capi.Engine(0)
    try:
        eng.set_option("strict_order", 1)
        eng.set_map(xyz, None, stamp=1)
        eng.set_likelihood_params(match_dist_min=0.05, match_dist_flat=0.01)
        for lik_index, word in ((2, "1/16"), (0, "27-cell")):
            eng.set_option("lik_index", lik_index)
            with pytest.raises(capi.EngineError, match=r"error -4: .*" + word):
                eng.measure_batch(identity, queries)
        o = pyoracle.Oracle(oracle_kind)
        o.set_map(xyz, None)
        o.set_likelihood_params(pyoracle.LikelihoodParams(match_dist_min=0.25, match_dist_flat=0.05))
        want_lik, want_q = o.likelihood_measure(identity, queries)
        o.close()
        eng.set_likelihood_params(match_dist_min=0.25, match_dist_flat=0.05)
        for lik_index in (2, 0):
            eng.set_option("lik_index", lik_index)
            lik, ratio, _ = eng.measure_batch(identity, queries)
            np.testing.assert_array_equal(lik, want_lik)
            np.testing.assert_array_equal(ratio, want_q)
        assert want_q[0] > 0.9
    finally:
        eng.close()
