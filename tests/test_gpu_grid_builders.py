"""The two linear-time map structures — the cell-sorted exact-NN grid and the DDA occupancy / voxel index — from their device
form and from their sequential host form (option grid_build_host), on the small maps at which a key, a clamp or an
installation can go wrong: the two forms share their statements (index_geometry.h, host_grid_builders.h) and must answer
every query with the same bits. On the maps without duplicate points the reference answers too. Then map updates on the
cell grid (merge / rebuild) and on the DDA grid (overlay / rebuild) against fresh engines on the merged map."""
import numpy as np
import pytest

from mcl_3dl_amd import capi
from oracle import pyoracle

pytestmark = pytest.mark.gpu

F32 = np.float32
DW = (1.0, 1.0, 5.0)
RADII = (0.2, 0.5)
GRID = 0.25            # dda_grid_size of every map here


def one_point():
    return np.array([[1.5, -2.25, 0.75]], F32), np.array([1], np.uint32), None


def column():
    """65 copies of one point and one far point straight above: a DDA grid of 1 x 1 x 25 voxels, a cell grid that is nothing
    but its margins in x and y, every point in one of two cells (65: past one wavefront's worth in a run)"""
    xyz = np.concatenate([np.tile(np.array([[0.5, 0.5, 0.25]], F32), (65, 1)), np.array([[0.5, 0.5, 6.25]], F32)])
    return xyz, (np.arange(66) % 3).astype(np.uint32), None


def five_four_three():
    """DDA dimensions 5 x 4 x 3 at a grid of 0.25 (extents 1.1, 0.8, 0.6: the bricks are not full), points on both corners"""
    rng = np.random.default_rng(5)
    lo, hi = np.array([-0.5, 0.25, 1.0]), np.array([0.6, 1.05, 1.6])
    xyz = np.concatenate([(lo + rng.random((120, 3)) * (hi - lo)).astype(F32), np.array([lo, hi], F32)])
    return xyz, (np.arange(len(xyz)) % 3).astype(np.uint32), None


def slab():
    """a jittered 200-point slab with a dist_weight and labels"""
    rng = np.random.default_rng(9)
    g = np.stack(np.meshgrid(np.arange(20), np.arange(10), indexing="ij"), -1).reshape(-1, 2) * 0.3
    xyz = np.c_[g, np.full(len(g), 0.5)] + rng.normal(0, 0.04, (len(g), 3))
    return xyz.astype(F32), (np.arange(len(xyz)) % 3).astype(np.uint32), DW


MAPS = {"one_point": one_point, "column_of_duplicates": column, "dda_5x4x3": five_four_three, "slab": slab}
NO_DUPLICATES = ("one_point", "dda_5x4x3", "slab")


def queries_for(xyz):
    """near every kind of place: map points, jittered ones, outside the grid on every side, a NaN"""
    rng = np.random.default_rng(3)
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    near = xyz[rng.integers(0, len(xyz), 150)] + rng.normal(0, 0.15, (150, 3))
    outside = []
    for a in range(3):
        for side, d in ((lo, -1.0), (hi, 1.0)):
            for dist in (0.1, 0.45, 0.9, 30.0):
                p = (lo + hi) / 2
                p[a] = side[a] + d * dist
                outside.append(p)
    return np.concatenate([xyz[:40], near, np.array(outside), [[np.nan, 0.0, 0.0]]]).astype(F32)


def rays_for(xyz):
    """rays that start inside, start outside, run along a face of the grid, or have zero length"""
    rng = np.random.default_rng(4)
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    mid, ext = (lo + hi) / 2, np.maximum(hi - lo, 0.5)
    inside_b = lo + rng.random((60, 3)) * (hi - lo)
    inside_e = xyz[rng.integers(0, len(xyz), 60)] + rng.normal(0, 0.3, (60, 3))
    outside_b = mid + rng.normal(0, 1.0, (60, 3)) * ext * 2
    outside_e = xyz[rng.integers(0, len(xyz), 60)].astype(np.float64)
    face_b, face_e = [], []
    for a in range(3):
        for side in (lo, hi):
            b, e = lo.copy(), hi.copy()
            b[a] = e[a] = side[a]
            face_b.append(b)
            face_e.append(e)
    zero = xyz[:4].astype(np.float64)
    begin = np.concatenate([inside_b, outside_b, face_b, zero, mid[None]])
    end = np.concatenate([inside_e, outside_e, face_e, zero, mid[None]])
    return begin.astype(F32), end.astype(F32)


def scene_for(xyz):
    """16 poses around the map and a 64-point scan, a split pose"""
    rng = np.random.default_rng(6)
    mid = ((xyz.min(0) + xyz.max(0)) / 2).astype(np.float64)
    poses = np.zeros((16, 7), F32)
    poses[:, :3] = mid + rng.normal(0, 0.1, (16, 3))
    yaw = rng.normal(0, 0.05, 16)
    poses[:, 5], poses[:, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    scan = (xyz[rng.integers(0, len(xyz), 64)] - mid + rng.normal(0, 0.08, (64, 3))).astype(F32)
    return poses, scan


def answers(eng, xyz):
    """every query the two structures serve, as a flat list of arrays"""
    q = queries_for(xyz)
    begin, end = rays_for(xyz)
    poses, scan = scene_for(xyz)
    out = []
    for r in RADII:
        out += list(eng.radius_search(q, r))
    out += list(eng.beam_status(begin, end))
    for k in range(len(begin)):                     # every ray: the face rays and the zero-length ones among them
        wp, collided, hit, n = eng.dda_trace(begin[k], end[k])
        out += [wp, np.array([collided, hit, n])]
    out += list(eng.match_split(poses[0], scan + F32(0.0), unmatch_dist=0.5, match_dist=0.1))
    out += list(eng.measure_batch(poses, scan)[:2])
    return out


def make_engine(mode, xyz, label, dw, stamp):
    eng = capi.Engine(0)
    eng.set_option("grid_build_host", mode)
    eng.set_option("lik_index", 0)
    eng.set_map(xyz, label, stamp=stamp, dist_weight=dw)
    eng.set_likelihood_params()
    eng.set_beam_params(dda_grid_size=GRID, num_points=8, filter_label_max=1)
    return eng


def assert_same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg="%s, array %d" % (what, k))


@pytest.mark.parametrize("name", list(MAPS))
def test_both_forms_answer_alike_and_as_the_reference(name):
    xyz, label, dw = MAPS[name]()
    out = {}
    for mode in (0, 1):
        eng = make_engine(mode, xyz, label, dw, stamp=70 + mode)
        try:
            out[mode] = answers(eng, xyz)
            assert eng.get_option("grid_build_host") == mode
        finally:
            eng.close()
    assert_same(out[0], out[1], name)
    idx = out[0][0]
    assert (idx[:min(40, len(xyz))] >= 0).all() and idx[-1] < 0            # map points find themselves, the NaN nothing
    assert (idx < 0).sum() >= 6                                            # ... and the queries far outside nothing either
    if name in ("dda_5x4x3", "slab"):
        assert (out[0][2 * len(RADII) + 1] >= 0).any()                     # some ray collides with a map point
    if name not in NO_DUPLICATES:
        return
    ref = pyoracle.Oracle("ref")
    try:
        ref.set_map(xyz, label, dist_weight=dw)
        ref.set_likelihood_params(pyoracle.LikelihoodParams())
        ref.set_beam_params(pyoracle.BeamParams(dda_grid_size=GRID, num_points=8, filter_label_max=1))
        q = queries_for(xyz)[:-1]                                          # (the kd-tree is not asked about the NaN)
        for k, r in enumerate(RADII):
            found, w_idx, _ = ref.radius_search(q, r)
            got = out[0][2 * k][:-1]
            np.testing.assert_array_equal(got >= 0, found > 0)
            np.testing.assert_array_equal(got[found > 0], w_idx[found > 0])
        w_st, w_hit = ref.beam_status(*rays_for(xyz))
        np.testing.assert_array_equal(out[0][2 * len(RADII)], w_st)
        np.testing.assert_array_equal(out[0][2 * len(RADII) + 1], w_hit)
    finally:
        ref.close()


def test_map_updates_merge_overlay_or_rebuild_and_equal_fresh_engines():
    xyz, label, dw = slab()
    n_base = len(xyz)
    lo, hi = xyz.min(0), xyz.max(0)
    lowest, highest = xyz[np.lexsort((xyz[:, 0], xyz[:, 1], xyz[:, 2]))[[0, -1]]]
    rng = np.random.default_rng(11)
    inside = (lo + rng.random((40, 3)) * (hi - lo)).astype(F32)
    updates = [
        ("one point", inside[:1], True),
        ("lowest and highest occupied cell", np.array([lowest, highest, lo, hi], F32), True),
        ("a larger one", inside, True),
        ("replaced by a smaller one", inside[5:12], True),
        ("withdrawn", np.zeros((0, 3), F32), True),
        ("leaves the bounds", np.concatenate([inside[:6], [hi + F32(1.5)]]).astype(F32), False),
    ]
    inc = make_engine(0, xyz, label, dw, stamp=1)
    try:
        answers(inc, xyz)                                                  # builds both grids on the base map
        for step, (what, upd, stays) in enumerate(updates):
            r0, m0 = inc.get_option("lik_grid_rebuilds"), inc.get_option("lik_grid_merges")
            o0 = inc.get_option("dda_overlay_updates")
            lab = (np.arange(len(upd)) % 3).astype(np.uint32)
            n_map, _ = inc.map_update(upd, lab, leaf=None, stamp=10 + step)
            assert n_map == n_base + len(upd)
            m_xyz, m_lab = inc.map_download()
            np.testing.assert_array_equal(m_xyz[n_base:], upd)
            got = answers(inc, xyz)
            for mode in (0, 1):
                fresh = make_engine(mode, m_xyz, m_lab, dw, stamp=100 + 2 * step + mode)
                try:
                    assert_same(got, answers(fresh, xyz), "%s, fresh engine with grid_build_host %d" % (what, mode))
                finally:
                    fresh.close()
            r1, m1 = inc.get_option("lik_grid_rebuilds"), inc.get_option("lik_grid_merges")
            o1 = inc.get_option("dda_overlay_updates")
            # the cell grid: a merge when there is something to merge, one rebuild for the update that left the bounds
            assert (r1 - r0, m1 - m0) == ((0, 1 if len(upd) else 0) if stays else (1, 0)), (what, r0, r1, m0, m1)
            # the DDA grid: the overlay when and only when the update stayed inside, and then all of the update is in it
            assert o1 - o0 == (1 if stays else 0), (what, o0, o1)
            assert inc.get_option("dda_overlay_points") == (len(upd) if stays else 0), what
    finally:
        inc.close()
