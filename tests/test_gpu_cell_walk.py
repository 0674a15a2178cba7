"""GPU tests of the walk over the cell-sorted map (csrc/cell_grid.h) at the places where its callers could drift apart:
mcl3dl_hip_radius_search, match_split, the kd-tree caster's searches and the 27-cell likelihood scan, on ONE tiny map.

The map: about 200 points in 3 x 2 x 2 cells of a grid of 7 x 6 x 6 (the builder puts two empty cells around the points on every
side; 7 x 6 x 12 with dist_weight (1, 1, 5)), two of the twelve inner cells emptied, two pairs of exactly coincident points.

Expected values are brute force in numpy float32 — flann::L2_Simple's ((dx*dx) + dy*dy) + dz*dz, strict `<` against
float32(float64(r) * r), the lowest map index on ties — which is exact: index and squared distance are compared with
assert_array_equal, nothing here has a tolerance.

The engine derives the reach of a stand-alone search as ceil(r / cell) + 1 >= 2, so radius_search runs reach 2, 3 and 4: five
rows of a layer (one batch of the five-row forms), seven (two batches, the second partial) and nine (5 + 4). Reach 1 — three
rows — is match_split's first pass (every call with reach > 1 starts with it) and the kd-tree caster's first search on the 0.202 m
grid, whose interior cells take the nine-row fetch and whose border cells the general form."""
import functools

import numpy as np
import pytest

import beam_kdtree_cases as cases
from mcl_3dl_amd import capi

pytestmark = pytest.mark.gpu

DW5 = (1.0, 1.0, 5.0)
MATCH_DIST_MIN = np.float32(0.2)
CELL = MATCH_DIST_MIN * np.float32(1.01)   # lik_cell_edge
INV = np.float32(1.0) / CELL
RADII = {0.15: 2, 0.3: 3, 0.5: 4}          # radius -> ceil(r / cell) + 1


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def tiny_map():
    rng = np.random.default_rng(20261)
    c = float(CELL)
    ext = np.array([2.5, 1.5, 1.5]) * c
    base = np.array([1.0, -0.5, 0.3])
    p = rng.uniform(0.0, 1.0, (230, 3)) * ext
    p[0], p[1] = 0.0, ext                       # the corners: the grid's extent does not depend on the draw
    local = np.floor(p / c).astype(int)
    hole = (np.all(local == (1, 0, 1), 1) | np.all(local == (2, 1, 0), 1))
    p = p[~hole][:198]
    xyz = (p + base).astype(np.float32)
    xyz = np.concatenate([xyz, xyz[[10, 20]]], 0)   # 198 = copy of 10, 199 = copy of 20: exact ties, the lower index wins
    xyz = np.ascontiguousarray(xyz)
    xyz.setflags(write=False)
    return xyz


def rescaled(a, dist_weight):
    a = np.asarray(a, np.float32)
    return a if dist_weight is None else a * np.asarray(dist_weight, np.float32)   # one float product per coordinate


def grid_of(dist_weight):
    """(origin, dims) of the cell grid over the rescaled map, in index_geometry.h's float expressions."""
    s = rescaled(tiny_map(), dist_weight)
    mn, mx = s.min(0), s.max(0)
    o = mn - np.float32(2.0) * CELL
    dim = np.floor((mx - o) * INV).astype(int) + 3
    return o, dim


def cell_centre(o, idx):
    return o + (np.asarray(idx, np.float32) + np.float32(0.5)) * CELL


def queries(dist_weight, reach):
    """Unscaled query points whose rescaled positions are: the centre of every cell, the cells 0.5, `reach` and `reach + 1`
    cells outside each of the six faces, the coincident map points, NaN and +inf."""
    o, dim = grid_of(dist_weight)
    ii = np.stack(np.meshgrid(*[np.arange(d) for d in dim], indexing="ij"), -1).reshape(-1, 3)
    q = [cell_centre(o, ii)]
    mid = dim // 2
    for axis in range(3):
        for k in (-1, -reach, -reach - 1, dim[axis], dim[axis] - 1 + reach, dim[axis] + reach):
            c = mid.copy()
            c[axis] = k
            q.append(cell_centre(o, c)[None])
    q = np.concatenate(q, 0)
    if dist_weight is not None:
        q = q / np.asarray(dist_weight, np.float32)
    m = tiny_map()
    q = np.concatenate([q, m[[10, 20, 198]], m[[10, 20]] + np.float32(0.01)], 0).astype(np.float32)
    special = np.array([[np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0]], np.float32)
    return np.ascontiguousarray(q), special


def brute_force(query, radius, dist_weight):
    """(index, squared distance) of the nearest map point with d2 < r2, -1 / -1.0 where there is none."""
    m = rescaled(tiny_map(), dist_weight)
    q = rescaled(query, dist_weight)
    r = np.float32(radius)
    r2 = np.float32(np.float64(r) * np.float64(r))
    with np.errstate(invalid="ignore"):
        dx, dy, dz = (q[:, None, a] - m[None, :, a] for a in range(3))
        d2 = ((dx * dx) + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        cand = np.where(d2 < r2, d2, np.float32(np.inf))
    idx = np.argmin(cand, 1).astype(np.int32)           # first occurrence: the lowest index on ties
    sq = cand[np.arange(len(q)), idx]
    none = ~np.isfinite(sq)
    ties = int(np.sum((np.sum(cand == sq[:, None], 1) > 1) & ~none))
    return np.where(none, -1, idx).astype(np.int32), np.where(none, np.float32(-1.0), sq).astype(np.float32), ties


def install(e, dist_weight, stamp, match_dist_min=float(MATCH_DIST_MIN)):
    m = tiny_map()
    e.set_map(m, np.zeros(len(m), np.uint32), stamp=stamp, dist_weight=dist_weight)
    e.set_likelihood_params(match_dist_min=match_dist_min)
    e.set_beam_params()


def test_the_map_is_the_one_described():
    m = tiny_map()
    assert len(m) == 200 and np.array_equal(m[198], m[10]) and np.array_equal(m[199], m[20])
    o, dim = grid_of(None)
    assert tuple(dim) == (7, 6, 6)
    assert tuple(grid_of(DW5)[1]) == (7, 6, 12)
    cells = np.floor((m - o) * INV).astype(int)
    occupied = {tuple(c) for c in cells}
    assert len(occupied) == 10 and all(2 <= c[0] <= 4 and 2 <= c[1] <= 3 and 2 <= c[2] <= 3 for c in occupied)


@pytest.mark.parametrize("dist_weight", [None, DW5], ids=str)
@pytest.mark.parametrize("radius", sorted(RADII))
def test_radius_search_equals_brute_force(eng, radius, dist_weight):
    reach = RADII[radius]
    assert int(np.ceil(np.float32(radius) / CELL)) + 1 == reach
    install(eng, dist_weight, 9900)
    q, special = queries(dist_weight, reach)
    q = np.concatenate([q, special], 0)
    want_idx, want_sq, ties = brute_force(q, radius, dist_weight)
    found = int(np.sum(want_idx >= 0))
    print("radius %.2f (reach %d), %s: %d queries, %d find a neighbour, %d of them on a tie" % (radius, reach, dist_weight, len(q), found, ties))
    assert found >= 20 and np.sum(want_idx < 0) >= 40 and ties >= 3
    assert want_idx[-1] == -1 and want_idx[-2] == -1   # NaN, +inf
    idx, sq = eng.radius_search(q, radius)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(sq, want_sq)


@pytest.mark.parametrize("dist_weight", [None, DW5], ids=str)
@pytest.mark.parametrize("unmatch_dist", [0.15, 0.3])
def test_match_split_counts_and_membership(eng, unmatch_dist, dist_weight):
    """reach 2 and 3, each behind the first pass over the 27 cells (reach 1). The identity pose leaves the finite points as they
    are; the NaN and the +inf query, the last two, come out of the rotation's products with 0 as points with NaN coordinates:
    no cell, no neighbour — unmatched."""
    match_dist = 0.05
    install(eng, dist_weight, 9910)
    q, special = queries(dist_weight, RADII[unmatch_dist])
    want_idx, want_sq, _ = brute_force(q, unmatch_dist, dist_weight)
    want_unmatched = want_idx < 0
    want_matched = (want_idx >= 0) & (want_sq.astype(np.float64) < match_dist * match_dist)   # src/mcl_3dl.cpp:778, in double
    assert want_matched.sum() >= 5 and want_unmatched.sum() >= 40 and (~want_matched & ~want_unmatched).sum() >= 5
    pose = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
    matched, unmatched = eng.match_split(pose, np.concatenate([q, special], 0), unmatch_dist=unmatch_dist, match_dist=match_dist)
    assert (len(matched), len(unmatched)) == (int(want_matched.sum()), int(want_unmatched.sum()) + len(special))
    np.testing.assert_array_equal(matched, q[want_matched])
    np.testing.assert_array_equal(unmatched[:-len(special)], q[want_unmatched])
    assert np.all(np.any(np.isnan(unmatched[-len(special):]), 1))


@functools.lru_cache(maxsize=None)
def tiny_rays():
    """400 rays through and beside the map: begins up to three cells outside the points' box (border cells and beyond the
    grid), ends on map points (HIT / SHORT / TOTAL_REFLECTION) or anywhere in the same box (mostly LONG)."""
    rng = np.random.default_rng(20262)
    m = tiny_map()
    lo, hi = m.min(0) - 3 * float(CELL), m.max(0) + 3 * float(CELL)
    begin = rng.uniform(lo, hi, (400, 3)).astype(np.float32)
    end = rng.uniform(lo, hi, (400, 3)).astype(np.float32)
    on = rng.integers(0, len(m), 250)
    end[:250] = m[on] + rng.normal(0, 0.03, (250, 3)).astype(np.float32)
    return begin, end


@pytest.mark.parametrize("dist_weight", [None, DW5], ids=str)
@pytest.mark.parametrize("match_dist_min,reaches", [(0.2, (1, 2)), (0.06, (2, 5))])
def test_kd_caster_statuses_equal_the_oracle(eng, oracle_kind, match_dist_min, reaches, dist_weight):
    """The caster's radii on 0.1 m map grids are 0.0707 and 0.2707 m. On the 0.202 m grid they reach 1 and 2 cells: the first
    search is the nine-row fetch in interior cells and the general form in border cells. On a 0.0606 m grid they reach 2 and
    5: the general form with one full batch of five rows, and with eleven rows in three batches."""
    cell = float(np.float32(match_dist_min) * np.float32(1.01))
    assert tuple(int(np.ceil(r / cell + 0.005)) for r in (0.0707107, 0.2707107)) == reaches
    begin, end = tiny_rays()
    m = tiny_map()
    o = cases.make_oracle(oracle_kind, m, np.zeros(len(m), np.uint32), dist_weight)
    want_st, want_hit = o.beam_status(begin, end)
    counts = [int(np.sum(want_st == s)) for s in range(4)]
    print("kd-tree caster on the tiny map, cell %.4f, %s: oracle counts %s" % (cell, dist_weight, counts))
    assert min(counts) >= 5
    install(eng, dist_weight, 9920, match_dist_min=match_dist_min)
    eng.set_beam_raycast(1)
    try:
        st, hit = eng.beam_status(begin, end)
    finally:
        eng.set_beam_raycast(0)
    np.testing.assert_array_equal(st, want_st)
    np.testing.assert_array_equal(hit, want_hit)


@pytest.mark.parametrize("dist_weight", [None, DW5], ids=str)
def test_cell_scan_likelihood_equals_the_candidate_index(eng, dist_weight):
    """lik_index 0 (the nine-row fetch of nearest_d2) against lik_index 2 on 4 particles x 64 points: the same nearest
    distances, so the same terms, sums and match ratios."""
    rng = np.random.default_rng(20263)
    m = tiny_map()
    scan = (m[rng.integers(0, len(m), 64)] + rng.normal(0, 0.08, (64, 3))).astype(np.float32)
    scan[:8] += np.float32(1.0)   # off the map
    poses = np.zeros((4, 7), np.float32)
    poses[:, 6] = 1.0
    poses[1, :3] = (0.05, -0.03, 0.02)
    poses[2, 3:] = (0.0, 0.0, 0.02, 0.9998)
    poses[3, :3] = (-0.2, 0.1, 0.0)
    install(eng, dist_weight, 9930)
    try:
        eng.set_option("lik_index", 0)
        lik0, ratio0, _ = eng.measure_batch(poses, scan)
        eng.set_option("lik_index", 2)
        lik2, ratio2, _ = eng.measure_batch(poses, scan)
    finally:
        eng.set_option("lik_index", 2)
    assert np.all(ratio2 > 0.1) and len(np.unique(lik2)) == 4
    np.testing.assert_array_equal(lik0, lik2)
    np.testing.assert_array_equal(ratio0, ratio2)
