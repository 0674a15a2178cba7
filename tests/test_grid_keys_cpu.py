"""The keys, geometry and counting sort that the builders of the two map grids share (mcl_3dl_amd/csrc/index_geometry.h),
compiled for the host (tests/cpp/grid_keys_check.cpp) and held bit for bit against a numpy float32 / float64 restatement of
the reference's expressions: RaycastUsingDDA::updatePointCloud / toIndex / getArrayIndex (raycast_using_dda.h:162-190,
205-210, 225-228) for the DDA grid, PointRepresentation::vectorize (one float product per coordinate) for the rescale, and
the cell grid's own definition (floor((s - o) * inv) per axis, origin two cells below the bounds, x fastest).
The program is built a second time with the address and undefined-behaviour sanitizers and run on the same inputs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def jitter(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    return (np.asarray(lo, np.float64) + rng.random((n, 3)) * (np.asarray(hi, np.float64) - np.asarray(lo, np.float64))).astype(F32)


def with_corners(xyz):
    """... plus a point exactly on the minimum and one exactly on the maximum corner"""
    return np.concatenate([xyz, xyz.min(0, keepdims=True), xyz.max(0, keepdims=True)]).astype(F32)


def lattice(step, counts, origin):
    """points on multiples of `step` (exact in float32 for the steps used): the extent is an exact multiple of the edge"""
    g = np.stack(np.meshgrid(*[np.arange(c) for c in counts], indexing="ij"), -1).reshape(-1, 3)
    return (np.asarray(origin, np.float64) + g * step).astype(F32)


def five_four_three():
    """DDA dimensions 5 x 4 x 3 at a grid of 0.25: extents 1.1, 0.8, 0.6 -> 4 + 1, 3 + 1, 2 + 1 (bricks not full)"""
    return with_corners(np.concatenate([jitter(120, 5, (-0.5, 0.25, 1.0), (0.6, 1.05, 1.6)),
                                        np.array([[-0.5, 0.25, 1.0], [0.6, 1.05, 1.6]], F32)]))


NON_FINITE = np.array([[np.nan, 0.0, 0.0], [1.0, np.inf, 2.0], [0.5, 0.5, -np.inf]], F32)

# name -> (points, cell edge, dist_weight or None, dda_grid_size, any)
CASES = {
    "one_point": (np.array([[1.5, -2.25, 0.75]], F32), 0.202, None, 0.1, False),
    "two_identical_points": (np.array([[1.5, -2.25, 0.75]] * 2, F32), 0.202, None, 0.1, False),
    "corners_grid_0.1": (with_corners(jitter(200, 1, (-3, -2, 0), (4, 3, 1.5))), 0.202, None, 0.1, False),
    "corners_grid_0.25": (with_corners(jitter(200, 2, (-3, -2, 0), (4, 3, 1.5))), 0.303, None, 0.25, False),
    "extent_multiple_of_the_edge": (lattice(0.25, (9, 5, 3), (-1.0, 0.5, 0.0)), 0.5, None, 0.25, False),
    "dda_5x4x3": (five_four_three(), 0.202, None, 0.25, False),
    "two_km_out": (with_corners(jitter(200, 3, (2000, -2000, 2000), (2004, -1997, 2001))), 0.202, None, 0.1, False),
    "dist_weight_1_1_5": (with_corners(jitter(200, 4, (-3, -2, 0), (4, 3, 1.5))), 0.202, (1.0, 1.0, 5.0), 0.1, False),
    "non_finite_any": (np.concatenate([jitter(60, 6, (-1, -1, 0), (1, 1, 1)), NON_FINITE,
                                       jitter(60, 7, (-1, -1, 0), (1, 1, 1))]), 0.202, None, 0.1, True),
}


def build(tmp, extra=()):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp / ("grid_keys_check" + ("_san" if extra else "")))
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *extra, "-I",
                    os.path.join(ROOT, "mcl_3dl_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "grid_keys_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("grid_keys")


@pytest.fixture(scope="module")
def exe(workdir):
    return build(workdir)


def rescale(xyz, weight):
    """PointRepresentation::vectorize: one float product per coordinate when a dist_weight is set"""
    return xyz if weight is None else (xyz * np.asarray(weight, F32)).astype(F32)


def run(exe, workdir, name):
    xyz, cell, weight, grid, any_rule = CASES[name]
    src, dst = str(workdir / (name + ".in")), str(workdir / (name + ".out"))
    with open(src, "wb") as f:
        np.array([len(xyz), int(any_rule), int(not any_rule)], np.uint32).tofile(f)
        np.array([cell], F32).tofile(f)
        np.array([F32(grid)], np.float64).tofile(f)      # the engine widens its float option
        np.ascontiguousarray(xyz, F32).tofile(f)
        np.ascontiguousarray(rescale(xyz, weight), F32).tofile(f)
    subprocess.run([exe, src, dst], check=True, timeout=120)
    return np.fromfile(dst, np.uint64)


def counting_sort(key, n_keys):
    start = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_keys))])
    return start, np.argsort(key, kind="stable")


def f32_bits(a):
    return np.asarray(a, F32).view(np.uint32).astype(np.uint64)


def expected(name):
    """The same words from numpy: float32 arithmetic where the reference's is float, float64 where it is double."""
    xyz, cell, weight, grid, any_rule = CASES[name]
    cell, grid = F32(cell), np.float64(F32(grid))
    n = len(xyz)
    s = rescale(xyz, weight)
    fin = np.isfinite(s).all(1)
    assert any_rule or fin.all()
    mn, mx = s[fin].min(0), s[fin].max(0)
    inv = F32(1) / cell
    o = (mn - F32(2) * cell).astype(F32)
    dim = np.floor(((mx - o).astype(F32) * inv).astype(F32)).astype(np.int64) + 3
    c = np.zeros((n, 3), np.int64)
    c[fin] = np.floor(((s[fin] - o).astype(F32) * inv).astype(F32)).astype(np.int64)
    c = np.clip(c, 0, dim - 1)
    key = (c[:, 2] * dim[1] + c[:, 1]) * dim[0] + c[:, 0]
    key[~fin] = 0                                         # cell 0 by decree
    start, order = counting_sort(key, int(np.prod(dim)))
    words = [f32_bits(o), f32_bits([inv]), dim, key, start, order]
    if not any_rule:
        mn, mx = xyz.min(0), xyz.max(0)
        # map_size = (size_t)((max - min) / dda_grid_size) + 1: float difference, double division
        dd = ((mx - mn).astype(F32).astype(np.float64) / grid).astype(np.int64) + 1
        bd = (dd + 3) // 4
        total = int(np.prod(dd))
        # toIndex: (int)((p - min) / dda_grid_size); getArrayIndex: x fastest
        v = ((xyz - mn).astype(F32).astype(np.float64) / grid).astype(np.int64)
        vox = v[:, 0] + v[:, 1] * dd[0] + v[:, 2] * (dd[0] * dd[1])
        assert (v >= 0).all() and (v < dd).all()
        brick = ((v[:, 2] >> 2) * bd[1] + (v[:, 1] >> 2)) * bd[0] + (v[:, 0] >> 2)
        bit = np.uint64(1) << (((v[:, 2] & 3) << 4) | ((v[:, 1] & 3) << 2) | (v[:, 0] & 3)).astype(np.uint64)
        vstart, vorder = counting_sort(vox, total)
        g = np.stack(np.meshgrid(np.arange(dd[2]), np.arange(dd[1]), np.arange(dd[0]), indexing="ij"), -1).reshape(-1, 3)[:, ::-1]
        gb = ((g[:, 2] >> 2) * bd[1] + (g[:, 1] >> 2)) * bd[0] + (g[:, 0] >> 2)
        gm = np.uint64(1) << (((g[:, 2] & 3) << 4) | ((g[:, 1] & 3) << 2) | (g[:, 0] & 3)).astype(np.uint64)
        assert len(np.unique(np.stack([gb.astype(np.uint64), gm], 1), axis=0)) == total     # one bit per voxel
        per_voxel = np.stack([np.arange(total).astype(np.uint64), gb.astype(np.uint64), gm, gb.astype(np.uint64), gm], 1)
        words += [dd, bd, np.array([np.float64(total)]).view(np.uint64), vox, brick, bit, vstart, vorder, per_voxel.reshape(-1)]
    return np.concatenate([np.asarray(w).astype(np.uint64) for w in words]), dim, (None if any_rule else dd)


@pytest.mark.parametrize("name", list(CASES))
def test_shared_keys_equal_the_restated_reference(exe, workdir, name):
    want, _, _ = expected(name)
    np.testing.assert_array_equal(run(exe, workdir, name), want)


def test_the_cases_are_what_their_names_say():
    assert tuple(expected("dda_5x4x3")[2]) == (5, 4, 3)
    _, dim, dd = expected("extent_multiple_of_the_edge")
    xyz, cell, _, grid, _ = CASES["extent_multiple_of_the_edge"]
    ext = xyz.max(0) - xyz.min(0)
    np.testing.assert_array_equal(ext / F32(cell), np.round(ext / F32(cell)))     # whole cells, whole voxels
    np.testing.assert_array_equal(dd, (ext / F32(grid)).astype(np.int64) + 1)     # the maximum corner opens the last voxel
    np.testing.assert_array_equal(dim, (ext / F32(cell)).astype(np.int64) + 5)    # two cells below, the corner's own, two above
    assert np.abs(CASES["two_km_out"][0]).min() >= 1997.0
    fin = np.isfinite(CASES["non_finite_any"][0]).all(1)
    assert np.count_nonzero(~fin) == 3 and fin[0] and fin[-1]
    for name in ("corners_grid_0.1", "corners_grid_0.25", "dda_5x4x3", "two_km_out", "dist_weight_1_1_5"):
        xyz = CASES[name][0]
        assert (xyz == xyz.min(0)).all(1).any() and (xyz == xyz.max(0)).all(1).any()


def wide_geometry(exe, workdir):
    """cell_grid_geometry alone over an extent no grid covers: 1e9 along x at a cell edge of 0.202 is 4.95e9 cells, which no int
    holds — that axis counts as INT_MAX cells (every builder then refuses the grid by its cell count), the others as usual"""
    xyz = np.array([[0.0, 1.0, -1.0], [1.0e9, 2.0, 0.5]], F32)
    cell = F32(0.202)
    src, dst = str(workdir / "wide.in"), str(workdir / "wide.out")
    with open(src, "wb") as f:
        np.array([len(xyz), 2, 0], np.uint32).tofile(f)
        np.array([cell], F32).tofile(f)
        np.array([0.1], np.float64).tofile(f)
        xyz.tofile(f)
        xyz.tofile(f)
    subprocess.run([exe, src, dst], check=True, timeout=120)
    got = np.fromfile(dst, np.uint64)
    inv = F32(1) / cell
    o = (xyz.min(0) - F32(2) * cell).astype(F32)
    c = np.floor(((xyz.max(0) - o).astype(F32) * inv).astype(F32))
    assert c[0] > 2.0 ** 31 and (c[1:] < 100).all()
    dim = [2147483647, int(c[1]) + 3, int(c[2]) + 3]
    np.testing.assert_array_equal(got, np.concatenate([f32_bits(o), f32_bits([inv]), np.array(dim, np.uint64)]))


def test_an_axis_past_the_int_range_counts_as_int_max_cells(exe, workdir):
    wide_geometry(exe, workdir)


def test_sanitized_build_runs_clean_on_the_same_inputs(workdir):
    san = build(workdir, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for name in CASES:
        np.testing.assert_array_equal(run(san, workdir, name), expected(name)[0])
    wide_geometry(san, workdir)
