"""The numpy restatements of tests/cloud_ref.py against what already exists on the CPU, over the very inputs of
test_gpu_cloud_edges.py (tests/cloud_cases.py), so that the GPU tests do not rest on an unchecked reference:
  * voxel_grid and clip equal the compiled reference-backed oracle (pcl::VoxelGrid restated in oracle/shims, the reference's own
    filter() lambdas), array for array;
  * morton_order equals mcl3dl_hip_scan_order_host (host library only), range_order a plain lexicographic sort;
  * the Morton keys and the range keys equal, bit for bit, those of mcl_3dl_amd/csrc/cloud_keys.h compiled for the host
    (tests/cpp/scan_keys_check.cpp): the one statement the sort kernels and the host ordering share."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_cases as cases
import cloud_ref
from mcl_3dl_amd import capi
from oracle import pyoracle


@pytest.fixture(scope="module")
def ref():
    if not pyoracle.available("ref"):
        pytest.fail("oracle/_ref is not built: run `python -c 'import __graft_entry__ as g; g.build()'` where the "
                    "reference's sources exist (the built library travels with the tree)")
    return pyoracle.Oracle("ref")


def set_clips(ref, lik4, beam4):
    names = ("clip_near", "clip_far", "clip_z_min", "clip_z_max")
    ref.set_likelihood_params(pyoracle.LikelihoodParams(**dict(zip(names, lik4))))
    ref.set_beam_params(pyoracle.BeamParams(**dict(zip(names, beam4))))


@pytest.mark.parametrize("case", [c[1] for c in cases.vg_all_cases()], ids=[c[0] for c in cases.vg_all_cases()])
def test_voxel_grid_equals_the_oracle(ref, case):
    xyz, label, leaf = case()
    got_xyz, got_label = cloud_ref.voxel_grid(xyz, label, leaf)
    want_xyz, want_label = ref.voxel_grid(xyz, label, leaf)
    np.testing.assert_array_equal(got_xyz, want_xyz)
    np.testing.assert_array_equal(got_label, want_label)


def test_the_voxel_grid_inputs_are_what_their_names_say():
    for cells in cases.VG_KEY_WIDTHS:
        xyz, _, leaf = cases.vg_key_width(cells)
        lay = cloud_ref.voxel_layout(xyz, leaf)
        assert lay["cells"] == cells and not lay["passthrough"] and np.count_nonzero(~lay["finite"]) == 2
    a = cloud_ref.voxel_layout(*cases.vg_arith("extent_filtered_0.147")[::2])
    b = cloud_ref.voxel_layout(*cases.vg_arith("extent_passthrough_0.14")[::2])
    assert int(np.prod(a["d"])) == 2022734532 and not a["passthrough"]
    assert int(np.prod(b["d"])) == 2336094904 and b["passthrough"]
    np.testing.assert_array_equal(cases.vg_arith("extent_filtered_0.147")[0], cases.vg_arith("extent_passthrough_0.14")[0])
    key = cloud_ref.voxel_sorted_keys(*cases.vg_run("heads_on_1023_and_1024")[::2])
    assert key[1022] != key[1023] != key[1024]
    key = cloud_ref.voxel_sorted_keys(*cases.vg_run("leaf_5000_in_9000")[::2])
    assert key[1999] != key[2000] and key[2000] == key[6999] != key[7000]
    key = cloud_ref.voxel_sorted_keys(*cases.vg_run("leaf_600_voted")[::2])
    assert key[799] != key[800] and key[800] == key[1399] != key[1400]
    assert len(np.unique(cloud_ref.voxel_sorted_keys(*cases.vg_run("leaf_3000")[::2]))) == 1
    assert len(np.unique(cloud_ref.voxel_sorted_keys(*cases.vg_run("own_leaf_4000")[::2]))) == 4000
    assert cloud_ref.voxel_layout(*cases.vg_degenerate("all_non_finite")[::2]) is None
    assert np.count_nonzero(cloud_ref.voxel_layout(*cases.vg_degenerate("two_finite")[::2])["finite"]) == 2


def check_clip(ref, xyz, label, lik4, beam4):
    set_clips(ref, lik4, beam4)
    for model, c4 in ((0, lik4), (1, beam4)):
        got_xyz, got_label = cloud_ref.clip(xyz, *c4, label=label)
        want_xyz, want_label, _ = ref.clip(model, xyz, label)
        np.testing.assert_array_equal(got_xyz, want_xyz)
        np.testing.assert_array_equal(got_label, want_label)


@pytest.mark.parametrize("n", cases.CLIP_SIZES)
@pytest.mark.parametrize("pattern", list(cases.CLIP_PATTERNS))
def test_clip_equals_the_oracle_on_the_lattice(ref, n, pattern):
    xyz, label = cases.clip_lattice(n)
    lik4, beam4, keep_lik, keep_beam = cases.CLIP_PATTERNS[pattern]
    check_clip(ref, xyz, label, lik4, beam4)
    # the lattice does what its name says: the VoxelGrid hands it back as it is, the clips keep the named indices
    vg_xyz, vg_label = cloud_ref.voxel_grid(xyz, label, cases.CLIP_LEAF)
    np.testing.assert_array_equal(vg_xyz, xyz)
    np.testing.assert_array_equal(vg_label, label)
    for c4, kind in ((lik4, keep_lik), (beam4, keep_beam)):
        np.testing.assert_array_equal(cloud_ref.clip(xyz, *c4)[0], xyz[cases.clip_pattern_mask(kind, n)])


@pytest.mark.parametrize("with_nan", [False, True])
def test_clip_equals_the_oracle_on_the_thresholds(ref, with_nan):
    xyz, label, on = cases.clip_threshold_cloud(with_nan)
    check_clip(ref, xyz, label, cases.CLIP_EDGE_LIK, cases.CLIP_EDGE_BEAM)
    # every point ON a threshold of a model is kept by that model (7 per model), and so is every point with a NaN
    for c4, mine in ((cases.CLIP_EDGE_LIK, on[:7]), (cases.CLIP_EDGE_BEAM, on[7:])):
        kept = cloud_ref.clip(xyz, *c4)[0]
        for p in mine:
            assert (kept == p).all(1).any(), p
        assert np.count_nonzero(np.isnan(kept).any(1)) == (4 if with_nan else 0)
    if not with_nan:
        vg = cloud_ref.voxel_grid(xyz, label, (0.01, 0.01, 0.01))[0]      # (the GPU test puts this filter in front)
        for p in on:
            assert (vg == p).all(1).any(), p


@pytest.mark.parametrize("n", cases.LIK_SIZES)
def test_morton_order_equals_the_host_ordering(n):
    scan = cases.lik_scan(n)
    np.testing.assert_array_equal(cloud_ref.morton_order(scan), capi.scan_order_host(scan))
    if n >= 63:
        assert len(np.unique(cloud_ref.morton_keys(scan))) < 3 * n // 4      # many points per cell
    if n == cases.LIK_WIDE:
        assert np.ptp(scan[:, 0]) > 256.0


@pytest.mark.parametrize("n", cases.BEAM_SIZES)
def test_range_order_is_the_lexicographic_order_of_range_and_index(n):
    xyz, og, origins = cases.beam_scan(n)
    assert np.isfinite(xyz).all()
    d = xyz.astype(np.float64) - origins.astype(np.float64)[og]       # exact: the points sit on a 1/64 m lattice
    r2 = (d * d).sum(1)
    want = np.lexsort((np.arange(n), r2))
    np.testing.assert_array_equal(cloud_ref.range_order(xyz, og, origins), want)
    # equal ranges from different origins and exact duplicates are both there
    first = np.argsort(r2, kind="stable")
    same = r2[first][1:] == r2[first][:-1]
    assert np.count_nonzero(same & (og[first][1:] != og[first][:-1])) > n // 16
    assert n - len(np.unique(np.c_[xyz, og], axis=0)) >= n // 8 - 1


# ---- the keys of cloud_keys.h, compiled for the host ----------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scan_keys(tmp_path_factory):
    """keys(lik xyz, beam xyz, origin ids, origins) -> (dropped bits, Morton keys, range keys' bits) from scan_keys_check."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("scan_keys")
    exe = str(tmp / "scan_keys_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "mcl_3dl_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "scan_keys_check.cpp")], check=True)

    def keys(lik=None, beam=None, og=None, origins=None):
        lik = np.zeros((0, 3), np.float32) if lik is None else np.ascontiguousarray(lik, np.float32).reshape(-1, 3)
        beam = np.zeros((0, 3), np.float32) if beam is None else np.ascontiguousarray(beam, np.float32).reshape(-1, 3)
        og = np.zeros(len(beam), np.uint32) if og is None else np.ascontiguousarray(og, np.uint32)
        origins = np.zeros((0, 3), np.float32) if origins is None else np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as f:
            np.array([len(lik), len(beam), len(origins)], np.uint32).tofile(f)
            for a in (lik, beam, og, origins):
                a.tofile(f)
        subprocess.run([exe, src, dst], check=True, timeout=120)
        out = np.fromfile(dst, np.uint32)
        assert len(out) == 1 + len(lik) + len(beam)
        return int(out[0]), out[1:1 + len(lik)], out[1 + len(lik):]
    return keys


def range_key_bits(xyz, og, origins):
    """The float32 expression of cloud_ref.range_order, viewed as uint32."""
    xyz, origins = np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(origins, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = xyz - origins[np.asarray(og, np.int64)]
        key = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return key.view(np.uint32)


ALL_NON_FINITE_3 = np.array([[np.nan, 0.0, 0.0], [1.0, np.inf, 2.0], [np.nan, -np.inf, np.inf]], np.float32)


@pytest.mark.parametrize("n", cases.LIK_SIZES + ["all_non_finite_3"])
def test_morton_keys_equal_the_header_compiled_for_the_host(scan_keys, n):
    scan = ALL_NON_FINITE_3 if n == "all_non_finite_3" else cases.lik_scan(n)
    drop, got, _ = scan_keys(lik=scan)
    want = cloud_ref.morton_keys(scan)
    np.testing.assert_array_equal(got, want)
    fin = cloud_ref.finite_rows(scan)
    if fin.any():
        with np.errstate(over="ignore"):
            cells = int(cloud_ref._cell((scan[fin].max(0) - scan[fin].min(0)) * np.float32(4)).max())
        assert drop == max(0, 3 * cells.bit_length() - cloud_ref.MORTON_BITS)
    else:
        assert drop == 0                            # the corners stay at +-FLT_MAX: an extent of -inf, no cell, no bit to drop
    if n == cases.LIK_WIDE:
        assert drop == 30 - cloud_ref.MORTON_BITS   # cells clamp at 1023: all ten bits per axis in use
    if n in cases.LIK_NONFINITE:
        assert np.count_nonzero(~fin) == 4


@pytest.mark.parametrize("n", cases.BEAM_SIZES)
def test_range_keys_equal_the_header_compiled_for_the_host(scan_keys, n):
    xyz, og, origins = cases.beam_scan(n)
    _, _, got = scan_keys(beam=xyz, og=og, origins=origins)
    np.testing.assert_array_equal(got, range_key_bits(xyz, og, origins))
    # sorting the bits as unsigned integers is sorting the ranges
    np.testing.assert_array_equal(np.argsort(got, kind="stable"), cloud_ref.range_order(xyz, og, origins))


def test_range_keys_of_non_finite_points_sort_last(scan_keys):
    origins = np.array([[0.5, -1.0, 0.25]], np.float32)
    xyz = np.array([[np.nan, 1.0, 2.0], [np.inf, 1.0, 2.0], [3.0, -np.inf, 2.0], [3.0, 1.0, 2.0]], np.float32)
    _, _, got = scan_keys(beam=xyz, og=np.zeros(4, np.uint32), origins=origins)
    np.testing.assert_array_equal(got, range_key_bits(xyz, np.zeros(4, np.int64), origins))
    assert got[0] > 0x7f800000                      # NaN: above +inf's bits, behind every other range
    assert got[1] == 0x7f800000 and got[2] == 0x7f800000
    assert got[3] < 0x7f800000
