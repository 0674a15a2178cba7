"""The steps that feed the measurement kernels — VoxelGrid, both clip filters, the sampler's gather, the scan ordering — at every
size class of their kernels (mcl_3dl_amd/csrc/cloud_kernels.h, sort_kernels.h as its real users instantiate it: leaf, Morton and
range keys made inside the sort, points written by its last pass), compared EXACTLY with the plain numpy restatements of
tests/cloud_ref.py (which test_cloud_ref_cpu.py pins against the compiled oracle on the same inputs, tests/cloud_cases.py) and,
for VoxelGrid and the clips, with the reference-backed oracle itself. The installed scans are read back through
scan_download(5 / 6): a ray in the wrong place, or the wrong origin id next to the right point, changes no score but shows here.
No tolerance anywhere: equal arrays."""
import functools

import numpy as np
import pytest

import cloud_cases as cases
import cloud_ref
from mcl_3dl_amd.synthetic import make_scene
from oracle import pyoracle

pytestmark = pytest.mark.gpu

CLIP_NAMES = ("clip_near", "clip_far", "clip_z_min", "clip_z_max")


@pytest.fixture(scope="module")
def ref():
    if not pyoracle.available("ref"):
        pytest.fail("oracle/_ref is not built: run `python -c 'import __graft_entry__ as g; g.build()'` where the "
                    "reference's sources exist (the built library travels with the tree)")
    return pyoracle.Oracle("ref")


@pytest.fixture
def order_on_device(engine):
    """scan_order_device = 1: every scan is ordered on the device; the test switches to 0 (host) itself. Restored afterwards."""
    before = engine.get_option("scan_order_device")
    engine.set_option("scan_order_device", 1)
    try:
        yield engine
    finally:
        engine.set_option("scan_order_device", before)


@functools.lru_cache(maxsize=None)
def vg_want(case_id):
    """the restatement's answer for a VoxelGrid input, computed once and shared"""
    xyz, label, leaf = VG_CASES[case_id]()
    out = cloud_ref.voxel_grid(xyz, label, leaf)
    for a in out:
        a.setflags(write=False)
    return out


VG_CASES = dict(cases.vg_all_cases())


def assert_cloud(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


# ---- VoxelGrid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(VG_CASES))
def test_voxel_grid(engine, ref, case_id):
    """Sizes 2 .. 524 289 (one launch, 1024 / 4096 elements per work-group, rocprim), leaves that run across one or several
    whole work-groups of the centroid kernel, heads on a block's last and first entry, leaf indices of 8 .. 31 bits with the
    non-finite key on a power of two, points on leaf boundaries, far from the origin, either side of the int32 overflow rule,
    and clouds with no or two finite points."""
    xyz, label, leaf = VG_CASES[case_id]()
    want = vg_want(case_id)
    n_full, n_lik, n_beam = engine.scan_begin(xyz, label, leaf=leaf, clip_lik=None, clip_beam=None)
    got = engine.scan_download(0)
    assert (n_full, n_lik, n_beam) == (len(want[0]), 0, 0)
    assert_cloud(got, want)
    assert_cloud(got, ref.voxel_grid(xyz, label, leaf))


def test_voxel_grid_inputs_reach_the_edges_they_are_named_for():
    key = cloud_ref.voxel_sorted_keys(*cases.vg_run("heads_on_1023_and_1024")[::2])
    assert key[1022] != key[1023] != key[1024]                    # heads on sorted entries 1023 and 1024
    key = cloud_ref.voxel_sorted_keys(*cases.vg_run("leaf_5000_in_9000")[::2])
    assert key[1999] != key[2000] and key[2000] == key[6999] != key[7000]
    for cells in cases.VG_KEY_WIDTHS:
        lay = cloud_ref.voxel_layout(*cases.vg_key_width(cells)[::2])
        assert lay["cells"] == cells and not lay["passthrough"] and not lay["finite"].all()
    a = cloud_ref.voxel_layout(*cases.vg_arith("extent_filtered_0.147")[::2])
    b = cloud_ref.voxel_layout(*cases.vg_arith("extent_passthrough_0.14")[::2])
    assert (int(np.prod(a["d"])), a["passthrough"]) == (2022734532, False)
    assert (int(np.prod(b["d"])), b["passthrough"]) == (2336094904, True)
    assert len(vg_want("arith_extent_filtered_0.147")[0]) < 6000 == len(vg_want("arith_extent_passthrough_0.14")[0])
    assert len(vg_want("degenerate_all_non_finite")[0]) == 0 and 1 <= len(vg_want("degenerate_two_finite")[0]) <= 2


def test_voxel_grid_back_to_back_large_and_tiny(engine):
    """524 289 points, then 2, then again: the min / max ticket is left ready and the work arrays grow and are reused."""
    for case_id in ("size_524289", "size_2", "size_524289", "size_2", "size_65537"):
        xyz, label, leaf = VG_CASES[case_id]()
        assert engine.scan_begin(xyz, label, leaf=leaf, clip_lik=None, clip_beam=None)[0] == len(vg_want(case_id)[0])
        assert_cloud(engine.scan_download(0), vg_want(case_id))


OTHER_PRODUCERS = ["size_2049", "size_65537", "size_524289", "run_leaf_5000_in_9000", "cells_%d" % 2**24]


@pytest.mark.parametrize("case_id", OTHER_PRODUCERS)
def test_voxel_grid_from_the_wire_format(engine, case_id):
    """the min / max of cloud_decode_minmax_kernel in front of the same filter"""
    xyz, label, leaf = VG_CASES[case_id]()
    buf = cases.pointcloud2_bytes(xyz, label)
    n_full, _, _ = engine.scan_begin_pointcloud2(buf, len(xyz), 32, 4, 8, 12, off_label=24, label_override=0xFFFFFFFF, leaf=leaf,
                                                 clip_lik=None, clip_beam=None)
    assert n_full == len(vg_want(case_id)[0])
    assert_cloud(engine.scan_download(0), vg_want(case_id))


@pytest.mark.parametrize("case_id", OTHER_PRODUCERS)
def test_voxel_grid_of_the_map(engine, case_id):
    """cloud_minmax_kernel + voxel_grid_now (leaf count read back at once) through set_map_downsampled"""
    xyz, label, leaf = VG_CASES[case_id]()
    assert engine.set_map_downsampled(xyz, label, leaf=leaf, stamp=9100) == len(vg_want(case_id)[0])
    assert_cloud(engine.map_download(), vg_want(case_id))


# ---- clips ----------------------------------------------------------------------------------------------------------------
def check_clips(engine, ref, xyz, label, leaf, lik4, beam4):
    """both clipped clouds against the restatement and the oracle, applied to the cloud the clip kernels were given"""
    n_full, n_lik, n_beam = engine.scan_begin(xyz, label, leaf=leaf, clip_lik=lik4, clip_beam=beam4)
    full = engine.scan_download(0)
    assert n_full == len(full[0])
    ref.set_likelihood_params(pyoracle.LikelihoodParams(**dict(zip(CLIP_NAMES, lik4))))
    ref.set_beam_params(pyoracle.BeamParams(**dict(zip(CLIP_NAMES, beam4))))
    out = []
    for model, which, c4, cnt in ((0, 1, lik4, n_lik), (1, 2, beam4, n_beam)):
        got = engine.scan_download(which)
        assert cnt == len(got[0])
        assert_cloud(got, cloud_ref.clip(full[0], *c4, label=full[1]))
        assert_cloud(got, ref.clip(model, full[0], full[1])[:2])
        out.append(got)
    return full, out


@pytest.mark.parametrize("filtered", [True, False], ids=["count_on_device", "count_from_host"])
@pytest.mark.parametrize("pattern", list(cases.CLIP_PATTERNS))
@pytest.mark.parametrize("n", cases.CLIP_SIZES)
def test_clips_at_block_edges(engine, ref, n, pattern, filtered):
    """Clouds of 1023 .. 4097 points in front of the two clip kernels, with the VoxelGrid in front (the count stays on the
    device) and without: all kept, none kept by one model while the other keeps every other point, only the last point kept."""
    xyz, label = cases.clip_lattice(n)
    lik4, beam4, keep_lik, keep_beam = cases.CLIP_PATTERNS[pattern]
    full, (got_lik, got_beam) = check_clips(engine, ref, xyz, label, cases.CLIP_LEAF if filtered else None, lik4, beam4)
    assert_cloud(full, (xyz, label))       # (the lattice comes back from the filter point for point)
    for got, kind in ((got_lik, keep_lik), (got_beam, keep_beam)):
        m = cases.clip_pattern_mask(kind, n)
        assert_cloud(got, (xyz[m], label[m]))


@pytest.mark.parametrize("filtered", [True, False], ids=["count_on_device", "count_from_host"])
def test_clips_keep_points_on_their_thresholds(engine, ref, filtered):
    """r^2 exactly far^2 and near^2, z exactly z_min and z_max: kept (the reference's comparisons are strict)"""
    xyz, label, on = cases.clip_threshold_cloud(False)
    _, got = check_clips(engine, ref, xyz, label, (0.01, 0.01, 0.01) if filtered else None, cases.CLIP_EDGE_LIK,
                         cases.CLIP_EDGE_BEAM)
    for (kept, _), mine in zip(got, (on[:7], on[7:])):
        for p in mine:
            assert (kept == p).all(1).any(), p
        assert 0 < len(kept) < len(xyz)


def test_clips_keep_nan_points(engine, ref):
    xyz, label, _ = cases.clip_threshold_cloud(True)
    _, got = check_clips(engine, ref, xyz, label, None, cases.CLIP_EDGE_LIK, cases.CLIP_EDGE_BEAM)
    for kept, _ in got:
        assert np.count_nonzero(np.isnan(kept).any(1)) == 4


# ---- likelihood scan order ------------------------------------------------------------------------------------------------
def check_installed_lik(engine, scan, order):
    np.testing.assert_array_equal(engine.scan_order(len(scan)), order)
    got_xyz, got_w = engine.scan_download(5)
    np.testing.assert_array_equal(got_xyz, scan[order])
    assert not got_w.any()


@pytest.mark.parametrize("n", cases.LIK_SIZES)
def test_likelihood_scan_order(order_on_device, n):
    """Morton keys made inside the sort, the scan written by its last pass: one work-group, 1 and 4 rounds per work-group,
    rocprim + apply kernel above 524 288; NaN / +-inf points, clamped cells. The same through the host ordering up to 65 537."""
    engine = order_on_device
    scan = cases.lik_scan(n)
    order = cloud_ref.morton_order(scan)
    engine.upload_scan(scan)
    check_installed_lik(engine, scan, order)
    if n <= cases.LIK_HOST_MAX:
        engine.set_option("scan_order_device", 0)
        engine.upload_scan(scan)
        check_installed_lik(engine, scan, order)


# ---- beam scan order ------------------------------------------------------------------------------------------------------
def check_installed_beam(engine, xyz, og, order):
    got_xyz, got_og = engine.scan_download(6)
    np.testing.assert_array_equal(got_xyz, xyz[order])
    np.testing.assert_array_equal(got_og, og[order])


@pytest.mark.parametrize("n", cases.BEAM_SIZES)
def test_beam_scan_order(order_on_device, n):
    """Range keys made inside the sort, four passes: rays in ascending range from their own origin, ties in input order, every
    origin id still next to its point — on both paths."""
    engine = order_on_device
    xyz, og, origins = cases.beam_scan(n)
    lik = cases.lik_scan(63)
    order = cloud_ref.range_order(xyz, og, origins)
    for where in (1, 0):
        engine.set_option("scan_order_device", where)
        engine.upload_scan(lik, xyz, og, origins)
        check_installed_beam(engine, xyz, og, order)
        check_installed_lik(engine, lik, cloud_ref.morton_order(lik))


@pytest.mark.parametrize("n_b", [2049, 4097])
def test_beam_scores_do_not_depend_on_where_the_scan_was_ordered(order_on_device, oracle_kind, n_b):
    engine = order_on_device
    sc = make_scene(n=91, n_p=4, n_s=200, n_b=n_b, seed=21)
    origins = np.concatenate([sc.origins, sc.origins + np.float32(0.125), sc.origins - np.float32(0.0625)])
    beam = sc.scan_beam.copy()
    og = (np.arange(n_b) % 3).astype(np.uint32)
    beam[100:140], og[100:140] = beam[:40], og[:40]                  # exact duplicates
    assert np.isfinite(beam).all()
    engine.set_map(sc.map_xyz, sc.map_label, stamp=9200)
    engine.set_likelihood_params()
    engine.set_beam_params(num_points=n_b)
    order = cloud_ref.range_order(beam, og, origins)
    out = {}
    for where in (1, 0):
        engine.set_option("scan_order_device", where)
        out[where] = engine.measure_batch(sc.poses, sc.scan_lik, beam, og, origins)
        check_installed_beam(engine, beam, og, order)                # (installed by the update call itself)
        check_installed_lik(engine, sc.scan_lik, cloud_ref.morton_order(sc.scan_lik))
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a, b)
    o = pyoracle.Oracle(oracle_kind)
    o.set_map(sc.map_xyz, sc.map_label)
    o.set_beam_params(pyoracle.BeamParams(num_points=n_b))
    want, _ = o.beam_measure(sc.poses, beam, og, origins)
    np.testing.assert_array_equal(out[1][2], want)
    assert (want > 0).all() and (want < 1).any()      # some rays are penalised: the score is not trivially 1


# ---- gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2048, 2049, 70000])
def test_gather_and_order_of_a_drawn_sample(engine, m):
    """scan_finish: the drawn points (repeated indices included) in the caller's order, then installed in the engine's order"""
    xyz, label, _ = cases.vg_size(65537)
    rng = np.random.default_rng(m)
    _, n_lik, n_beam = engine.scan_begin(xyz, label, leaf=None, clip_lik=(0.5, 10.0, -2.0, 2.0), clip_beam=(0.5, 4.0, -1.0, 1.0))
    clipped = engine.scan_download(1)
    clipped_beam = engine.scan_download(2)
    assert_cloud(clipped, cloud_ref.clip(xyz, 0.5, 10.0, -2.0, 2.0, label=label))
    assert n_lik == len(clipped[0]) > 30000 and n_beam == len(clipped_beam[0]) > 10000
    idx = rng.integers(0, n_lik, m).astype(np.uint32)
    idx[m // 2:m // 2 + 300] = idx[:300]
    idx_b = rng.integers(0, n_beam, 2049).astype(np.uint32)
    keep = np.isfinite(clipped_beam[0][idx_b]).all(1)                # (finite rays only)
    idx_b = idx_b[keep]
    origins = np.concatenate([cases.BEAM_ORIGINS, np.array([[0.25, 0.25, 0.25]], np.float32)])   # labels 0 .. 3 name them
    engine.scan_finish(idx, idx_b, origins=origins)
    sample = clipped[0][idx], clipped[1][idx]
    assert_cloud(engine.scan_download(3), sample)
    check_installed_lik(engine, sample[0], cloud_ref.morton_order(sample[0]))
    sample_b = clipped_beam[0][idx_b], clipped_beam[1][idx_b]        # label = the accumulated cloud's index = origin id
    assert_cloud(engine.scan_download(4), sample_b)
    check_installed_beam(engine, sample_b[0], sample_b[1], cloud_ref.range_order(sample_b[0], sample_b[1], origins))


def test_installed_scans_need_no_prepared_scan(engine):
    """which = 5 / 6 follow the installed scan (has_scan), not scan_begin's state"""
    from mcl_3dl_amd import capi
    xyz, og, origins = cases.beam_scan(2047)
    engine.set_map_downsampled(*cases.vg_size(63)[:2], leaf=cases.LEAF_BOX, stamp=9300)   # (borrows and drops the prepared scan)
    with pytest.raises(capi.EngineError, match="no prepared scan"):
        engine.scan_download(0)
    engine.upload_scan(cases.lik_scan(64), xyz, og, origins)
    assert len(engine.scan_download(5)[0]) == 64 and len(engine.scan_download(6)[0]) == 2047
    with pytest.raises(capi.EngineError, match="0..6"):
        engine.scan_download(7)
