"""Scan intake ("Scan intake"): an update's scans reach a context ordered on the host and pushed, raw and ordered by
the chip-wide sort, taken over and ordered by one work-group per scan (stage_kernels.h), taken over by stage_pack_kernel and
ordered by the chip-wide sort, or through a device group's ranks. Every route makes its keys with the functions of
mcl_3dl_amd/csrc/cloud_keys.h and sorts them stably, so every route installs the same bytes: the permutation of
cloud_ref.morton_order, the beam scan in cloud_ref.range_order. The sizes sit where a route changes."""
import ctypes as C

import numpy as np
import pytest

import cloud_ref
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
N_P = 16
ORIGINS = np.array([[0.0, 0.0, 0.5], [0.3, -0.2, 0.6], [-0.4, 0.1, 0.4]], np.float32)
# (n_s, n_b): small scans | ST_MAX_POINTS = 2048, one work-group against pack + chip-wide sort | scan_order_device = 4096 on
# n_s + n_b, at its default | one scan empty
PAIRS = [(1, 1), (96, 3), (2048, 2048), (2049, 40), (4090, 5), (4090, 6), (0, 48), (300, 0)]


@pytest.fixture(scope="module")
def scene():
    return make_scene(n=91, n_p=N_P, n_s=4090, n_b=2048, seed=515)


def configure(engine, sc, n_b, stamp, dist_weight=(1.0, 1.0, 5.0)):
    engine.set_map(sc.map_xyz, sc.map_label, stamp=stamp, dist_weight=dist_weight)
    engine.set_likelihood_params()
    engine.set_beam_params(num_points=max(n_b, 1))


def scans(sc, n_s, n_b):
    """(lik, beam, origin ids): the likelihood scan with one NaN point and exact duplicates where its size has room for them."""
    lik = sc.scan_lik[:n_s].copy()
    if n_s >= 16:
        lik[n_s // 2:n_s // 2 + n_s // 8] = lik[:n_s // 8]
        lik[5, 1] = np.nan
    return np.ascontiguousarray(lik), np.ascontiguousarray(sc.scan_beam[:n_b]), (np.arange(n_b) % 3).astype(np.uint32)


def installed(eng, n_s):
    """The installed scans of a context as bytes: (likelihood xyz, beam xyz, beam origin ids, permutation)."""
    lik, lik_lab = eng.scan_download(5)
    beam, beam_lab = eng.scan_download(6)
    assert len(lik) == n_s and not lik_lab.any()
    return lik.view(np.uint32), beam.view(np.uint32), beam_lab, eng.scan_order(n_s)


def group_of_two(sc, n_b, stamp):
    g = capi.Group([0, 0], collective="host")
    configure(g, sc, n_b, stamp)
    return g


@pytest.mark.parametrize("n_s,n_b", PAIRS)
def test_every_route_installs_the_same_bytes(engine, scene, n_s, n_b):
    sc = scene
    lik, beam, og = scans(sc, n_s, n_b)
    w0 = np.full(N_P, 1.0 / N_P, np.float32)
    configure(engine, sc, n_b, stamp=9500 + n_s + n_b)
    d = engine.get_option("scan_order_device")
    got = {}
    try:
        for where in (0, 1):                       # 0 = ordered on the host, 1 = on the device, whatever the size
            engine.set_option("scan_order_device", where)
            engine.upload_scan(lik, beam, og, ORIGINS)
            got["upload_scan, scan_order_device=%d" % where] = installed(engine, n_s)
        engine.set_option("scan_order_device", d)
        engine.upload_scan(lik, beam, og, ORIGINS)
        got["upload_scan"] = installed(engine, n_s)
        for stage, zero_copy in ((1, 1), (1, 0), (0, 0)):
            engine.set_option("update_stage", stage)
            engine.set_option("update_zero_copy", zero_copy)
            engine.measure_update(sc.poses, w0, lik, beam, og, ORIGINS)
            got["measure_update, update_stage=%d, update_zero_copy=%d" % (stage, zero_copy)] = installed(engine, n_s)
        engine.set_option("update_stage", 1)
        engine.set_option("update_zero_copy", 1)
        engine.measure_batch(sc.poses, lik, beam, og, ORIGINS)
        got["measure_batch"] = installed(engine, n_s)
    finally:
        engine.set_option("scan_order_device", d)
        engine.set_option("update_stage", 1)
        engine.set_option("update_zero_copy", 1)
    g = group_of_two(sc, n_b, stamp=9600 + n_s + n_b)
    try:
        g.measure_update(sc.poses, w0, lik, beam, og, ORIGINS)
        for r in range(2):
            got["group measure_update, rank %d" % r] = installed(g.context(r), n_s)
        g.measure_batch(sc.poses, lik, beam, og, ORIGINS)
        for r in range(2):
            got["group measure_batch, rank %d" % r] = installed(g.context(r), n_s)
    finally:
        g.close()
    perm = cloud_ref.morton_order(lik)
    order = cloud_ref.range_order(beam, og, ORIGINS)
    want = (lik[perm].view(np.uint32), beam[order].view(np.uint32), og[order], perm)
    for route, have in got.items():
        for name, a, b in zip(("likelihood scan", "beam scan", "beam origin ids", "permutation"), have, want):
            np.testing.assert_array_equal(a, b, err_msg="%s: %s" % (route, name))


def test_non_finite_beam_ranges_sort_last_on_host_and_device(engine, scene):
    """The host orders the beam scan by the range key's BITS, as the device does: a NaN range (bits above +inf's) goes behind
    every other, an infinite one in front of it. (upload_scan only: the beam model is not run on such points.)"""
    sc = scene
    _, beam, og = scans(sc, 0, 300)
    beam[17, 0] = np.nan
    beam[200, 2] = np.inf
    configure(engine, sc, 300, stamp=9701)
    d = engine.get_option("scan_order_device")
    got = []
    try:
        for where in (0, 1):
            engine.set_option("scan_order_device", where)
            engine.upload_scan(None, beam, og, ORIGINS)
            xyz, lab = engine.scan_download(6)
            got.append((xyz.view(np.uint32), lab))
    finally:
        engine.set_option("scan_order_device", d)
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], got[1][1])
    finite = np.delete(np.arange(300), [17, 200])
    order = np.r_[finite[cloud_ref.range_order(beam[finite], og[finite], ORIGINS)], 200, 17]
    np.testing.assert_array_equal(got[0][0], beam[order].view(np.uint32))
    np.testing.assert_array_equal(got[0][1], og[order])


UPDATE_ROUTES = [("upload_scan", "scan_order_device", 0), ("upload_scan", "scan_order_device", 1),
                 ("measure_update", "update_stage", 1), ("measure_update", "update_stage", 0)]


@pytest.mark.parametrize("call,option,value", UPDATE_ROUTES, ids=["%s-%s=%d" % r for r in UPDATE_ROUTES])
def test_argument_errors_keep_their_wording(engine, scene, call, option, value):
    sc = scene
    lik, beam, og = scans(sc, 96, 8)
    w0 = np.full(N_P, 1.0 / N_P, np.float32)
    configure(engine, sc, 8, stamp=9702)

    def run(lik, beam, og, origins):
        if call == "upload_scan":
            engine.upload_scan(lik, beam, og, origins)
        else:
            engine.measure_update(sc.poses, w0, lik, beam, og, origins)

    def run_oversized():
        # a point count no array can have: refused by the check, before anything is read
        one, n = capi._ptr(lik), 2**31
        if call == "upload_scan":
            engine._check(engine.lib.mcl3dl_hip_upload_scan(engine.h, one, n, None, None, 0, None, 0))
        else:
            st = [C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)]
            w = w0.copy()
            engine._check(engine.lib.mcl3dl_hip_measure_update(
                engine.h, capi._ptr(sc.poses), None, capi._ptr(w), N_P, one, n, None, None, 0, None, 0, None, None, None,
                *[C.byref(s) for s in st]))

    before = engine.get_option(option)
    try:
        engine.set_option(option, value)
        with pytest.raises(capi.EngineError, match="null scan array"):
            run(lik, beam, og, np.zeros((0, 3), np.float32))
        bad = og.copy()
        bad[5] = 3
        with pytest.raises(capi.EngineError, match="beam point 5 names origin 3 but only 3 origins were given"):
            run(lik, beam, bad, ORIGINS)
        with pytest.raises(capi.EngineError, match="scan too large"):
            run_oversized()
        run(lik, beam, og, ORIGINS)                # (and the context still works)
    finally:
        engine.set_option(option, before)
