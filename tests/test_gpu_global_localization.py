"""Global localisation on the GPU (mcl_3dl_amd/csrc/api_global_loc.inl, global_loc_kernels.h) against cbGlobalLocalization
(src/mcl_3dl.cpp:1039-1099) composed from the reference-backed CPU oracle the way the reference composes its own parts
(tests/global_loc_ref.py). Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import global_loc_ref as glr
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import cube_map, make_scene, quat_from_rpy, quat_to_matrix
from oracle import pyoracle

pytestmark = pytest.mark.gpu
F = np.float32
CONFIGS = [([0], None, 1), ([0], None, 0), ([0, 0, 0], "host", 1)]
IDS = ["n1-direct", "n1-rccl", "n3-host"]
DW = (1.0, 1.0, 5.0)
IMU = quat_from_rpy([0.03, -0.05, 0.4]).astype(F)  # a tilted unit quaternion
# NormalLikelihood(sigma = 1)(0), the node's odometry factor for a zero error vector: the oracle's update applies it
ODOM0 = F(1.0 / np.sqrt(2.0 * np.pi))
# (name, cube n, jitter, dist_weight, grid, centroids, kept, removed): the counts were measured with the oracle alone
POINT_CASES = [
    ("a-lattice", 91, 0.0, (1.0, 1.0, 1.0), 0.3, 5674, 1807, 3867),
    ("b-jitter", 91, 0.04, DW, 0.3, 5755, 2246, 3509),
    ("c-grid05", 91, 0.04, DW, 0.5, 2163, 877, 1286),
    ("d-n201", 201, 0.04, DW, 0.3, 26936, 9443, 17493),
]


def scene_map(n, jitter):
    return make_scene(n=n, n_p=8, n_s=64, n_b=0, seed=31, map_jitter=jitter).map_xyz


def group(cfg):
    devices, collective, direct = cfg
    g = capi.Group(devices, collective=collective)
    g.set_option("direct_single", direct)
    return g


def configure(obj, map_xyz, dist_weight=DW, stamp=8100):
    obj.set_map(map_xyz, None, stamp=stamp, dist_weight=dist_weight)
    obj.set_likelihood_params()
    obj.set_beam_params()


def group_map_update(g, xyz, leaf=(0.2, 0.2, 0.2), stamp=8200):
    """mcl3dl_hip_map_update on every context of the group (the map is replicated)."""
    pts = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    lf = np.asarray(leaf, F)
    g.lib.mcl3dl_hip_group_context.restype = C.c_void_p
    for r in range(g.n):
        ctx = C.c_void_p(g.lib.mcl3dl_hip_group_context(g.h, r))
        n = C.c_size_t(0)
        rc = g.lib.mcl3dl_hip_map_update(ctx, capi._ptr(pts), None, len(pts), capi._ptr(lf), int(stamp), C.byref(n), None)
        assert rc == 0, g.lib.mcl3dl_hip_last_error(ctx).decode()


@pytest.fixture(scope="module")
def map_b():
    return scene_map(91, 0.04)


@pytest.fixture(scope="module")
def points_b(map_b):
    return glr.standable_points(map_b, 0.3, DW)[0]


@pytest.mark.parametrize("case", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_points_are_the_oracle_compositions(case):
    _, n, jitter, dw, grid, n_centroids, n_kept, n_removed = case
    m = scene_map(n, jitter)
    want, centroids, sq, found = glr.standable_points(m, grid, dw)
    near = np.abs(sq[found > 0] - F(grid * grid)).min()
    print("%s: map %d, centroids %d, kept %d, removed %d, closest decision |d2 - r2| = %.3g"
          % (case[0], len(m), len(centroids), len(want), len(centroids) - len(want), near))
    # the yardstick itself: a filter that keeps or drops everything cannot pass
    assert (len(centroids), len(want), len(centroids) - len(want)) == (n_centroids, n_kept, n_removed)
    e = capi.Engine(0)
    try:
        e.set_map(m, None, stamp=8000, dist_weight=dw)
        got, got_centroids = e.global_localization_points(grid)
        assert got_centroids == n_centroids
        np.testing.assert_array_equal(got, want)
        # and again: the call leaves nothing behind that changes its own result
        got2, _ = e.global_localization_points(grid)
        np.testing.assert_array_equal(got2, want)
    finally:
        e.close()


@pytest.mark.parametrize("div_yaw", [12, 5])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_seeded_particles_are_resident(cfg, div_yaw, map_b, points_b):
    want_s, want_w = glr.particles(points_b, div_yaw, IMU)
    if div_yaw == 5:
        assert len(want_s) % 3 != 0  # shards of unequal size (12 yaws always split evenly over three ranks)
    g = group(cfg)
    try:
        configure(g, map_b)
        # something else is resident, with odometry noise, and a resampling is under way: all of it is replaced
        g.upload_state(np.tile(np.arange(13, dtype=F), (77, 1)))
        g.set_odom_noise(np.ones((77, 4), F))
        g.resample_begin(0)
        n_points, n_particles = g.global_localization(0.3, div_yaw, IMU)
        assert (n_points, n_particles) == (len(points_b), len(points_b) * div_yaw)
        assert g.resident() == n_particles
        got_s, got_w = g.download_state()
        np.testing.assert_array_equal(got_s.view(np.uint32), want_s.view(np.uint32))
        np.testing.assert_array_equal(got_w, want_w)
        assert got_w[0] == F(1.0 / F(n_points))  # one over the number of POINTS
        np.testing.assert_array_equal(g.download_odom_noise(), 0.0)
        with pytest.raises(capi.EngineError, match="before group_resample_begin"):
            g.resample_plan(0, 0.0)
    finally:
        g.close()


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[2]], ids=[IDS[0], IDS[2]])
def test_same_as_uploading_the_same_particles(cfg, map_b, points_b):
    sc = make_scene(n=91, n_p=8, n_s=300, n_b=16, seed=31, map_jitter=0.04)
    want_s, want_w = glr.particles(points_b, 12, IMU)
    a, b = group(cfg), group(cfg)
    try:
        for g in (a, b):
            configure(g, map_b)
        a.global_localization(0.3, 12, IMU)
        b.upload_state(want_s, want_w)
        ra = a.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        rb = b.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        for k in ("weights", "lik", "quality", "beam"):
            np.testing.assert_array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32), err_msg=k)
        assert F(ra["entropy"]).view(np.uint32) == F(rb["entropy"]).view(np.uint32)
        ea, eb = a.expectation(), b.expectation()
        np.testing.assert_array_equal(ea[0].view(np.uint32), eb[0].view(np.uint32))
        assert ea[1:] == eb[1:]
        for x, y in zip(a.download_state(), b.download_state()):
            np.testing.assert_array_equal(x, y)
    finally:
        a.close()
        b.close()


def test_base_map_only(map_b, points_b):
    sc = make_scene(n=91, n_p=8, n_s=300, n_b=16, seed=31, map_jitter=0.04)
    rng = np.random.default_rng(11)
    # a table-sized blob of new points in the middle of the room: standable points of its own if it were looked at
    overlay = (rng.uniform(-0.8, 0.8, (4000, 3)) * np.array([1.0, 1.0, 0.02]) + np.array([0.4, -0.3, -2.0])).astype(F)
    want_s, want_w = glr.particles(points_b, 5, IMU)
    e = capi.Engine(0)
    seeded, uploaded = group(CONFIGS[0]), group(CONFIGS[0])
    try:
        configure(e, map_b)
        e.map_update(overlay, None, leaf=(0.2, 0.2, 0.2), stamp=8201)
        assert len(e.map_download()[0]) > len(map_b)
        np.testing.assert_array_equal(e.global_localization_points(0.3)[0], points_b)
        e.map_update(None, None, leaf=(0.2, 0.2, 0.2), stamp=8202)  # overlay removed
        np.testing.assert_array_equal(e.global_localization_points(0.3)[0], points_b)
        # the overlay is still part of the map the next update measures against
        for g in (seeded, uploaded):
            configure(g, map_b)
            group_map_update(g, overlay)
        assert seeded.global_localization(0.3, 5, IMU) == (len(points_b), len(want_s))
        np.testing.assert_array_equal(seeded.download_state()[0], want_s)
        uploaded.upload_state(want_s, want_w)
        ra = seeded.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        rb = uploaded.update_resident(sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        for k in ("weights", "lik", "quality", "beam"):
            np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    finally:
        e.close()
        seeded.close()
        uploaded.close()


def test_map_index_is_left_alone(map_b, points_b):
    sc = make_scene(n=91, n_p=64, n_s=300, n_b=16, seed=31, map_jitter=0.04)
    e = capi.Engine(0)
    try:
        configure(e, map_b)
        q = sc.scan_lik + sc.true_pose[:3]
        before_update = e.measure_update(sc.poses, sc.weights, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        before_search = e.radius_search(q, 0.4)  # builds the cell-sorted map too
        stats, footprint = e.index_stats(), e.memory_footprint()
        assert stats["build_ms"] > 0 and all(footprint[k] > 0 for k in ("lik_points", "lik_cells", "dda_bits", "cand_table"))
        np.testing.assert_array_equal(e.global_localization_points(0.3)[0], points_b)
        assert e.index_stats() == stats and e.memory_footprint() == footprint
        after_update = e.measure_update(sc.poses, sc.weights, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        after_search = e.radius_search(q, 0.4)
        # no rebuild happened behind the update either: the build time is that of the one build
        assert e.index_stats() == stats and e.memory_footprint() == footprint
        for k in ("weights", "lik", "quality", "beam"):
            np.testing.assert_array_equal(before_update[k], after_update[k], err_msg=k)
        for x, y in zip(before_search, after_search):
            np.testing.assert_array_equal(x, y)
    finally:
        e.close()


def test_errors_leave_the_resident_particles_alone(map_b, points_b):
    st = np.random.default_rng(3).normal(0, 1, (50, 13)).astype(F)
    w = np.random.default_rng(4).uniform(0.1, 1, 50).astype(F)

    def unchanged(g):
        assert g.resident() == 50
        s2, w2 = g.download_state()
        np.testing.assert_array_equal(s2, st)
        np.testing.assert_array_equal(w2, w)

    g = group(CONFIGS[2])
    try:
        g.upload_state(st, w)
        with pytest.raises(capi.EngineError, match=r"error -5: .*no map"):
            g.global_localization(0.3, 12)
        unchanged(g)
        configure(g, map_b)
        for grid in (0.0, -0.3, float("nan")):
            with pytest.raises(capi.EngineError, match=r"error -3: .*grid"):
                g.global_localization(grid, 12)
        with pytest.raises(capi.EngineError, match=r"error -3: .*div_yaw"):
            g.global_localization(0.3, 0)
        with pytest.raises(capi.EngineError, match=r"error -3: .*imu_quat"):
            g.global_localization(0.3, 12, [0.0, 0.0, np.inf, 1.0])
        need = len(points_b) * 12
        with pytest.raises(capi.EngineError, match=r"error -3: .*%d particles needed" % need):
            g.global_localization(0.3, 12, max_particles=need - 1)
        unchanged(g)
        assert g.global_localization(0.3, 12, max_particles=need) == (len(points_b), need)
        # dist_weight_z * (0.01 + grid) < grid: every centroid finds itself
        g.upload_state(st, w)
        configure(g, scene_map(61, 0.04), dist_weight=(1.0, 1.0, 0.5), stamp=8300)
        with pytest.raises(capi.EngineError, match=r"error -5: .*no standable point"):
            g.global_localization(0.3, 12)
        unchanged(g)
    finally:
        g.close()
    e = capi.Engine(0)
    try:
        with pytest.raises(capi.EngineError, match=r"error -5: .*no map"):
            e.global_localization_points(0.3)
        e.set_map(map_b, None, stamp=8000, dist_weight=DW)
        with pytest.raises(capi.EngineError, match=r"error -5: .*global_localization_points first"):
            e.global_localization_seed_device(12, 0, 10)
        n, c = C.c_size_t(0), C.c_size_t(0)
        small = np.zeros((10, 3), F)
        assert e.lib.mcl3dl_hip_global_localization_points(e.h, 0.3, capi._ptr(small), 10, C.byref(n), C.byref(c)) == -3
        assert n.value == len(points_b)  # the count is there for the caller to come back with enough room
        with pytest.raises(capi.EngineError, match=r"error -3: .*exist"):
            e.global_localization_seed_device(12, len(points_b) * 12 - 5, 10)
    finally:
        e.close()


def test_seed_device_slices(map_b, points_b):
    import torch
    want_s, want_w = glr.particles(points_b, 12, IMU)
    e = capi.Engine(0)
    try:
        e.set_map(map_b, None, stamp=8000, dist_weight=DW)
        e.global_localization_points(0.3)
        first, count = 1001, 4099
        dev = torch.device("cuda:0")
        d_s = torch.full((count + 1, 13), -7.0, dtype=torch.float32, device=dev)
        d_p = torch.full((count + 1, 7), -7.0, dtype=torch.float32, device=dev)
        d_w = torch.full((count + 1,), -7.0, dtype=torch.float32, device=dev)
        e.global_localization_seed_device(12, first, count, d_s, d_p, d_w, imu_quat=IMU)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d_s[:count].cpu().numpy(), want_s[first:first + count])
        np.testing.assert_array_equal(d_p[:count].cpu().numpy(), want_s[first:first + count, :7])
        np.testing.assert_array_equal(d_w[:count].cpu().numpy(), want_w[first:first + count])
        for t in (d_s, d_p, d_w):  # nothing past the slice
            assert bool(torch.all(t[count:] == -7.0))
        e.global_localization_seed_device(12, first, count, None, d_p, None, imu_quat=IMU)  # any output may be absent
    finally:
        e.close()


# ---- the sweep: the feature used for what it is for ------------------------------------------------------------------------
SWEEP_GRID, SWEEP_DIV_YAW, SWEEP_NUM, SWEEP_DEF, SWEEP_GL = 0.3, 12, 500, 300, 8
SWEEP_SIGMA6 = [0.1, 0.1, 0.05, 0.02, 0.02, 0.05]


def sweep_world():
    """Hollow cube (n = 61) with two boxes standing on the floor, jittered by +-0.03: asymmetric, so that one pose explains a
    scan. Returns (map, random stream positioned behind the jitter draw, true position, true yaw)."""
    rng = np.random.default_rng(7)
    n = 61
    half = n * 0.1 / 2
    m = cube_map(n, 0.1).astype(np.float64)

    def box(x0, x1, y0, y1, h):
        pts = []
        zs = np.arange(-half + 0.05, -half + h, 0.1)
        for x in np.arange(x0, x1 + 1e-9, 0.1):
            for z in zs:
                pts += [[x, y0, z], [x, y1, z]]
        for y in np.arange(y0, y1 + 1e-9, 0.1):
            for z in zs:
                pts += [[x0, y, z], [x1, y, z]]
        for x in np.arange(x0, x1 + 1e-9, 0.1):
            for y in np.arange(y0, y1 + 1e-9, 0.1):
                pts.append([x, y, -half + h])
        return np.array(pts)

    m = np.concatenate([m, box(0.8, 1.9, -2.2, -0.9, 1.5), box(-2.4, -2.2, 0.3, 2.5, 2.0)])
    m = (m + rng.uniform(-0.03, 0.03, m.shape)).astype(F)
    return m, rng, np.array([-0.63, 1.12, -half + 0.02]), 2 * np.pi * 4 / SWEEP_DIV_YAW + 0.09


def test_global_localization_sweep_follows_the_reference():
    """Seed, then measure / resample / shrink by a quarter until 500 particles are left (src/mcl_3dl.cpp:875-888), the same
    sequence with the same drawn numbers on the reference-backed oracle: states and weights equal bit for bit after every
    iteration. That the sweep finds the pose is a condition on the INPUT and is asserted for the oracle's result; with the
    oracle alone the best particle ended 0.06-0.11 m and 0.02 rad from the truth."""
    m, rng, tp, tyaw = sweep_world()
    rot = quat_to_matrix(quat_from_rpy([0, 0, tyaw]))
    local = (m.astype(np.float64) - tp) @ rot
    r2 = local[:, 0] ** 2 + local[:, 1] ** 2
    vis = np.nonzero((r2 < 100) & (r2 > 0.25) & (local[:, 2] > -2) & (local[:, 2] < 2))[0]
    no_beam, origin = np.zeros((0, 3), F), np.zeros((1, 3), F)

    points = glr.standable_points(m, SWEEP_GRID, DW)[0]
    st, w = glr.particles(points, SWEEP_DIV_YAW)
    assert (len(points), len(st)) == (1147, 13764)
    ref = glr.ref_oracle()
    ref.set_map(m, None, stamp=9, dist_weight=DW)
    ref.set_likelihood_params(pyoracle.LikelihoodParams())
    ref.set_beam_params(pyoracle.BeamParams())
    g = group(CONFIGS[0])
    try:
        configure(g, m, stamp=9)
        g.set_option("strict_order", 1)  # the reference's float sums for the weights at every particle count
        assert g.global_localization(SWEEP_GRID, SWEEP_DIV_YAW) == (1147, 13764)
        it = 0
        while len(st) > SWEEP_NUM:
            n = len(st)
            num = max(SWEEP_GL, SWEEP_DEF * SWEEP_NUM // n)
            idx = rng.integers(0, len(vis), num)
            scan = (local[vis[idx]] + rng.normal(0, 0.01, (num, 3))).astype(F)
            # ---- measure
            want = ref.measure_update(st[:, :7], w, scan, no_beam, None, origin)
            got = g.update_resident(scan, extra=np.full(n, ODOM0, F))
            np.testing.assert_array_equal(got["lik"], want["lik"], err_msg="likelihoods, iteration %d" % it)
            np.testing.assert_array_equal(got["weights"], want["weights"], err_msg="weights, iteration %d" % it)
            assert got["restored"] == want["restored"]
            w = want["weights"]
            # ---- resample, the noise of the duplicated particles drawn by the reference's own engine
            seed = 1000 + it
            st, w = ref.resample(st, w, seed, SWEEP_SIGMA6)
            pstep = g.resample_begin(0)
            initial_p, _ = ref.resample_draws(seed, pstep, SWEEP_SIGMA6, 0)
            _, _, n_dup = g.resample_plan(0, initial_p)
            _, noise = ref.resample_draws(seed, pstep, SWEEP_SIGMA6, n_dup)
            g.resample_apply(noise)
            # ---- resizeParticle to three quarters
            n_out = max(SWEEP_NUM, int(n * 0.75))
            st, w = ref.resize(st, w, n_out)
            g.resample_begin(n_out)
            assert g.resample_plan(1)[2] == 0
            g.resample_apply(None)
            got_s, got_w = g.download_state()
            np.testing.assert_array_equal(got_s.view(np.uint32), st.view(np.uint32), err_msg="states, iteration %d" % it)
            np.testing.assert_array_equal(got_w, w, err_msg="weights after resize, iteration %d" % it)
            it += 1
        assert it == 12 and len(st) == SWEEP_NUM
        # ---- where the 500 particles are
        scan = (local[vis[rng.integers(0, len(vis), SWEEP_DEF)]] + rng.normal(0, 0.01, (SWEEP_DEF, 3))).astype(F)
        want = ref.measure_update(st[:, :7], w, scan, no_beam, None, origin)
        got = g.update_resident(scan, extra=np.full(len(st), ODOM0, F))
        np.testing.assert_array_equal(got["weights"], want["weights"])
        _, i_max, _ = ref.expectation(st[:, :7], want["weights"])
        assert g.expectation()[2] == i_max
        best = st[i_max, :7].astype(np.float64)
        err_xy = np.hypot(*(best[:2] - tp[:2]))
        err_yaw = abs((2 * np.arctan2(best[5], best[6]) - tyaw + np.pi) % (2 * np.pi) - np.pi)
        print("sweep: best particle %.3f m, %.3f rad from the true pose after %d iterations" % (err_xy, err_yaw, it))
        assert err_xy < SWEEP_GRID and err_yaw < np.pi / SWEEP_DIV_YAW  # the ORACLE's result: a condition on the input
    finally:
        g.close()
        ref.close()
