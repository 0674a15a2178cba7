"""Clouds accumulated on the device (mcl_3dl_amd/csrc/scan_accum.h, host_cloud.h, api_cloud.inl, api_group_state.inl):
mcl3dl_hip_scan_accum_clear / _push / _push_pointcloud2 / _size / _download, _scan_begin_accumulated and their group forms.

Yardsticks: tests/scan_accum_ref.py — the float32 restatement of both transforms that tests/test_scan_accum_cpu.py holds against
float64 and against the header compiled for the host — and the parent's own route: the restatement applied on the host, the
finished cloud and its labels handed to scan_begin. Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import rng_index_ref as rir
import scan_accum_ref as sar
import test_gpu_scan_prepared as tsp
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
F = np.float32
LEAF, CLIP_LIK, CLIP_BEAM = tsp.LEAF, tsp.CLIP_LIK, tsp.CLIP_BEAM
PREP = dict(leaf=LEAF, clip_lik=CLIP_LIK, clip_beam=CLIP_BEAM)
# either side of a wavefront, of a 256-thread work-group and of the second min / max work-group (1024 points each), and several
ELEVEN = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3001)
# (point_step, off_x, off_y, off_z, off_label): xyz + intensity; a label field present (it is ignored); unaligned
LAYOUTS = {"step16": (16, 0, 4, 8, None), "step32-label": (32, 0, 4, 8, 16), "step22-unaligned": (22, 2, 10, 6, None)}


def hom(m):
    return np.vstack([np.asarray(m, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])


class Frames:
    """Three sensors mounted on the robot, the robot somewhere in the odom frame: odom <- sensor per cloud, base_link <- odom, and
    the sensors' positions in base_link (the per-cloud origins of src/mcl_3dl.cpp:343-359)."""

    def __init__(self):
        robot = hom(sar.rigid((0.01, -0.02, 0.8), (250.0, -120.0, 3.0)))
        mounts = [hom(sar.rigid((0.0, 0.0, 0.0), (0.0, 0.0, 0.5))), hom(sar.rigid((0.02, 0.3, -1.2), (0.2, 0.0, 0.5))),
                  hom(sar.rigid((-0.4, 0.01, 2.5), (-0.1, 0.1, 0.6)))]
        self.mounts = mounts
        self.to_odom = [(robot @ s)[:3].astype(F) for s in mounts]
        self.to_base = np.linalg.inv(robot)[:3].astype(F)
        self.origins = np.stack([s[:3, 3] for s in mounts]).astype(F)

    def sensor_clouds(self, pieces):
        """What each sensor would have seen for the robot-frame piece to come out (up to float32 rounding)."""
        out = []
        for s, p in zip(self.mounts, pieces):
            q = np.concatenate([p.astype(np.float64), np.ones((len(p), 1))], 1) @ np.linalg.inv(s).T
            out.append(np.ascontiguousarray(q[:, :3].astype(F)))
        return out


@pytest.fixture(scope="module")
def sc():
    return make_scene(n=91, n_p=300, n_s=1800, n_b=600, seed=41)


@pytest.fixture(scope="module")
def frames():
    return Frames()


@pytest.fixture(scope="module")
def three(sc, frames):
    """Three sensor clouds, about 3000 points, and what the parent's route makes of them on the host: (clouds, host cloud in
    base_link, labels)."""
    clouds = frames.sensor_clouds([sc.scan_lik, sc.scan_beam, sc.scan_lik[::3] + F(0.004)])
    acc, lab = sar.accumulate(clouds, frames.to_odom)
    return clouds, sar.to_base(acc, frames.to_base), lab


@pytest.fixture(scope="module")
def eng(sc):
    e = capi.Engine(0)
    tsp.configure(e, sc)
    yield e
    e.close()


@pytest.fixture(scope="module")
def g1(sc):
    g = tsp.make_group(sc, [0], None, 1)
    yield g
    g.close()


@pytest.fixture(scope="module")
def g3(sc):
    g = tsp.make_group(sc, [0, 0, 0], "host", 1)
    yield g
    g.close()


@pytest.fixture(scope="module")
def g1s(sc):
    g = tsp.make_group(sc, [0], None, 0)
    yield g
    g.close()


@pytest.fixture(params=["n1-direct", "n3-host", "n1-sharded"])
def group(request, g1, g3, g1s):
    return {"n1-direct": g1, "n3-host": g3, "n1-sharded": g1s}[request.param]


def push_all(obj, clouds, affines):
    obj.scan_accum_clear()
    total = 0
    for k, (c, m) in enumerate(zip(clouds, affines)):
        total += len(c)
        assert obj.scan_accum_push(c, m) == (k, total)


def push_pc2(obj, cloud, affine, layout, rng=None):
    step, ox, oy, oz, ol = LAYOUTS[layout]
    labels = None if ol is None else np.full(len(cloud), 777, np.uint32)
    fill = 0xA5 if rng is None else int(rng.integers(0, 256))
    return obj.scan_accum_push_pointcloud2(sar.pack_pointcloud2(cloud, step, ox, oy, oz, fill, ol, labels), len(cloud), step, ox,
                                           oy, oz, affine)


def assert_cloud(got, xyz, label):
    np.testing.assert_array_equal(got[0].view(np.uint32), np.asarray(xyz, F).reshape(-1, 3).view(np.uint32))
    np.testing.assert_array_equal(got[1], label)


def prepared(e):
    return [e.scan_download(k) for k in (0, 1, 2)]


def assert_same_clouds(got, want):
    for a, b in zip(got, want):
        assert_cloud(a, b[0], b[1])


def test_bits_of_the_accumulation(eng):
    rng = np.random.default_rng(11)
    clouds = [rng.uniform(-40.0, 40.0, (n, 3)).astype(F) for n in ELEVEN]
    affines = [sar.rigid(rng.uniform(-3.1, 3.1, 3), rng.uniform(-t, t, 3)) for t in (0, 1, 10, 50, 100, 300, 500, 1000, 2000, 2000)]
    affines.insert(4, None)   # one cloud is appended as it is
    to_base = sar.rigid((0.03, -0.01, -2.2), (-1800.0, 1500.0, 20.0))
    push_all(eng, clouds, affines)
    want_xyz, want_lab = sar.accumulate(clouds, affines)
    assert eng.scan_accum_size() == (11, sum(ELEVEN)) and len(want_xyz) == sum(ELEVEN)
    np.testing.assert_array_equal(want_lab, np.repeat(np.arange(11, dtype=np.uint32), ELEVEN))
    assert_cloud(eng.scan_accum_download(), want_xyz, want_lab)
    assert eng.scan_begin_accumulated(to_base, leaf=None, clip_lik=None, clip_beam=None) == (sum(ELEVEN), 0, 0)
    assert_cloud(eng.scan_download(0), sar.to_base(want_xyz, to_base), want_lab)
    # no second transform: the accumulation's own bits
    eng.scan_begin_accumulated(None, leaf=None, clip_lik=None, clip_beam=None)
    assert_cloud(eng.scan_download(0), want_xyz, want_lab)
    assert_cloud(eng.scan_accum_download(), want_xyz, want_lab)


def test_same_as_the_parents_route_end_to_end(eng, sc, frames, three):
    clouds, host_cloud, host_lab = three
    pose = sc.poses[0]
    want_sizes = eng.scan_begin(host_cloud, host_lab, **PREP)
    n_full, n_lik, n_beam = want_sizes
    assert n_full < len(host_cloud) and n_lik > 0 and n_beam > 0 and n_lik != n_beam
    want = prepared(eng)
    assert set(np.unique(want[2][1])) == {0, 1, 2}   # every origin casts rays
    idx_l, idx_b, _ = rir.scan_draws(12345, 700, n_lik, 48, n_beam)
    eng.scan_finish(idx_l, idx_b, origins=frames.origins)
    want_installed = tsp.installed(eng, sc.poses)
    want_split = eng.match_split(pose)
    assert np.count_nonzero(want_installed[-1][4]) > len(sc.poses) // 2   # the beam model is on
    # the new route, behind something else in the scan path's buffers
    eng.scan_begin(sc.scan_lik[:100], None, **PREP)
    push_all(eng, clouds, frames.to_odom)
    assert eng.scan_begin_accumulated(frames.to_base, **PREP) == want_sizes
    assert_same_clouds(prepared(eng), want)
    eng.scan_finish(idx_l, idx_b, origins=frames.origins)
    tsp.assert_same_installed(tsp.installed(eng, sc.poses), want_installed)
    got_split = eng.match_split(pose)
    assert len(want_split[0]) > 0 and len(want_split[1]) > 0
    for a, b in zip(got_split, want_split):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_pointcloud2_form_equals_the_plain_push(eng, frames, three, layout):
    clouds = three[0]
    push_all(eng, clouds, frames.to_odom)
    want = eng.scan_accum_download()
    eng.scan_accum_clear()
    total = 0
    for k, (c, m) in enumerate(zip(clouds, frames.to_odom)):
        total += len(c)
        assert push_pc2(eng, c, m, layout) == (k, total)
    assert_cloud(eng.scan_accum_download(), want[0], want[1])
    assert_cloud(want, *sar.accumulate(clouds, frames.to_odom))


def test_growth_keeps_the_contents():
    """A context of its own, so that the buffer starts empty: 100 points, then 200 000 (the buffer grows), then 350 001 (more than
    a staged copy takes: straight from the caller's array, and the buffer grows again). Then 200 000 twice with nothing between:
    the second finds more than a staging block's worth of copies pending and drains the stream."""
    rng = np.random.default_rng(5)
    clouds = [rng.uniform(-30.0, 30.0, (n, 3)).astype(F) for n in (100, 200000, 350001)]
    affines = [sar.rigid((0.1, 0.2, 0.3), (5.0, 6.0, 7.0)), sar.rigid((-1.0, 0.5, 2.0), (-300.0, 20.0, 1.0)), None]
    e = capi.Engine(0)
    try:
        assert e.scan_accum_size() == (0, 0)
        assert e.scan_accum_push(clouds[0], affines[0]) == (0, 100)
        first = e.scan_accum_download()
        assert e.scan_accum_push(clouds[1], affines[1]) == (1, 200100)
        want_xyz, want_lab = sar.accumulate(clouds[:2], affines[:2])
        got = e.scan_accum_download()
        assert_cloud((got[0][:100], got[1][:100]), first[0], first[1])
        assert_cloud(got, want_xyz, want_lab)
        scratch = clouds[2].copy()
        assert e.scan_accum_push(scratch, affines[2]) == (2, 550101)
        scratch[:] = 0.0   # the caller's array is its own again when the push returns
        assert_cloud(e.scan_accum_download(), *sar.accumulate(clouds, affines))
        # cleared and filled again: nothing of the old contents shows
        e.scan_accum_clear()
        assert e.scan_accum_push(clouds[0], None) == (0, 100)
        assert_cloud(e.scan_accum_download(), clouds[0], np.zeros(100, np.uint32))
        assert e.scan_accum_push(clouds[1], affines[1]) == (1, 200100)
        assert e.scan_accum_push(clouds[1], affines[0]) == (2, 400100)
        assert_cloud(e.scan_accum_download(), *sar.accumulate([clouds[0], clouds[1], clouds[1]], [None, affines[1], affines[0]]))
    finally:
        e.close()


def test_lifetime(eng, sc, frames, three):
    clouds, host_cloud, host_lab = three
    push_all(eng, clouds[:2], frames.to_odom[:2])
    sizes = eng.scan_begin_accumulated(frames.to_base, **PREP)
    first = prepared(eng)
    held = eng.scan_accum_download()
    assert eng.scan_begin_accumulated(frames.to_base, **PREP) == sizes
    assert_same_clouds(prepared(eng), first)
    assert_cloud(eng.scan_accum_download(), held[0], held[1])
    # a push behind it continues the index, and the next begin sees all three
    assert eng.scan_accum_push(clouds[2], frames.to_odom[2]) == (2, len(host_cloud))
    eng.scan_begin_accumulated(frames.to_base, **PREP)
    got = prepared(eng)
    want_sizes = eng.scan_begin(host_cloud, host_lab, **PREP)
    assert_same_clouds(got, prepared(eng))
    # cleared: nothing to begin with, and the prepared scan is still there
    eng.scan_accum_clear()
    assert eng.scan_accum_size() == (0, 0) and len(eng.scan_accum_download()[0]) == 0
    with pytest.raises(capi.EngineError, match="-5.*scan_accum_push"):
        eng.scan_begin_accumulated(frames.to_base, **PREP)
    assert_same_clouds(prepared(eng), got)
    idx_l, idx_b, _ = rir.scan_draws(7, 96, want_sizes[1], 3, want_sizes[2])
    eng.scan_finish(idx_l, idx_b, origins=frames.origins)
    assert len(eng.scan_download(3)[0]) == 96 and len(eng.scan_download(4)[0]) == 3
    assert eng.scan_accum_push(clouds[0], None) == (0, len(clouds[0]))


def test_no_aliasing(sc, frames, three):
    """A context of its own: its map is updated. Between the two pushes everything else that writes the scan path's raw buffer
    and the upload staging runs."""
    import torch
    clouds = three[0]
    e = capi.Engine(0)
    try:
        tsp.configure(e, sc)
        push_all(e, clouds[:2], frames.to_odom[:2])
        e.scan_begin_accumulated(frames.to_base, **PREP)
        want, want_acc = prepared(e), e.scan_accum_download()
        e.scan_accum_clear()
        assert e.scan_accum_push(clouds[0], frames.to_odom[0]) == (0, len(clouds[0]))
        # an unrelated cloud through scan_begin + scan_finish + an update
        other = np.concatenate([sc.scan_beam, sc.scan_lik[5::7]], 0) + F(0.01)
        _, n_lik, n_beam = e.scan_begin(other, None, **PREP)
        idx_l, idx_b, _ = rir.scan_draws(3, 200, n_lik, 8, n_beam)
        e.scan_finish(idx_l, idx_b, origins=sc.origins)
        dev = torch.device("cuda", 0)
        n_p = len(sc.poses)
        d_pose = torch.from_numpy(sc.poses).to(dev)
        d_w = torch.full((n_p,), 1.0 / n_p, dtype=torch.float32, device=dev)
        d_st = torch.zeros(4, dtype=torch.float32, device=dev)
        e.update_device(d_pose, n_p, d_w, d_st)
        e.synchronize()
        # a map update, and a match_split with points of its own
        e.map_update(sc.map_xyz[::50] + F(0.03), None)
        e.match_split(sc.poses[0], xyz=sc.scan_lik[:300])
        assert e.scan_accum_push(clouds[1], frames.to_odom[1]) == (1, len(clouds[0]) + len(clouds[1]))
        assert_cloud(e.scan_accum_download(), want_acc[0], want_acc[1])
        e.scan_begin_accumulated(frames.to_base, **PREP)
        assert_same_clouds(prepared(e), want)
    finally:
        e.close()


def test_seeded_sequence_against_a_model():
    """pushes of both forms, clears, scan_begin_accumulated and scan_begin of other clouds in a seeded order; the VoxelGrid and the
    clips are skipped, so that the prepared cloud is the raw one and the model stays a few lines of numpy."""
    rng = np.random.default_rng(20240)
    mats = [None, sar.rigid((0.2, -0.1, 1.0), (3.0, -4.0, 0.5)), sar.rigid((-2.0, 0.4, 0.3), (-700.0, 900.0, 12.0)),
            sar.rigid((0.0, 0.0, 3.0), (2000.0, 2000.0, -5.0))]
    raw = dict(leaf=None, clip_lik=None, clip_beam=None)
    e = capi.Engine(0)
    try:
        clouds, affines, prep = [], [], None
        ops = ["push", "pc2", "clear", "begin_acc", "scan_begin"]
        steps = list(rng.choice(ops, 30, p=[0.3, 0.25, 0.1, 0.25, 0.1]))
        steps[:4] = ["push", "pc2", "scan_begin", "begin_acc"]
        steps[12:14] = ["clear", "begin_acc"]   # (nothing to begin with: -5)
        seen = set()
        for step in steps:
            n = int(rng.integers(1, 400))
            cloud = rng.uniform(-20.0, 20.0, (n, 3)).astype(F)
            m = mats[int(rng.integers(0, len(mats)))]
            if step in ("push", "pc2"):
                if step == "push":
                    got = e.scan_accum_push(cloud, m)
                else:
                    got = push_pc2(e, cloud, m, sorted(LAYOUTS)[int(rng.integers(0, 3))], rng)
                clouds.append(cloud)
                affines.append(m)
                assert got == (len(clouds) - 1, sum(len(c) for c in clouds))
            elif step == "clear":
                e.scan_accum_clear()
                clouds, affines = [], []
            elif step == "begin_acc":
                if clouds:
                    acc, lab = sar.accumulate(clouds, affines)
                    assert e.scan_begin_accumulated(m, **raw) == (len(acc), 0, 0)
                    prep = (sar.to_base(acc, m), lab)
                else:
                    step = "begin_acc-empty"
                    with pytest.raises(capi.EngineError, match="-5"):
                        e.scan_begin_accumulated(m, **raw)
            else:
                lab = rng.integers(0, 9, n).astype(np.uint32)
                assert e.scan_begin(cloud, lab, **raw) == (n, 0, 0)
                prep = (cloud, lab)
            seen.add(step)
            acc, lab = sar.accumulate(clouds, affines)
            assert e.scan_accum_size() == (len(clouds), len(acc))
            assert_cloud(e.scan_accum_download(), acc, lab)
            if prep is not None:
                assert_cloud(e.scan_download(0), prep[0], prep[1])
        assert seen == set(ops) | {"begin_acc-empty"}, seen
    finally:
        e.close()


def long_way_labelled(eng, g, cloud, label, idx_l, idx_b, origins):
    """tests/test_gpu_scan_prepared.py's long_way for a cloud that carries labels: prepare on one context, fetch the sampled clouds,
    hand them to the group as host scans."""
    eng.scan_begin(cloud, label, **PREP)
    eng.scan_finish(idx_l, idx_b, origins=origins)
    lik_xyz, _ = eng.scan_download(3)
    beam_xyz, beam_label = eng.scan_download(4)
    return g.update_resident(lik_xyz, beam_xyz, beam_label, origins)


def test_groups(group, eng, sc, frames, three):
    g = group
    clouds, host_cloud, host_lab = three
    n_p = 301 if g.n == 3 else 300
    s, w = tsp.states(sc, n_p)
    # the single context's
    push_all(eng, clouds, frames.to_odom)
    want_sizes = eng.scan_begin_accumulated(frames.to_base, **PREP)
    want_acc, want_prep = eng.scan_accum_download(), prepared(eng)
    # the group's: both forms of push
    g.scan_accum_clear()
    assert g.scan_accum_size() == (0, 0)
    assert g.scan_accum_push(clouds[0], frames.to_odom[0]) == (0, len(clouds[0]))
    assert push_pc2(g, clouds[1], frames.to_odom[1], "step22-unaligned") == (1, len(clouds[0]) + len(clouds[1]))
    assert g.scan_accum_push(clouds[2], frames.to_odom[2]) == (2, len(host_cloud))
    assert g.scan_accum_size() == (3, len(host_cloud))
    assert g.scan_begin_accumulated(frames.to_base, **PREP) == want_sizes
    for r in range(g.n):
        ctx = g.context(r)
        assert_cloud(ctx.scan_accum_download(), want_acc[0], want_acc[1])
        assert_same_clouds(prepared(ctx), want_prep)
        ctx.close()
    state = 2024
    idx_l, idx_b, behind = rir.scan_draws(state, 700, want_sizes[1], 48, want_sizes[2])
    g.upload_state(s, w)
    assert g.scan_finish_drawn(700, 48, frames.origins, state) == (700, 48, behind)
    got = g.update_resident_prepared()
    g.upload_state(s, w)
    want = long_way_labelled(eng, g, host_cloud, host_lab, idx_l, idx_b, frames.origins)
    assert np.count_nonzero(want["lik"]) > n_p // 2 and np.count_nonzero(want["beam"]) > n_p // 2
    tsp.assert_same_update(got, want)
    # one cloud, label 0 throughout: that file's long_way itself, which hands scan_begin no labels
    g.scan_accum_clear()
    acc, _ = sar.accumulate(clouds[:1], frames.to_odom[:1])
    one = sar.to_base(acc, frames.to_base)
    assert g.scan_accum_push(clouds[0], frames.to_odom[0]) == (0, len(one))
    _, n_lik, n_beam = g.scan_begin_accumulated(frames.to_base, **PREP)
    idx_l, idx_b, behind = rir.scan_draws(state, 700, n_lik, 16, n_beam)
    g.upload_state(s, w)
    assert g.scan_finish_drawn(700, 16, frames.origins[:1], state) == (700, 16, behind)
    got = g.update_resident_prepared()
    g.upload_state(s, w)
    tsp.assert_same_update(got, tsp.long_way(eng, g, one, idx_l, idx_b, frames.origins[:1]))


def test_errors_leave_the_accumulation_and_the_prepared_scan(eng, g3, frames, three):
    clouds = three[0]
    lib = eng.lib
    push_all(eng, clouds[:2], frames.to_odom[:2])
    eng.scan_begin_accumulated(frames.to_base, **PREP)
    held, prep = eng.scan_accum_download(), prepared(eng)
    size = eng.scan_accum_size()

    def untouched():
        assert eng.scan_accum_size() == size
        assert_cloud(eng.scan_accum_download(), held[0], held[1])
        assert_same_clouds(prepared(eng), prep)

    def raw_push(xyz, n, affine):
        idx, tot = C.c_size_t(99), C.c_size_t(99)
        rc = lib.mcl3dl_hip_scan_accum_push(eng.h, capi._ptr(xyz), n, capi._ptr(affine), C.byref(idx), C.byref(tot))
        return rc, lib.mcl3dl_hip_last_error(eng.h).decode()

    some = clouds[2][:10]
    ok = np.ascontiguousarray(frames.to_odom[2].reshape(-1))
    with pytest.raises(capi.EngineError, match="-3.*Given PointCloud2 is empty"):
        eng.scan_accum_push(np.zeros((0, 3), F), ok)
    with pytest.raises(capi.EngineError, match="-3.*Given PointCloud2 is empty"):
        eng.scan_accum_push_pointcloud2(b"", 0, 16, 0, 4, 8, ok)
    rc, msg = raw_push(None, 10, ok)
    assert rc == -3 and "null" in msg, msg
    assert lib.mcl3dl_hip_scan_accum_push_pointcloud2(eng.h, None, 10, 16, 0, 4, 8, None, None, None) == -3
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 7, 11):
            m = ok.copy()
            m[k] = bad
            with pytest.raises(capi.EngineError, match="-3.*affine12.%d" % k):
                eng.scan_accum_push(some, m)
            with pytest.raises(capi.EngineError, match="-3.*affine12.%d" % k):
                push_pc2(eng, some, m, "step16")
            with pytest.raises(capi.EngineError, match="-3.*affine12.%d" % k):
                eng.scan_begin_accumulated(m, **PREP)
    untouched()
    data = sar.pack_pointcloud2(some, 16, 0, 4, 8)
    for offs in ((0, 4, 13), (13, 4, 8), (0, 16, 8)):
        with pytest.raises(capi.EngineError, match="-3.*does not fit point_step"):
            eng.scan_accum_push_pointcloud2(data, len(some), 16, *offs, ok)
    with pytest.raises(capi.EngineError, match="-3.*x, y, z"):
        eng.scan_accum_push_pointcloud2(data, len(some), 16, 0, -1, 8, ok)
    # 2^31 - 1 points in total at the most (refused before the array is looked at)
    rc, msg = raw_push(some, 2 ** 31 - size[1], ok)
    assert rc == -3 and "2147483647" in msg, msg
    n = C.c_size_t(0)
    small = np.zeros((size[1] - 1, 3), F)
    assert lib.mcl3dl_hip_scan_accum_download(eng.h, capi._ptr(small), None, len(small), C.byref(n)) == -3 and n.value == size[1]
    untouched()
    # a refused push consumed no index
    assert eng.scan_accum_push(some, ok) == (2, size[1] + 10)
    # the group's forms report the same, on every rank
    g3.scan_accum_clear()
    assert g3.scan_accum_push(clouds[0], frames.to_odom[0]) == (0, len(clouds[0]))
    g3.scan_begin_accumulated(frames.to_base, **PREP)
    before = [(c.scan_accum_download(), prepared(c)) for c in (g3.context(r) for r in range(g3.n))]
    with pytest.raises(capi.EngineError, match="-3.*Given PointCloud2 is empty"):
        g3.scan_accum_push(np.zeros((0, 3), F), ok)
    bad = ok.copy()
    bad[3] = np.nan
    with pytest.raises(capi.EngineError, match="-3.*affine12.3"):
        g3.scan_accum_push(some, bad)
    with pytest.raises(capi.EngineError, match="-3.*affine12.3"):
        g3.scan_begin_accumulated(bad, **PREP)
    with pytest.raises(capi.EngineError, match="-3.*does not fit point_step"):
        g3.scan_accum_push_pointcloud2(data, len(some), 16, 0, 4, 13, ok)
    assert g3.scan_accum_size() == (1, len(clouds[0]))
    for r, (acc, prep_r) in enumerate(before):
        ctx = g3.context(r)
        assert_cloud(ctx.scan_accum_download(), acc[0], acc[1])
        assert_same_clouds(prepared(ctx), prep_r)
        ctx.close()
    g3.scan_accum_clear()
    with pytest.raises(capi.EngineError, match="-5.*scan_accum_push"):
        g3.scan_begin_accumulated(frames.to_base, **PREP)
    assert_same_clouds(prepared(g3.context(0)), before[0][1])
