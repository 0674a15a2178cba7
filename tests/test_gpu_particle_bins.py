"""The occupied-bin statistic on the GPU (mcl_3dl_amd/csrc/particle_bins_kernels.h, api_particle_bins.inl)
against tests/particle_bins_ref.py: keys, counts, leaders, occupied and occupied_alive bit for bit; masses bit for bit where
every summation order is exact, and within the bound of fp64 summation in any order otherwise.

The distributions are laid out in SORTED order (one bin per x cell, particles then shuffled), so that runs sit where the
segmented reduction can go wrong: on a work-group's last entry, across several work-groups of 1024 entries, all in one run."""
import ctypes as C

import numpy as np
import pytest

import particle_bins_ref as ref
from mcl_3dl_amd import capi

pytestmark = pytest.mark.gpu
F = np.float32
BLOCK = 1024          # entries per work-group of the reduction (PB_BLOCK)
BIN = (0.5, 0.5, 0.5)
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4097]
DISTRIBUTIONS = ["one-bin", "distinct", "runs-1-2-3", "run-from-block-end", "run-over-blocks"]


@pytest.fixture(scope="module")
def eng():
    import torch  # noqa: F401  (before the engine: one shared HIP runtime in the process)
    e = capi.Engine(0)
    yield e
    e.close()


def bin_ids(n, dist):
    """The bin of every SORTED position."""
    if dist == "one-bin":
        return np.zeros(n, np.int64)
    if dist == "distinct":
        return np.arange(n, dtype=np.int64)
    if dist == "runs-1-2-3":
        lengths = np.arange(1, int(np.sqrt(2 * n)) + 3)
        return np.repeat(np.arange(len(lengths)), lengths)[:n]
    if dist == "run-from-block-end":      # ... of the first work-group: positions 1023 ... 1027; distinct bins around it
        start, end = min(BLOCK - 1, n - 1), min(BLOCK + 4, n)
    else:                                 # three whole work-groups and parts of two more (at 4097; the same shape scaled below)
        start, end = (700, n) if n >= 4 * BLOCK + 1 else (n // 6, n - n // 7)
    ids = np.arange(n, dtype=np.int64)
    ids[start:end] = start
    return ids


def rows_of(ids, seed, yaw=False):
    """One particle per sorted position in the x cell ids[k] (cell centres: exact in float32), in shuffled particle order."""
    rng = np.random.default_rng(seed)
    n = len(ids)
    rows = np.zeros((n, 7), F)
    rows[:, 0] = (ids.astype(np.float64) + 0.5) * BIN[0] - 3.0
    rows[:, 1], rows[:, 2] = -1.25, 0.75
    rows[:, 6] = 1.0
    if yaw:
        q = rng.normal(size=(n, 4))
        rows[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return rows[rng.permutation(n)]


def exact_weights(n, seed, levels):
    """Multiples of 2^-20 below levels * 2^-20: every summation order is exact in fp64 (and ties in mass abound)."""
    return (np.random.default_rng(seed).integers(0, levels, n).astype(np.float64) * 2.0 ** -20).astype(F)


def on_device(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


def run(eng, rows, w, bin_xyz=BIN, yaw_bins=1, top_k=16, stride=7):
    rows = np.ascontiguousarray(rows, F).reshape(-1, 7)
    if stride > 7:
        wide = np.full((len(rows), stride), 1e30, F)   # what lies behind the pose is never read
        wide[:, :7] = rows
        rows = wide
    d_rows, d_w = on_device(rows, np.asarray(w, F))
    return eng.particle_bins_device(d_rows, d_w, len(rows), bin_xyz, yaw_bins=yaw_bins, top_k=top_k, row_stride=stride)


def reference(rows, w, bin_xyz=BIN, yaw_bins=1, top_k=16):
    return ref.bins(rows, w, bin_xyz, yaw_bins, capi.yaw_sector_table(yaw_bins), top_k=top_k)


def top_rows(got):
    return [(got["top_bin"][k].tolist(), float(got["top_mass"][k]), int(got["top_count"][k]), int(got["top_leader"][k]))
            for k in range(len(got["top_mass"]))]


def assert_exact(got, want, top_k=16):
    assert (got["occupied"], got["occupied_alive"], got["nonfinite"]) == (want["occupied"], want["occupied_alive"], want["nonfinite"])
    assert len(got["top_mass"]) == min(top_k, want["occupied"])
    rows = top_rows(got)
    assert rows == want["top"]                                        # bins, counts, leaders, the ORDER (mass, then key)
    assert [np.float64(r[1]).tobytes() for r in rows] == [np.float64(r[1]).tobytes() for r in want["top"]]   # the masses' bits


# ---- sizes x distributions, weights whose sums are exact ---------------------------------------------------------------------
@pytest.mark.parametrize("dist", DISTRIBUTIONS)
@pytest.mark.parametrize("n", SIZES)
def test_exact_masses_counts_leaders_and_order(eng, n, dist):
    ids = bin_ids(n, dist)
    rows = rows_of(ids, seed=n)
    # few weight levels where bins are many: masses tie and the key decides, zero masses leave bins dead
    w = exact_weights(n, seed=n + 1, levels=6 if dist in ("distinct", "run-from-block-end") else 4096)
    want = reference(rows, w)
    assert want["occupied"] == len(np.unique(ids))
    if dist == "distinct" and n >= 63:
        masses = [r[1] for r in want["top"]]
        assert len(set(masses)) < len(masses) and want["occupied_alive"] < want["occupied"]   # the case holds a tie and dead bins
    assert_exact(run(eng, rows, w), want)


@pytest.mark.parametrize("n", [70001, 524289])
@pytest.mark.parametrize("n_bins", [1, 8])
def test_converged_filters_at_large_sizes(eng, n, n_bins):
    """Everything in one bin, and in about eight: runs of tens of thousands of entries over up to 513 work-groups."""
    rng = np.random.default_rng(n + n_bins)
    ids = np.sort(rng.integers(0, n_bins, n))
    rows = rows_of(ids, seed=n)
    w = exact_weights(n, seed=n + 2, levels=4096)
    want = reference(rows, w)
    assert want["occupied"] == n_bins
    assert_exact(run(eng, rows, w), want)


# ---- float weights: any order of fp64 additions -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1025, 4097, 70001])
def test_random_weights_within_the_summation_bound(eng, n):
    rng = np.random.default_rng(n)
    ids = np.sort(rng.integers(0, 13, n))
    rows = rows_of(ids, seed=n + 5)
    w = (rng.random(n) ** 8).astype(F)     # eight orders of magnitude
    want = reference(rows, w)
    got = run(eng, rows, w)
    assert (got["occupied"], got["occupied_alive"], got["nonfinite"]) == (want["occupied"], want["occupied_alive"], 0)
    assert want["occupied"] <= 16 and len(got["top_mass"]) == want["occupied"]
    rows_got = top_rows(got)
    assert sorted((r[0], r[2], r[3]) for r in rows_got) == sorted((r[0], r[2], r[3]) for r in want["top"])
    by_bin = {tuple(ref.key_parts(k, want["grid"], 1)): b for k, b in want["bins"].items()}
    for bin4, mass, count, _ in rows_got:
        _, exact, _, abs_mass = by_bin[tuple(bin4)]
        # count fp64 additions of floats in ANY order stay within count * 2^-53 * sum |w| of the exact sum: nothing is measured
        assert abs(mass - exact) <= count * 2.0 ** -53 * abs_mass, (bin4, mass, exact)
    assert all(a[1] >= b[1] for a, b in zip(rows_got, rows_got[1:]))
    again = run(eng, rows, w)                                           # the same data, the same bits
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k


# ---- yaw sectors, strides, edge cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [7, 13])
@pytest.mark.parametrize("yaw_bins", [1, 4, 36])
def test_yaw_sectors_and_row_strides(eng, yaw_bins, stride):
    n = 3001
    rng = np.random.default_rng(yaw_bins)
    rows = rows_of(np.sort(rng.integers(0, 5, n)), seed=stride, yaw=True)
    rows[:, 1:3] = rng.uniform(-0.9, 0.9, (n, 2))          # a few cells in y and z as well
    rows[7, 3:] = np.nan                                     # a NaN quaternion: sector 0
    rows[8, 3:] = [0.5, 0.5, 0.5, -0.5]                      # t0 = t1 = 0: sector 0
    w = exact_weights(n, seed=3, levels=4096)
    want = reference(rows, w, yaw_bins=yaw_bins)
    assert want["occupied"] > 16 * min(yaw_bins, 4)
    got = run(eng, rows, w, yaw_bins=yaw_bins, stride=stride)
    assert_exact(got, want)
    assert (got["top_bin"][:, 3] < yaw_bins).all() and (yaw_bins == 1 or got["top_bin"][:, 3].max() > 0)
    table = capi.yaw_sector_table(yaw_bins)
    assert ref.sectors(*ref.yaw_terms(rows[7:9, 3:]), table).tolist() == [0, 0]


def test_zero_weights_nonfinite_positions_and_top_k(eng):
    ids = np.repeat(np.arange(5), [3, 1, 4, 2, 6])
    rows = rows_of(ids, seed=1)
    w = np.zeros(len(ids), F)
    got = run(eng, rows, w)
    want = reference(rows, w)
    assert (got["occupied"], got["occupied_alive"]) == (5, 0) and want["occupied_alive"] == 0
    assert_exact(got, want)                                             # top_k = 16 > occupied: five rows, ordered by key
    for bin4, _, _, leader in top_rows(got):                            # all weights tie: the lowest index leads
        members = np.nonzero(ref.keys(rows, want["grid"], capi.yaw_sector_table(1)) ==
                             [k for k in want["bins"] if ref.key_parts(k, want["grid"], 1) == bin4][0])[0]
        assert leader == members.min()
    w = exact_weights(len(ids), seed=2, levels=64) + F(2.0 ** -20)
    w[rows[:, 0] == rows[:, 0].min()] = 0                               # one dead bin among live ones
    assert_exact(run(eng, rows, w, top_k=0), reference(rows, w, top_k=0), top_k=0)
    assert run(eng, rows, w)["occupied_alive"] == 4
    assert_exact(run(eng, rows, w, top_k=2), reference(rows, w, top_k=2), top_k=2)
    # non-finite positions: counted, in no bin, and no part of the extent
    bad = rows.copy()
    bad[[0, 5], 0], bad[9, 2] = [np.nan, np.inf], -np.inf
    want = reference(bad, w)
    assert want["nonfinite"] == 3
    got = run(eng, bad, w)
    assert_exact(got, want)
    assert int(got["top_count"].sum()) == len(ids) - 3
    bad[:, 1] = np.nan                                                   # nobody has a position
    got = run(eng, bad, w)
    assert (got["occupied"], got["occupied_alive"], got["nonfinite"], len(got["top_mass"])) == (0, 0, len(ids), 0)


def test_null_outputs(eng):
    rows = rows_of(np.repeat(np.arange(3), 4), seed=4)
    w = exact_weights(12, seed=4, levels=64)
    d_rows, d_w = on_device(rows, w)
    b = np.asarray(BIN, F)
    lib, occupied = eng.lib, C.c_size_t(0)
    args = (eng.h, capi._ptr(d_rows), 7, capi._ptr(d_w), 12, capi._ptr(b), 1)
    assert lib.mcl3dl_hip_particle_bins_device(*args, 16, None, None, None, None, None, None, None, None) == 0
    assert lib.mcl3dl_hip_particle_bins_device(*args, 0, C.byref(occupied), None, None, None, None, None, None, None) == 0
    assert occupied.value == 3
    mass = np.zeros(16, np.float64)
    assert lib.mcl3dl_hip_particle_bins_device(*args, 16, None, None, None, None, capi._ptr(mass), None, None, None) == 0
    assert mass[:3].tolist() == [r[1] for r in reference(rows, w)["top"]] and not mass[3:].any()


def test_bad_arguments_and_an_extent_beyond_the_key_space(eng):
    rows = rows_of(np.arange(10), seed=6)
    w = exact_weights(10, seed=6, levels=64)
    for kwargs in (dict(bin_xyz=(0.5, 0.0, 0.5)), dict(bin_xyz=(0.5, -1.0, 0.5)), dict(yaw_bins=0), dict(yaw_bins=2),
                   dict(yaw_bins=65), dict(top_k=-1), dict(top_k=17), dict(stride=6)):
        with pytest.raises(capi.EngineError, match="error -3"):
            run(eng, rows, w, **kwargs)
    d_rows, d_w = on_device(rows, w)
    with pytest.raises(capi.EngineError, match="error -3"):
        eng.particle_bins_device(d_rows, d_w, 0, BIN)
    far = rows.copy()
    far[3, :3] = [4.0e3, -4.0e3, 4.0e3]
    with pytest.raises(capi.EngineError, match="too small for the particles' extent"):
        run(eng, far, w, bin_xyz=(0.001, 0.001, 0.001), yaw_bins=4)
    with pytest.raises(ref.BinsTooSmall):
        reference(far, w, bin_xyz=(0.001, 0.001, 0.001), yaw_bins=4)
    coarse = (50.0, 50.0, 50.0)                                          # the context works on, and coarser bins fit
    assert_exact(run(eng, far, w, bin_xyz=coarse), reference(far, w, bin_xyz=coarse))
    assert_exact(run(eng, rows, w), reference(rows, w))


# ---- the group form ---------------------------------------------------------------------------------------------------------
def states_of(rows7, seed):
    s = np.random.default_rng(seed).normal(size=(len(rows7), 13)).astype(F)
    s[:, :7] = rows7
    return s


@pytest.mark.parametrize("devices,collective,direct,n", [([0], None, 1, 3001), ([0], None, 0, 3001), ([0, 0, 0], "host", 1, 3001),
                                                        ([0] * 5, "host", 1, 3001), ([0] * 5, "host", 1, 3)],
                         ids=["n1-direct", "n1-rccl", "n3-host", "n5-host", "n5-three"])
def test_group_equals_the_context_form_on_the_concatenated_states(eng, devices, collective, direct, n):
    rng = np.random.default_rng(n)
    rows = rows_of(np.sort(rng.integers(0, 7, n)), seed=n, yaw=True)
    w = exact_weights(n, seed=9, levels=4096)
    if n > 100:
        rows[11, 0], w[::5] = np.nan, 0
    g = capi.Group(devices, collective=collective)
    try:
        g.set_option("direct_single", direct)   # 0: one rank takes the sharded path, its all-gathers over RCCL
        g.upload_state(states_of(rows, 3), w)
        before = g.collective_stats()
        got = g.particle_bins(BIN, yaw_bins=4, top_k=16)
        stats = g.collective_stats()                                    # one voted round, of the group's kind
        assert stats["rccl"] == before["rccl"] + (direct == 0) and stats["host"] == before["host"] + (collective == "host")
        s, w_back = g.download_state()
        want = run(eng, s[:, :7], w_back, yaw_bins=4)
        wide = run(eng, s[:, :7], w_back, yaw_bins=4, stride=13)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
            np.testing.assert_array_equal(wide[k], want[k], err_msg=k)
        assert_exact(got, reference(rows, w, yaw_bins=4))
        assert got["nonfinite"] == (1 if n > 100 else 0)
        for leader, mass in zip(got["top_leader"], got["top_mass"]):    # leaders are global particle indices
            state, weight = g.download_particle(int(leader))
            np.testing.assert_array_equal(state[:7], rows[leader])
            assert weight == w[leader] and weight <= mass
        with pytest.raises(capi.EngineError, match="error -3"):
            g.particle_bins(BIN, yaw_bins=2)
        assert g.particle_bins(BIN, yaw_bins=4, top_k=16)["top_mass"].tobytes() == got["top_mass"].tobytes()
    finally:
        g.close()


def test_group_without_resident_particles():
    g = capi.Group([0])
    try:
        with pytest.raises(capi.EngineError, match="error -5"):
            g.particle_bins(BIN)
    finally:
        g.close()


# ---- end to end: global localisation -> occupied bins -> KLD bound -> resize ---------------------------------------------------------
def test_kld_sized_particle_set_after_global_localization():
    from mcl_3dl_amd.synthetic import make_scene
    map_xyz = make_scene(n=91, n_p=8, n_s=64, n_b=0, seed=31, map_jitter=0.04).map_xyz
    num_particles, div_yaw, bin3 = 64, 4, (2.0, 2.0, 2.0)
    g = capi.Group([0])
    try:
        g.set_map(map_xyz, None, stamp=8100, dist_weight=(1.0, 1.0, 5.0))
        g.set_likelihood_params()
        g.set_beam_params()
        n_points, n = g.global_localization(0.3, div_yaw)
        assert n == n_points * div_yaw == g.resident() and n > 4000
        first = g.particle_bins(bin3, yaw_bins=div_yaw, top_k=16)
        s, w = g.download_state()
        assert_exact(first, reference(s[:, :7], w, bin_xyz=bin3, yaw_bins=div_yaw))
        assert first["occupied"] == first["occupied_alive"] > 16 and first["nonfinite"] == 0
        n_kld = capi.kld_bound(first["occupied"], 0.05, 2.326)
        target = max(num_particles, min(int(n * 0.75), n_kld))             # the node's clamp around the bound
        assert num_particles < target == n_kld < int(n * 0.75)              # the bound, not the fixed factor, sizes the set
        g.resize_resident(target)
        assert g.resident() == target
        second = g.particle_bins(bin3, yaw_bins=div_yaw, top_k=16)
        s, w = g.download_state()
        assert_exact(second, reference(s[:, :7], w, bin_xyz=bin3, yaw_bins=div_yaw))
        assert 0 < second["occupied"] <= first["occupied"]
        state, _ = g.download_particle(int(second["top_leader"][0]))        # a hypothesis, read from its leader
        assert np.isfinite(state).all()
    finally:
        g.close()
