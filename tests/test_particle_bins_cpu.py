"""CPU tests of the occupied-bin statistic: the two pure host functions of the C ABI, the header's scalar
arithmetic compiled with g++ and held against tests/particle_bins_ref.py bit for bit, and the binding's marshalling against a
recording stand-in. The device pipeline is tests/test_gpu_particle_bins.py's."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import particle_bins_ref as ref
from mcl_3dl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- mcl3dl_hip_kld_bound ------------------------------------------------------------------------------------------------------
def kld_clear_of_an_integer(k, eps, z):
    """The exact value lies farther than 1e-9 (relative) from an integer: rounding in the double evaluation cannot move the ceil."""
    value, _ = ref.kld_bound_exact(k, eps, z, digits=50)
    return abs(value - value.to_integral_value()) / value > 1e-9


KLD_ALL = [(k, eps, z) for k in (2, 3, 10, 1000, 10 ** 6) for eps in (0.01, 0.05) for z in (0.99, 2.326)]
# decided by the reference computation alone, never by the code under test: 18 of the 20 combinations; (10^6, 0.01, 2.326) =
# 50164569.957... and (10^6, 0.05, 2.326) = 10032913.991... lie 8.6e-10 from an integer
KLD_CASES = [c for c in KLD_ALL if kld_clear_of_an_integer(*c)]


def test_kld_cases_are_nearly_all_combinations():
    assert len(KLD_CASES) == 18


@pytest.mark.parametrize("k,eps,z", KLD_CASES)
def test_kld_bound_is_the_formula_in_exact_arithmetic(k, eps, z):
    value, want = ref.kld_bound_exact(k, eps, z, digits=50)
    # asserted for the reference's own value, so that the comparison below cannot hide a disagreement about the ceil
    assert abs(value - value.to_integral_value()) / value > 1e-9, (k, eps, z, value)
    assert capi.kld_bound(k, eps, z) == want


@pytest.mark.parametrize("k,eps,z", [c for c in KLD_ALL if c not in KLD_CASES])
def test_kld_bound_next_to_an_integer_is_off_by_one_at_most(k, eps, z):
    _, want = ref.kld_bound_exact(k, eps, z, digits=50)
    assert abs(capi.kld_bound(k, eps, z) - want) <= 1


def test_kld_bound_edges():
    assert capi.kld_bound(0, 0.05, 2.326) == 1 and capi.kld_bound(1, 0.05, 2.326) == 1
    for z in (0.99, 2.326):
        got = [capi.kld_bound(k, 0.05, z) for k in range(1, 400)]
        assert all(b >= a for a, b in zip(got, got[1:])), z
        assert got[-1] > got[1] > 1
    lib = capi.load_library()
    n = C.c_size_t(77)
    for k, eps, z in ((10, 0.0, 1.0), (10, -0.1, 1.0), (10, 1.5, 1.0), (10, float("nan"), 1.0), (10, 0.05, float("inf")),
                      (10, 0.05, float("nan")), (2 ** 62, 0.01, 2.326)):
        assert lib.mcl3dl_hip_kld_bound(k, eps, z, C.byref(n)) == -3, (k, eps, z)
        assert n.value == 77
        with pytest.raises(ValueError):
            capi.kld_bound(k, eps, z)
    assert lib.mcl3dl_hip_kld_bound(10, 1.0, 0.0, C.byref(n)) == 0 and n.value >= 1   # epsilon = 1 is inside (0, 1]
    assert lib.mcl3dl_hip_kld_bound(10, 0.05, 2.0, None) == -3


# ---- mcl3dl_hip_yaw_sector_table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw_bins", [1, 3, 4, 64])
def test_yaw_sector_table(yaw_bins):
    t = capi.yaw_sector_table(yaw_bins)
    assert t.shape == (yaw_bins, 2) and t.dtype == np.float64
    assert t[0, 0] == 1.0 and t[0, 1] == 0.0
    assert np.abs(np.hypot(t[:, 0], t[:, 1]) - 1.0).max() <= 1e-15
    angle = 2.0 * np.pi * np.arange(yaw_bins) / yaw_bins
    assert np.abs(t[:, 0] - np.cos(angle)).max() <= 2e-16 and np.abs(t[:, 1] - np.sin(angle)).max() <= 2e-16
    if yaw_bins == 4:   # the quarter turns are exact
        assert t.tolist() == [[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]]


@pytest.mark.parametrize("yaw_bins", [0, 2, 65, -1])
def test_yaw_sector_table_refuses(yaw_bins):
    lib = capi.load_library()
    buf = np.full(200, 7.0)
    assert lib.mcl3dl_hip_yaw_sector_table(yaw_bins, buf.ctypes.data_as(C.c_void_p)) == -3
    assert (buf == 7.0).all()
    with pytest.raises(ValueError):
        capi.yaw_sector_table(yaw_bins)


# ---- the header's arithmetic on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header_check(tmp_path_factory):
    """check(rows7, bin_xyz, yaw_bins) -> (finite, parts (n, 3), sector, key, the header's own table) from particle_bins_check."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("particle_bins")
    exe = str(tmp / "particle_bins_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "mcl_3dl_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "particle_bins_check.cpp")], check=True)

    def check(rows7, bin_xyz, yaw_bins, table):
        rows7 = np.ascontiguousarray(rows7, np.float32).reshape(-1, 7)
        _, min_b, div = ref.make_grid(rows7[:, :3], bin_xyz, yaw_bins)
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as f:
            np.array([len(rows7), yaw_bins], np.int32).tofile(f)
            np.asarray(bin_xyz, np.float32).tofile(f)
            min_b.astype(np.int32).tofile(f)
            div.astype(np.uint32).tofile(f)
            np.ascontiguousarray(table, np.float64).tofile(f)
            rows7.tofile(f)
        subprocess.run([exe, src, dst], check=True, timeout=120)
        raw = np.fromfile(dst, np.uint8)
        rec = raw[:24 * len(rows7)].view(np.int32).reshape(-1, 6)
        own = raw[24 * len(rows7):].view(np.float64).reshape(-1, 2)
        return rec[:, 0].astype(bool), rec[:, 1:4], rec[:, 4], rec[:, 5].view(np.uint32).reshape(-1), own
    return check


def random_rows(n, seed, span=20.0):
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 7), np.float32)
    rows[:, :3] = rng.uniform(-span, span, (n, 3))
    q = rng.normal(size=(n, 4))
    rows[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return rows


def special_rows(bin_xyz):
    """Negative coordinates, coordinates exactly on bin edges, t0 = t1 = 0, a NaN quaternion, a non-finite position, the four
    axis-aligned headings from exact halves."""
    b = np.asarray(bin_xyz, np.float32)
    rows = []
    for k in (-7, -1, 0, 1, 2, 5, 33):   # on the edges, and an ulp either side of them
        edge = (np.float32(k) * b).astype(np.float32)
        for p in (edge, np.nextafter(edge, np.float32(-np.inf)), np.nextafter(edge, np.float32(np.inf))):
            rows.append(list(p) + [0, 0, 0, 1])
    rows.append([-3.25, -0.125, -9.5, 0, 0, 0, 1])
    rows.append([1, 2, 3, 0.5, 0.5, 0.5, -0.5])                 # x y + w z = 0 and 1 - 2 (y^2 + z^2) = 0: t0 = t1 = 0
    rows.append([1, 2, 3, np.nan, 0, 0, 1])
    rows.append([1, 2, 3, 0, np.nan, np.nan, np.nan])
    rows.append([np.nan, 2, 3, 0, 0, 0, 1])
    rows.append([1, np.inf, 3, 0, 0, 0, 1])
    rows += [[0, 0, 0] + q for q in AXIS_QUATS]
    return np.array(rows, np.float32)


# headings of exactly 0, 90, 180 and 270 degrees: every product in getRPY's t0 / t1 is a multiple of a quarter
AXIS_QUATS = [[0, 0, 0, 1], [0.5, 0.5, 0.5, 0.5], [0, 0, 1, 0], [0.5, -0.5, -0.5, 0.5]]


@pytest.mark.parametrize("bin_xyz,yaw_bins", [((0.3, 0.3, 0.3), 4), ((0.5, 0.25, 1.0), 36), ((0.3, 0.7, 0.11), 1),
                                              ((2.0, 2.0, 2.0), 3), ((0.05, 0.05, 5.0), 64)])
def test_header_arithmetic_is_the_references(header_check, bin_xyz, yaw_bins):
    rows = np.vstack([random_rows(12000, 5 + yaw_bins), special_rows(bin_xyz)])
    table = capi.yaw_sector_table(yaw_bins)
    finite, parts, sector, key, own_table = header_check(rows, bin_xyz, yaw_bins, table)
    assert own_table.tobytes() == table.tobytes()   # the library hands out the header's table
    grid = ref.make_grid(rows[:, :3], bin_xyz, yaw_bins)
    want_finite = ref.finite_rows(rows[:, :3])
    np.testing.assert_array_equal(finite, want_finite)
    assert (~want_finite).sum() == 2
    np.testing.assert_array_equal(parts[want_finite], ref.axis_bins(rows[:, :3], grid[0], grid[1])[want_finite])
    np.testing.assert_array_equal(sector, ref.sectors(*ref.yaw_terms(rows[:, 3:]), table))
    np.testing.assert_array_equal(key, ref.keys(rows, grid, table))
    assert (parts[want_finite] >= 0).all() and (parts[want_finite] < grid[2]).all()
    assert (sector >= 0).all() and (sector < yaw_bins).all()
    if yaw_bins > 1:
        assert len(np.unique(sector)) == yaw_bins


def test_sectors_on_the_boundaries_and_without_a_heading(header_check):
    bin_xyz = (0.3, 0.3, 0.3)
    table = capi.yaw_sector_table(4)
    rows = special_rows(bin_xyz)
    _, _, sector, _, _ = header_check(rows, bin_xyz, 4, table)
    assert sector[-4:].tolist() == [0, 1, 2, 3]       # a heading ON a boundary opens its sector
    t0, t1 = ref.yaw_terms(rows[:, 3:])
    degenerate = (t0 == 0) & (t1 == 0)
    assert degenerate.sum() == 1 and (sector[degenerate] == 0).all()
    without = np.isnan(t0) | np.isnan(t1)
    assert (sector[without] == 0).all() and without.sum() == 2
    # the sector follows atan2 wherever the heading is not within rounding of a boundary
    rnd = random_rows(4000, 11)
    for yaw_bins in (3, 4, 36, 64):
        tab = capi.yaw_sector_table(yaw_bins)
        _, _, sec, _, _ = header_check(rnd, bin_xyz, yaw_bins, tab)
        r0, r1 = ref.yaw_terms(rnd[:, 3:])
        turn = np.mod(np.arctan2(r1.astype(np.float64), r0.astype(np.float64)), 2 * np.pi) / (2 * np.pi) * yaw_bins
        clear = np.abs(turn - np.round(turn)) > 1e-6
        assert clear.sum() > 3900
        np.testing.assert_array_equal(sec[clear], np.floor(turn[clear]).astype(np.int32))


def test_reference_statistic_on_a_case_worked_by_hand():
    table = capi.yaw_sector_table(4)
    rows = np.array([[0.1, 0.1, 0.1] + AXIS_QUATS[0], [0.2, 0.2, 0.2] + AXIS_QUATS[0], [0.1, 0.1, 0.1] + AXIS_QUATS[1],
                     [-0.9, 0.1, 0.1] + AXIS_QUATS[0], [np.nan, 0, 0] + AXIS_QUATS[0]], np.float32)
    w = np.array([0.25, 0.5, 0.125, 0.0, 9.0], np.float32)
    got = ref.bins(rows, w, (1.0, 1.0, 1.0), 4, table, top_k=16)
    assert (got["occupied"], got["occupied_alive"], got["nonfinite"]) == (3, 2, 1)
    assert got["top"] == [([0, 0, 0, 0], 0.75, 2, 1), ([0, 0, 0, 1], 0.125, 1, 2), ([-1, 0, 0, 0], 0.0, 1, 3)]
    with pytest.raises(ref.BinsTooSmall):
        ref.make_grid(np.array([[0, 0, 0], [1e6, 1e6, 1e6]], np.float32), (0.01, 0.01, 0.01), 4)


# ---- the binding's marshalling -------------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for the library: logs (symbol, arguments), answers 0 — or what `returns` names — and writes `writes` into the
    size_t words and arrays it is handed, as the library would."""

    def __init__(self, returns=None, writes=None):
        self.log, self.returns, self.writes = [], returns or {}, writes

    def __getattr__(self, symbol):
        if symbol.startswith("__"):
            raise AttributeError(symbol)

        def call(*args):
            self.log.append((symbol, args))
            if self.writes and symbol in self.writes:
                self.writes[symbol](args)
            return self.returns.get(symbol, 0)
        return call


@pytest.fixture
def plain_ptr(monkeypatch):
    monkeypatch.setattr(capi, "_ptr", lambda a: a)   # the log sees the arrays themselves


def fill_outputs(args):
    """What the library writes behind the eight output arguments: 5 occupied, 4 alive, 1 non-finite, two top rows."""
    occupied, alive, nonfinite, bin4, mass, count, leader, top_n = args[-8:]
    k = min(2, len(mass))
    occupied._obj.value, alive._obj.value, nonfinite._obj.value, top_n._obj.value = 5, 4, 1, k
    if k:
        bin4[:k] = [[1, -2, 3, 0], [4, 5, -6, 7]][:k]
        mass[:k], count[:k], leader[:k] = [0.5, 0.25][:k], [10, 20][:k], [7, 9][:k]


def check_result(out):
    assert {k: v for k, v in out.items() if not k.startswith("top_")} == dict(occupied=5, occupied_alive=4, nonfinite=1)
    assert out["top_bin"].tolist() == [[1, -2, 3, 0], [4, 5, -6, 7]] and out["top_bin"].dtype == np.int32
    assert out["top_mass"].tolist() == [0.5, 0.25] and out["top_mass"].dtype == np.float64
    assert out["top_count"].tolist() == [10, 20] and out["top_leader"].tolist() == [7, 9]
    assert out["top_count"].dtype == out["top_leader"].dtype == np.uint32


def check_outputs(args, top_k):
    occupied, alive, nonfinite, bin4, mass, count, leader, top_n = args
    for word in (occupied, alive, nonfinite, top_n):
        assert isinstance(word._obj, C.c_size_t)
    assert bin4.shape == (top_k, 4) and bin4.dtype == np.int32 and bin4.flags.c_contiguous
    assert mass.shape == (top_k,) and mass.dtype == np.float64
    assert count.shape == leader.shape == (top_k,) and count.dtype == leader.dtype == np.uint32


def test_group_particle_bins_marshalling(plain_ptr):
    g = capi.Group.__new__(capi.Group)
    g.lib, g.h = Recorder(writes={"mcl3dl_hip_group_particle_bins": fill_outputs}), C.c_void_p(1)
    try:
        out = g.particle_bins(np.float64([0.5, 0.25, 1.0]), yaw_bins=36.0, top_k=3)
        (symbol, args), = g.lib.log
        assert symbol == "mcl3dl_hip_group_particle_bins" and len(args) == len(capi.SIGNATURES[symbol][1]) == 12
        assert args[0] is g.h and args[1].dtype == np.float32 and args[1].tolist() == [0.5, 0.25, 1.0]
        assert args[2:4] == (36, 3) and all(type(a) is int for a in args[2:4])
        check_outputs(args[4:], 3)
        check_result(out)
        g.lib.log.clear()
        out = g.particle_bins([1, 1, 1])                              # the defaults: one sector, no top rows
        (_, args), = g.lib.log
        assert args[2:4] == (1, 0)
        check_outputs(args[4:], 0)
        with pytest.raises(ValueError):
            g.particle_bins([1, 1])
        g.lib.returns = {"mcl3dl_hip_group_particle_bins": -3, "mcl3dl_hip_group_last_error": b"too small"}
        with pytest.raises(capi.EngineError, match="group error -3: too small"):
            g.particle_bins([1, 1, 1])
    finally:
        g.h = None


def test_engine_particle_bins_device_marshalling(plain_ptr):
    e = capi.Engine.__new__(capi.Engine)
    e.lib, e.h = Recorder(writes={"mcl3dl_hip_particle_bins_device": fill_outputs}), C.c_void_p(1)
    try:
        out = e.particle_bins_device(1234, 5678, 9.0, (0.5, 0.5, 0.5), yaw_bins=4, top_k=16, row_stride=13)
        (symbol, args), = e.lib.log
        assert symbol == "mcl3dl_hip_particle_bins_device" and len(args) == len(capi.SIGNATURES[symbol][1]) == 16
        assert args[0] is e.h and args[1:5] == (1234, 13, 5678, 9) and type(args[4]) is int
        assert args[5].dtype == np.float32 and args[5].tolist() == [0.5, 0.5, 0.5] and args[6:8] == (4, 16)
        check_outputs(args[8:], 16)
        check_result(out)
        e.lib.log.clear()
        e.particle_bins_device(1, 2, 3, [1, 2, 3])
        (_, args), = e.lib.log
        assert args[2] == 7 and args[6:8] == (1, 0)                    # pose rows, one sector, no top rows
        with pytest.raises(ValueError):
            e.particle_bins_device(1, 2, 3, [1, 2, 3, 4])
    finally:
        e.h = None


def test_module_functions_marshalling(monkeypatch, plain_ptr):
    lib = Recorder()
    monkeypatch.setattr(capi, "load_library", lambda: lib)
    t = capi.yaw_sector_table(36.0)
    n = capi.kld_bound(12.0, 0.05, 2)
    (s0, a0), (s1, a1) = lib.log
    assert s0 == "mcl3dl_hip_yaw_sector_table" and a0[0] == 36 and a0[1] is t and t.shape == (36, 2)
    assert s1 == "mcl3dl_hip_kld_bound" and a1[:3] == (12, 0.05, 2.0) and isinstance(a1[3]._obj, C.c_size_t) and n == 0
    assert type(a1[0]) is int and type(a1[2]) is float
    with pytest.raises(ValueError):
        capi.kld_bound(-1, 0.05, 2.0)
    assert len(lib.log) == 2                                           # a negative k never reaches the size_t argument


def test_signatures_and_mirrored_stay_apart():
    for name in ("yaw_sector_table", "kld_bound", "particle_bins_device", "group_particle_bins"):
        assert "mcl3dl_hip_" + name in capi.SIGNATURES
    assert "particle_bins" not in capi.MIRRORED and len(capi.MIRRORED) == 24
    assert math.isfinite(capi.kld_bound(100, 0.05, 2.326))
