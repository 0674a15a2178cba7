"""CPU tests of the cloud accumulation's arithmetic and surface (mcl_3dl_amd/csrc/scan_accum.h, include/mcl3dl_hip.h):
tests/scan_accum_ref.py — the yardstick of tests/test_gpu_scan_accum.py — against float64 within the stated bound and against the
header's own expression compiled for the host, and the new entry points declared, exported and bound."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import scan_accum_ref as sar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

NAMES = ["mcl3dl_hip_scan_accum_clear", "mcl3dl_hip_scan_accum_push", "mcl3dl_hip_scan_accum_push_pointcloud2",
         "mcl3dl_hip_scan_accum_size", "mcl3dl_hip_scan_accum_download", "mcl3dl_hip_scan_begin_accumulated",
         "mcl3dl_hip_group_scan_accum_clear", "mcl3dl_hip_group_scan_accum_push",
         "mcl3dl_hip_group_scan_accum_push_pointcloud2", "mcl3dl_hip_group_scan_accum_size",
         "mcl3dl_hip_group_scan_begin_accumulated"]


@pytest.fixture(scope="module")
def fixture():
    """Rotations about every axis and about all at once, translations from nothing to 2 km; points of a LiDAR's range, some on
    the axes, some tiny, some exactly zero."""
    rng = np.random.default_rng(2718)
    mats = [sar.rigid((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
            sar.rigid((0.7, 0.0, 0.0), (1.0, -2.0, 0.5)),
            sar.rigid((0.0, -1.1, 0.0), (-150.0, 80.0, 3.0)),
            sar.rigid((0.0, 0.0, 2.9), (2000.0, -2000.0, 31.0)),
            sar.rigid((0.3, -0.2, 1.7), (-1987.25, 1234.5, -12.0)),
            sar.rigid((3.1, 1.5, -3.0), (0.001, 2000.0, 0.0))]
    pts = rng.uniform(-100.0, 100.0, (100000, 3)).astype(F)
    pts[:1000] *= F(1e-3)
    pts[1000:1100, 1:] = 0.0
    pts[1100:1200, ::2] = 0.0
    pts[1200] = 0.0
    return mats, pts


def test_restatement_stays_inside_the_gamma4_bound(fixture):
    mats, pts = fixture
    worst = 0.0
    for m in mats:
        got = sar.affine_apply(m, pts).astype(np.float64)
        exact, bound, scale = sar.affine_bound(m, pts)
        # (`exact` is a float64 evaluation: its own error, at most gamma_4 at 2^-53 of the same scale, is added to the bound)
        err = np.abs(got - exact)
        assert np.all(err <= bound + 4 * 2.0 ** -53 * scale)
        worst = max(worst, float(np.max(err / np.maximum(scale, 1e-300))) / sar.U)
    print("largest error: %.2f u S (bound %.2f u S)" % (worst, sar.GAMMA4 / sar.U))
    assert worst > 0.5   # (the fixture does exercise the roundings)


def test_null_matrix_copies_bits_and_transforms_are_not_composed(fixture):
    mats, pts = fixture
    odd = pts[:8].copy()
    odd[0, 0], odd[1, 1], odd[2, 2] = np.nan, np.inf, -0.0
    np.testing.assert_array_equal(sar.affine_apply(None, odd).view(np.uint32), odd.view(np.uint32))
    clouds = [pts[:1000], pts[1000:1300], pts[1300:1301]]
    xyz, lab = sar.accumulate(clouds, [mats[3], None, mats[4]])
    assert xyz.dtype == F and len(xyz) == 1301
    np.testing.assert_array_equal(lab, np.repeat(np.arange(3, dtype=np.uint32), [1000, 300, 1]))
    np.testing.assert_array_equal(xyz[1000:1300], pts[1000:1300])
    # the stored floats are what the second transform reads: the composed matrix gives other bits at 2 km
    base = sar.to_base(xyz[:1000], mats[4])
    m1, m2 = (np.vstack([m.astype(np.float64), [0, 0, 0, 1]]) for m in (mats[3], mats[4]))
    composed = sar.affine_apply((m2 @ m1)[:3].astype(F), pts[:1000])
    assert np.count_nonzero(base != composed) > 100


def test_restatement_equals_the_header_compiled_for_the_host(fixture, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "scan_accum_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "mcl_3dl_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "scan_accum_check.cpp")], check=True)
    mats, pts = fixture
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([len(mats), len(pts)], np.uint32).tofile(f)
        np.stack(mats).astype(F).tofile(f)
        pts.tofile(f)
    subprocess.run([exe, src, dst], check=True, timeout=120)
    got = np.fromfile(dst, F).reshape(len(mats), len(pts), 3)
    for k, m in enumerate(mats):
        np.testing.assert_array_equal(got[k].view(np.uint32), sar.affine_apply(m, pts).view(np.uint32))


def test_pointcloud2_packer_round_trips():
    pts = np.arange(15, dtype=F).reshape(5, 3) - F(6.5)
    raw = np.frombuffer(sar.pack_pointcloud2(pts, 22, 2, 10, 6), np.uint8).reshape(5, 22)
    for k, off in enumerate((2, 10, 6)):
        np.testing.assert_array_equal(raw[:, off:off + 4].copy().view("<f4")[:, 0], pts[:, k])
    assert np.all(raw[:, :2] == 0xA5) and np.all(raw[:, 14:] == 0xA5)


def test_entry_points_are_declared_exported_and_bound():
    """The test of this file that needs the feature: header, library and binding name every new entry point."""
    from mcl_3dl_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcl3dl_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcl3dl_hip_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
    for cls in (capi.Engine, capi.Group):
        for method in ("scan_accum_clear", "scan_accum_push", "scan_accum_push_pointcloud2", "scan_accum_size",
                       "scan_begin_accumulated"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
    assert callable(capi.Engine.scan_accum_download) and not hasattr(capi.Group, "scan_accum_download")
    assert capi.load_library().mcl3dl_hip_abi_version() == 3
