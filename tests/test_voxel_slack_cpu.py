"""CPU test of the likelihood indices' geometry (tests/cpp/voxel_slack_check.cpp, a stand-alone program over
mcl_3dl_amd/csrc/index_geometry.h): on every grid the header lays out — five radii, three voxel ratios, cubes and stretched
voxels, three origins, 20 m to 5 km — every float within 8 floats of a voxel face lies inside the grown box V+ of the voxel the
kernels' float expression gives it (the premise of the candidate index's exactness proof, map_compiler.h), and two coordinates
closer than the radius get adjacent cells of the map's cell grid (the premise of the 27-cell scan). Built plain and with
AddressSanitizer + UndefinedBehaviorSanitizer, each a plain executable. The same sweep with the slack fixed at 1e-3 of a voxel
edge — the engine's rule before the slack was derived from the voxel count — must fail, for every radius up to 0.3 m, on the
grids of 1.1 km and longer: the sweep finds what it is there to find."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(flags, exe):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mcl_3dl_amd", "csrc"),
                    "-o", exe, os.path.join(HERE, "cpp", "voxel_slack_check.cpp")], check=True)
    return exe


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_every_float_lies_in_the_grown_box_of_its_voxel(tmp_path, flags):
    exe = build(flags, str(tmp_path / "voxel_slack_check.bin"))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.count("every float inside the V+ of its voxel") == 5
    assert run.stdout.count("every pair closer than r within one cell") == 5
    m = re.search(r"candidate grids: (\d+), refused (\d+), failing 0; cell grids: (\d+), refused (\d+), failing 0", run.stdout)
    assert m, run.stdout[-2000:]
    grids, refused, cell_grids, cell_refused = map(int, m.groups())
    # 5 radii x 3 ratios x 2 shapes x 3 origins x 5 extents x 2 long axes; only the finest voxels on the longest grids are refused
    assert grids == 900 and cell_grids == 150 and refused < grids // 10 and cell_refused < cell_grids // 5


def test_the_sweep_fails_on_a_slack_that_ignores_the_voxel_count(tmp_path):
    exe = build([], str(tmp_path / "voxel_slack_check.bin"))
    run = subprocess.run([exe, "--fixed-slack"], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 1 and "CHECKS FAILED" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    for r in ("0.05", "0.1", "0.2", "0.3"):
        assert re.search(r"^r %s: first float outside the V\+ of its voxel at face \d+ " % re.escape(r), run.stdout, re.M), r
        m = re.search(r"^r %s: grids with floats outside V\+ are ([\d ]+) m long" % re.escape(r), run.stdout, re.M)
        assert m, (r, run.stdout[-2000:])
        assert {1100, 2200, 5000} <= set(map(int, m.group(1).split())), m.group(0)


def test_the_long_map_cases_hold_their_triples():
    """tests/long_map_cases.py on the CPU: every variant yields at least 64 constructed triples (the generator asserts their
    properties in fp64), within the 12 000 points a map may have, on a grid long enough for the derived slack to matter."""
    import long_map_cases as cases
    for name in cases.VARIANTS:
        c = cases.make_case(name)
        assert cases.MIN_TRIPLES <= len(c["triples_q"]) <= cases.MAX_TRIPLES and len(c["map_xyz"]) <= 12000, name
        assert c["triples_rel"].min() >= 1e-6
        assert c["geom"]["voxels"].max() > 20000 and c["geom"]["grow"] > 2.0 * c["geom"]["grow_fixed"], name
        q = cases.face_queries(c, c["geom"])
        assert q.shape == (2000, 3) and q.dtype == np.float32 and np.isfinite(q).all()
