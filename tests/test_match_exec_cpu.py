"""CPU test of the implication behind the tiled likelihood kernel's specialised pose loop (tests/cpp/match_exec_check.cpp, a
stand-alone program over mcl_3dl_amd/csrc/host_options.h:lik_match_from_radius): for every accepted (r, flat) and every float
d2 below r2 the reference's dist is non-negative, so `matched` is the radius test. Built twice: optimised, and with
AddressSanitizer + UndefinedBehaviorSanitizer as a plain executable."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_matched_follows_from_the_radius_test(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "match_exec_check.bin")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fno-math-errno", "-Wall", "-Werror", "-pthread", *flags,
                    "-I", os.path.join(ROOT, "mcl_3dl_amd", "csrc"), "-o", exe, os.path.join(HERE, "cpp", "match_exec_check.cpp")],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(run.stdout)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count("accepted 1") == 5 and run.stdout.count(", 0 with dist < 0") == 5
