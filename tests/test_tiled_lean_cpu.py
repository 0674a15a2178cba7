"""CPU test of the tiled likelihood kernel's term slots (tests/cpp/tiled_lean_check.cpp, a stand-alone program over
mcl_3dl_amd/csrc/term_slots.h — the header the kernel includes): the slot mapping is a bijection that hands each fp64 reader its
terms in the order it has always added them, stores stay on 32 distinct banks per half wavefront and every 16-byte read is
conflict-free within its lane group. Built twice — optimised, and with AddressSanitizer + UndefinedBehaviorSanitizer — each a
plain executable."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_term_slots(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "tiled_lean_check.bin")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mcl_3dl_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "cpp", "tiled_lean_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count("term slots G = ") == 3
