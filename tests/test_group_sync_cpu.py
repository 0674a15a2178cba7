"""CPU test of the device group's thread synchronisation (tests/cpp/group_sync_check.cpp, a stand-alone program over
mcl_3dl_amd/csrc/host_group_sync.h: WorkerPool, VoteBarrier and run_round, the round by which the ranks enter a collective
together or not at all). Fake ranks, counters in place of GPU work, N = 1, 2, 3, 5: all ranks ok; each rank failing at the first
and at the second vote; two at once; 2000 rounds back to back; rounds behind a pause that sends the workers to sleep. Built three
times — optimised, ThreadSanitizer, AddressSanitizer + UndefinedBehaviorSanitizer — each a plain executable."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TRIVIAL = """
#include <atomic>
#include <thread>
int main() { std::atomic<int> n{0}; std::thread t([&] { ++n; }); t.join(); return n.load() == 1 ? 0 : 1; }
"""


def build(cxx, flags, src, exe):
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", *flags, "-I", os.path.join(ROOT, "mcl_3dl_amd", "csrc"),
                    "-o", exe, src], check=True)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=thread", "-g"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "tsan", "asan_ubsan"])
def test_ranks_enter_a_collective_together_or_not_at_all(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    if "-fsanitize=thread" in flags:
        # ThreadSanitizer cannot start everywhere (it maps fixed address ranges): skipped only where a trivial two-thread
        # program built the same way does not start either
        src = tmp_path / "trivial.cpp"
        src.write_text(TRIVIAL)
        trivial = str(tmp_path / "trivial.bin")
        build(cxx, flags, str(src), trivial)
        probe = subprocess.run([trivial], capture_output=True, text=True, timeout=120)
        if probe.returncode != 0:
            print(probe.stdout + probe.stderr)
            pytest.skip("ThreadSanitizer does not start here: " + (probe.stdout + probe.stderr).strip()[-400:])
    exe = str(tmp_path / "group_sync_check.bin")
    build(cxx, flags, os.path.join(HERE, "cpp", "group_sync_check.cpp"), exe)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count(": ok") == 4
