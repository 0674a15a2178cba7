"""How a device group splits n particles over its ranks (mcl_3dl_amd/csrc/shard_layout.h), compiled for the host
(tests/cpp/shard_layout_check.cpp): the bounds of every rank, the largest shard and the inverse map particle -> (rank, offset)
that the unpad kernel behind the padded all-gather runs — for every world size a group accepts (1..64, ROUND_MAX_RANKS of
host_group_sync.h) and every n in 0..300, which covers empty shards (n < world, where n // world is 0), equal shards and shards
one apart; and the first and last particle of every rank at the largest n a group takes. Yardsticks: the shards tile [0, n);
mcl_3dl_amd/distributed.py:shard_bounds; the inverse read off the bounds by a sorted search, not by the header's arithmetic.
The program is built a second time with the address and undefined-behaviour sanitizers and run on the same inputs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mcl_3dl_amd.distributed import shard_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD_MAX, N_MAX = 64, 300
N_LARGEST = 0x7fffffff // 16          # what mcl3dl_hip_group_upload_state accepts
EDGE_WORLDS = (1, 7, 64)


def build(tmp, extra=()):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp / ("shard_layout_check" + ("_san" if extra else "")))
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "mcl_3dl_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "shard_layout_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("shard_layout")


@pytest.fixture(scope="module")
def exe(workdir):
    return build(workdir)


def run(exe, workdir, mode, a, b):
    dst = str(workdir / ("%s_%d_%d.out" % (mode, a, b)))
    subprocess.run([exe, mode, str(a), str(b), dst], check=True, timeout=120)
    return np.fromfile(dst, np.uint32 if mode == "sweep" else np.uint64).astype(np.int64)


def bounds(n, world):
    """[lo], [hi] of every rank from distributed.shard_bounds, checked to tile [0, n) with sizes at most one apart"""
    lo, hi = (np.array(v, np.int64) for v in zip(*[shard_bounds(n, world, r) for r in range(world)]))
    assert lo[0] == 0 and hi[-1] == n and np.array_equal(lo[1:], hi[:-1])
    size = hi - lo
    assert size.max() - size.min() <= 1 and np.all(np.diff(size) <= 0)
    return lo, hi


@pytest.fixture(scope="module")
def sweep_expected():
    words = []
    for world in range(1, WORLD_MAX + 1):
        for n in range(N_MAX + 1):
            lo, hi = bounds(n, world)
            i = np.arange(n, dtype=np.int64)
            rank = np.searchsorted(hi, i, side="right")       # the rank whose [lo, hi) holds i
            offset = i - lo[rank]
            assert np.all((lo[rank] <= i) & (i < hi[rank]))
            cap = int((hi - lo).max())
            assert np.all(offset < cap)
            words += [[cap], np.stack([lo, hi], 1).reshape(-1), np.stack([rank, offset], 1).reshape(-1)]
    return np.concatenate([np.asarray(w, np.int64) for w in words])


def edges_expected(world):
    lo, hi = bounds(N_LARGEST, world)
    rec = [[int((hi - lo).max())]]
    for r in range(world):
        rec.append([lo[r], hi[r], r, 0, r, hi[r] - lo[r] - 1])
    return np.concatenate([np.asarray(w, np.int64) for w in rec])


def test_bounds_capacity_and_inverse_map_for_every_world_size(exe, workdir, sweep_expected):
    np.testing.assert_array_equal(run(exe, workdir, "sweep", WORLD_MAX, N_MAX), sweep_expected)


@pytest.mark.parametrize("world", EDGE_WORLDS)
def test_shard_edges_at_the_largest_particle_count(exe, workdir, world):
    np.testing.assert_array_equal(run(exe, workdir, "edges", N_LARGEST, world), edges_expected(world))


def test_sanitized_build_runs_clean_on_the_same_inputs(workdir, sweep_expected):
    san = build(workdir, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    np.testing.assert_array_equal(run(san, workdir, "sweep", WORLD_MAX, N_MAX), sweep_expected)
    for world in EDGE_WORLDS:
        np.testing.assert_array_equal(run(san, workdir, "edges", N_LARGEST, world), edges_expected(world))
