"""Reference side of the device-drawn normal-weighted sampler (mcl_3dl_amd/csrc/rng_weighted.h, double_chain.h,
rng_weighted_kernels.h): the door to tests/cpp/rng_weighted_emul.cpp, which holds the standard library's own loop
(std::default_random_engine, std::uniform_real_distribution<double>, std::lower_bound, std::unordered_set<size_t>), the plain
cumulative recurrence, the test inputs, and the CPU replay of the chain and of both kernel forms."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SINGLE_MAX = 1109          # rng_weighted.h: WEIGHTED_SINGLE_MAX, the most ids per model the one-work-group kernel serves
MAX_TOTAL = 2.0 ** 50      # rng_weighted.h: WEIGHTED_MAX_TOTAL
KINDS = ("ones", "rand", "ties", "big", "neg", "special")
LENGTHS = (1, 63, 64, 511, 512, 513, 70000)

_exe = None
_count = 0


def emul_exe(extra_flags=()):
    """tests/cpp/rng_weighted_emul.cpp, compiled once per process into a temporary directory (extra_flags: a build of its own)."""
    global _exe
    if _exe is not None and not extra_flags:
        return _exe
    import atexit
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="rng_weighted_emul_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "rng_weighted_emul.bin")
    subprocess.run(["g++", "-O2", *extra_flags, "-o", exe, os.path.join(HERE, "cpp", "rng_weighted_emul.cpp")], check=True)
    if not extra_flags:
        _exe = exe
    return exe


def _tmp(name):
    global _count
    _count += 1
    return os.path.join(os.path.dirname(emul_exe()), "%s_%d_%d.bin" % (name, os.getpid(), _count))


def _run(*args):
    return subprocess.run([emul_exe(), *[str(a) for a in args]], check=True, capture_output=True, text=True, timeout=300).stdout


def weights(kind, n, seed=None):
    """The emulator's test input `kind` of n float64 weights (seed: the selftest's own is n)."""
    out = _tmp("w")
    _run("weights", kind, int(n), int(n if seed is None else seed), out)
    w = np.fromfile(out, np.float64)
    os.remove(out)
    assert len(w) == n
    return w


def cumsum(w, impl="cumsum"):
    """cum[i] = w[i] + cum[i - 1] as the plain C++ loop (impl = "chain": the replayed wavefront)."""
    src, out = _tmp("w"), _tmp("cum")
    np.ascontiguousarray(w, np.float64).tofile(src)
    _run(impl, src, out)
    cum = np.fromfile(out, np.float64)
    os.remove(src)
    os.remove(out)
    return cum


def draw(impl, state, cum, num):
    """`num` distinct ids drawn over the cumulative weights `cum` from engine state `state`, in the order of the sampled cloud:
    impl = std (the standard library's loop), single / rounds (the replayed kernel forms).
    Returns (ids uint32[num], engine state behind, attempts made, rounds)."""
    src, out = _tmp("cum"), _tmp("ids")
    np.ascontiguousarray(cum, np.float64).tofile(src)
    txt = _run("draw", impl, int(state), src, int(num), out)
    fields = dict(kv.split("=") for kv in txt.split())
    ids = np.fromfile(out, np.uint32)
    os.remove(src)
    os.remove(out)
    assert len(ids) == num
    return ids, int(fields["state"]), int(fields["draws"]), int(fields["rounds"])


def host_draw_ms(state, cum, num, reps=10):
    """Milliseconds the standard library's loop takes for this draw on this host (g++ -O2), timed inside the emulator — no process
    start, no file — as the minimum over `reps` runs."""
    src = _tmp("cum")
    np.ascontiguousarray(cum, np.float64).tofile(src)
    txt = _run("drawtime", int(state), src, int(num), int(reps))
    os.remove(src)
    return float(dict(kv.split("=") for kv in txt.split())["host_ms"])


def sample(state, cum, n_cloud, num):
    """PointCloudSamplerWithNormal::sample's ids for one model: nothing from an empty cloud or for a count of 0, the whole cloud in
    its own order when it has at most `num` points (neither draws), else the standard library's loop over `cum`.
    Returns (ids, engine state behind)."""
    if n_cloud == 0 or num == 0:
        return np.zeros(0, np.uint32), state
    if n_cloud <= num:
        return np.arange(n_cloud, dtype=np.uint32), state
    assert len(cum) == n_cloud
    ids, behind, _, _ = draw("std", state, cum, num)
    return ids, behind


def same_doubles(got, want):
    """Bit for bit, except that a NaN is a NaN: the sign and payload of a NaN made by inf - inf are the adder's (x86 makes the
    negative default NaN, the GPU the positive one), not the recurrence's."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(nan_g, nan_w) and np.array_equal(got.view(np.uint64)[~nan_g], want.view(np.uint64)[~nan_w]))
