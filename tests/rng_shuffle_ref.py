"""Reference side of the shuffle of the sampled covariance (mcl_3dl_amd/csrc/rng_shuffle.h, rng_shuffle_kernels.h): the door to
tests/cpp/rng_shuffle_emul.cpp, which holds the standard library's own std::shuffle over std::default_random_engine (libstdc++),
the header's serial loop and the CPU replay of the kernels; and pf::covariance's sample_num (pf.h:326-331 with FLT_TYPE = float)."""
import os
import subprocess

import numpy as np

import rng_index_ref as rir

HERE = os.path.dirname(os.path.abspath(__file__))
PAIR_MAX = 46340  # the largest n of libstdc++'s pair path (urngrange / n >= n): made on the host; above, on the device
STARTS = [1, 12345, 2 ** 31 - 2, rir.A_INV, rir.BEFORE_MAX]
# (n, state) -> rejected attempts of the single path, as the emulator's self-test reports them
REJECTIONS = {(46341, 1): 1, (200001, 1): 6, (450408, 1): 27, (46341, 12345): 0}

_exe = None


def emul_exe(extra_flags=()):
    """tests/cpp/rng_shuffle_emul.cpp, compiled once per process into a temporary directory (extra_flags: a build of its own)."""
    global _exe
    if _exe is not None and not extra_flags:
        return _exe
    import atexit
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="rng_shuffle_emul_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "rng_shuffle_emul.bin")
    subprocess.run(["g++", "-O2", *extra_flags, "-o", exe, os.path.join(HERE, "cpp", "rng_shuffle_emul.cpp")], check=True)
    if not extra_flags:
        _exe = exe
    return exe


_memo = {}


def emul(impl, state, n, m):
    """The emulator's `shuffle`: impl = std (the standard library), serial (the header's loop), device (the replayed kernels).
    Returns (the first m entries uint32[m], engine state behind the whole shuffle, the printed fields). Kept per argument tuple."""
    key = (impl, int(state), int(n), int(m))
    if key not in _memo:
        exe = emul_exe()
        out = os.path.join(os.path.dirname(exe), "shuffle_%d.bin" % os.getpid())
        txt = subprocess.run([exe, "shuffle", impl, str(int(state)), str(int(n)), str(int(m)), out], check=True,
                             capture_output=True, text=True, timeout=300).stdout
        fields = {k: int(v) for k, v in (kv.split("=") for kv in txt.split())}
        v = np.fromfile(out, np.uint32)
        os.remove(out)
        assert len(v) == m
        v.setflags(write=False)
        _memo[key] = (v, fields["state"], fields)
    return _memo[key]


def sample_count(n, ratio):
    """min(n, (size_t)((float)n * ratio)): a float product, truncated."""
    return min(int(n), int(np.float32(n) * np.float32(ratio)))
