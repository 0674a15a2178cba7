"""Reference side of the device-drawn uniform sampler (mcl_3dl_amd/csrc/rng_index.h, rng_index_kernels.h): libstdc++'s
std::uniform_int_distribution<size_t>(0, n - 1) over std::default_random_engine (minstd_rand0) restated in integers — the yardstick
where neither the reference tree nor a compiler is at hand — and the door to tests/cpp/rng_index_emul.cpp, which holds the
standard library's own stream and the CPU replay of both kernel forms.

bits/uniform_int_dist.h, "fallback case (2 divisions)": the engine's min is 1, its max 2^31 - 2, urngrange = 2147483645. For a range
of n values: n <= urngrange: scaling = urngrange // n, past = n * scaling, repeat ret = engine() - 1 until ret < past, result
ret // scaling. n == 2147483646: ret = engine() - 1, no rejection (the same with scaling 1, past 2147483646). Larger ranges take the
up-scaling branch, which is not restated."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
M = 2 ** 31 - 1
A = 16807
URNG_RANGE = 2147483645
MAX_RANGE = 2147483646
A_INV = pow(A, M - 2, M)            # the engine state whose next output is 1 (ret = 0)
BEFORE_MAX = (M - 1) * A_INV % M    # ... whose next output is 2^31 - 2 (ret = urngrange)
RANGES = [1, 2, 3, 96, 4089, 65469, 10 ** 6, 1500000000, 2147483645, 2147483646]
# (state, range, count) whose first round of the rounds form falls short: tests/test_rng_index_cpu.py asserts that they do,
# tests/test_gpu_scan_prepared.py runs them on the device
SECOND_ROUND = [(13, 1500000000, 7), (889, 1500000000, 7)]

_BLOCK = 4096
_POW = None


def _powers():
    global _POW
    if _POW is None:
        p, x = np.zeros(_BLOCK, np.uint64), 1
        for i in range(_BLOCK):
            x = x * A % M
            p[i] = x
        _POW = p
    return _POW


def range_constants(n):
    """(scaling, past) of a range of n values."""
    assert 1 <= n <= MAX_RANGE
    if n > URNG_RANGE:
        return 1, MAX_RANGE
    scaling = URNG_RANGE // n
    return scaling, n * scaling


def draw(state, n, count):
    """count draws of uniform_int_distribution<size_t>(0, n - 1) from engine state `state`: (uint32[count], the state behind)."""
    assert 1 <= state <= M - 1
    scaling, past = range_constants(n)
    out = np.zeros(count, np.uint32)
    have, x = 0, int(state)
    pw = _powers()
    while have < count:
        # the next _BLOCK engine outputs: x 16807^(t + 1) mod (2^31 - 1); x < 2^31 and the powers < 2^31, so the product fits 64 bits
        v = (np.uint64(x) * pw) % np.uint64(M)
        ok = np.flatnonzero(v - np.uint64(1) < np.uint64(past))
        take = ok[:count - have]
        out[have:have + len(take)] = ((v[take] - np.uint64(1)) // np.uint64(scaling)).astype(np.uint32)
        have += len(take)
        # the stream stands behind the last ACCEPTED attempt when the draws are complete
        x = int(v[take[-1]]) if have == count else int(v[-1])
    return out, x


def scan_draws(state, n_s, n_lik_clipped, n_b, n_beam_clipped):
    """One scan's draws as measure() makes them (src/mcl_3dl.cpp:377-383, std::map order): beam's n_b over the clipped beam cloud
    first, then the likelihood's n_s; an empty cloud or a count of 0 draws nothing. Returns (idx_lik, idx_beam, state behind)."""
    idx_beam, idx_lik = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    if n_b and n_beam_clipped:
        idx_beam, state = draw(state, n_beam_clipped, n_b)
    if n_s and n_lik_clipped:
        idx_lik, state = draw(state, n_lik_clipped, n_s)
    return idx_lik, idx_beam, state


_exe = None


def emul_exe(extra_flags=()):
    """tests/cpp/rng_index_emul.cpp, compiled once per process into a temporary directory (extra_flags: a build of its own)."""
    global _exe
    if _exe is not None and not extra_flags:
        return _exe
    import atexit
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="rng_index_emul_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "rng_index_emul.bin")
    subprocess.run(["g++", "-O2", *extra_flags, "-o", exe, os.path.join(HERE, "cpp", "rng_index_emul.cpp")], check=True)
    if not extra_flags:
        _exe = exe
    return exe


def emul(impl, state, n_b, range_b, n_s, range_s):
    """The emulator's `draw`: impl = std (the standard library), single / rounds (the replayed kernel forms). Returns (idx_beam,
    idx_lik, engine state behind, rounds)."""
    exe = emul_exe()
    out = os.path.join(os.path.dirname(exe), "draw_%d.bin" % os.getpid())
    txt = subprocess.run([exe, "draw", impl, str(int(state)), str(int(n_b)), str(int(range_b)), str(int(n_s)), str(int(range_s)),
                          out], check=True, capture_output=True, text=True, timeout=300).stdout
    fields = dict(kv.split("=") for kv in txt.split())
    v = np.fromfile(out, np.uint32)
    os.remove(out)
    assert len(v) == n_b + n_s
    return v[:n_b], v[n_b:], int(fields["state"]), int(fields["rounds"])
