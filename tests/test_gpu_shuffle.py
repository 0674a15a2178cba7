"""mcl3dl_hip_rng_shuffle_prefix on the device (rng_shuffle_kernels.h, host_shuffle.h) against libstdc++'s own std::shuffle over
std::default_random_engine, which tests/cpp/rng_shuffle_emul.cpp holds: the first m entries in the shuffle's order and the engine
state behind the whole shuffle. From 46341 elements on the shuffle is made on the device; below, the library's serial loop runs
on the host (the standard library's pair path)."""
import ctypes as C

import numpy as np
import pytest

import rng_shuffle_ref as rsr
from mcl_3dl_amd import capi

pytestmark = pytest.mark.gpu
# start states with known rejections on the device path (tests/test_rng_shuffle_cpu.py asserts the counts): state 1 rejects 1
# attempt at 46341 and 6 at 200001; the edge state's first attempt, ret = urngrange, is rejected at step 1 of every shuffle
STATES = [1, rsr.rir.BEFORE_MAX]


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("n", [46341, 50000, 200001, 1, 2, 1000, 46340])
def test_prefix_equals_the_standard_library(engine, n, state):
    want, behind, _ = rsr.emul("std", state, n, n)
    if n > rsr.PAIR_MAX:
        fields = rsr.emul("device", state, n, 1)[2]
        print("n %d state %d: %d doubtful, %d rejected" % (n, state, fields["doubtful"], fields["rejected"]))
        assert fields["rejected"] > 0
    for m in sorted({1, max(1, n // 10), n}):
        got, st = engine.rng_shuffle_prefix(n, m, state)
        np.testing.assert_array_equal(got, want[:m])
        assert st == behind, (n, m)
    np.testing.assert_array_equal(np.sort(got), np.arange(n, dtype=np.uint32))  # m == n: a permutation of 0 .. n - 1
    # no entry asked for: the stream still stands behind the whole shuffle
    none, st = engine.rng_shuffle_prefix(n, 0, state)
    assert len(none) == 0 and st == behind


def test_a_stream_without_a_rejection(engine):
    n, state = 46341, 12345
    assert rsr.emul("device", state, n, 1)[2]["rejected"] == 0
    want, behind, _ = rsr.emul("std", state, n, n)
    got, st = engine.rng_shuffle_prefix(n, n, state)
    np.testing.assert_array_equal(got, want)
    assert st == behind


def test_errors_leave_the_state(engine):
    lib = engine.lib
    out = np.zeros(8, np.uint32)
    for n, m, state in ((0, 0, 5), (2 ** 31 - 1, 1, 5), (100, 101, 5), (50000, 50001, 5), (100, 4, 0), (50000, 4, 2 ** 31 - 1)):
        st = C.c_uint32(state)
        assert lib.mcl3dl_hip_rng_shuffle_prefix(engine.h, n, m, C.byref(st), capi._ptr(out)) == -3, (n, m, state)
        assert st.value == state and not out.any()
    st = C.c_uint32(5)
    assert lib.mcl3dl_hip_rng_shuffle_prefix(engine.h, 100, 4, C.byref(st), None) == -3 and st.value == 5
    assert lib.mcl3dl_hip_rng_shuffle_prefix(engine.h, 100, 4, None, capi._ptr(out)) == -3
