"""std::shuffle(iota(n), engine_) of pf::covariance restated (mcl_3dl_amd/csrc/rng_shuffle.h) against the standard library itself,
on the CPU: tests/cpp/rng_shuffle_emul.cpp replays the kernels of rng_shuffle_kernels.h lane by lane — runs of E attempts behind a
jump, the doubtful attempts counted, scanned and emitted in stream order, the one-wavefront resolve, every attempt's step, the
sort's contract, one chain walk per entry, the host's rounds — and must reproduce libstdc++'s std::shuffle over
std::default_random_engine in every entry and in the engine state behind. The header's serial loop, which the library runs on
the host for n <= 46340 (the standard library's pair path), is held against the same."""
import re
import subprocess

import numpy as np
import pytest

import rng_shuffle_ref as rsr

CASE = re.compile(r"^case (\S+) n=(\d+) m=(\d+) state=(\d+) rounds=(\d+) attempts=(\d+) doubtful=(\d+) rejected=(\d+) hops=(\d+) "
                  r"behind=(\d+) (\w+)$", flags=re.M)
SINGLE = [46341, 46342, 50000, 65537, 200001, 450408]
PAIR = [1, 2, 3, 4, 5, 7, 8, 100, 101, 1000, 46339, 46340]
FORCED = [2, 3, 64, 65, 257, 4097]


@pytest.fixture(scope="module")
def selftest():
    out = subprocess.run([rsr.emul_exe(), "selftest"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout[-3000:]
    keys = ("name", "n", "m", "state", "rounds", "attempts", "doubtful", "rejected", "hops", "behind", "verdict")
    cases = [dict(zip(keys, [c[0]] + [int(x) for x in c[1:10]] + [c[10]])) for c in CASE.findall(out.stdout)]
    assert cases and all(c["verdict"] == "equal" for c in cases)
    return cases


def named(cases, name):
    return [c for c in cases if c["name"] == name]


def test_replayed_kernels_equal_the_standard_library_on_the_single_path(selftest):
    """Every size of the device path from every start state, whole permutations: the standard library, the header's serial loop
    and the replayed kernels agree in every entry, in the engine state behind and in the number of rejected attempts."""
    single = named(selftest, "single")
    assert {(c["n"], c["state"]) for c in single} == {(n, s) for n in SINGLE for s in rsr.STARTS}
    assert all(c["m"] == c["n"] and c["rounds"] == 1 for c in single)
    for c in single:
        print("n %(n)d state %(state)d: %(doubtful)d doubtful, %(rejected)d rejected, longest chain %(hops)d hops" % c)
    got = {(c["n"], c["state"]): c["rejected"] for c in single}
    for key, want in rsr.REJECTIONS.items():
        assert got[key] == want, key
    # streams without a rejection and with rejections; a doubtful attempt that its own step accepts
    assert any(c["rejected"] == 0 for c in single) and any(c["rejected"] > 0 for c in single)
    assert any(c["doubtful"] > 0 for c in single) and any(c["doubtful"] > c["rejected"] for c in single)
    assert all(c["doubtful"] >= c["rejected"] for c in selftest if c["name"] != "pair")
    assert max(c["hops"] for c in single) <= 64


def test_serial_loop_equals_the_standard_library_on_the_pair_path(selftest):
    """What the library runs on the host: both parities of n, the sizes without a draw (1) and with one (2), and the threshold."""
    pair = named(selftest, "pair")
    assert {(c["n"], c["state"]) for c in pair} == {(n, s) for n in PAIR for s in rsr.STARTS}
    assert all(c["behind"] == c["state"] for c in pair if c["n"] == 1)  # nothing drawn
    assert any(c["rejected"] > 0 for c in pair)


def test_single_path_forced_at_wave_and_pass_boundaries(selftest):
    forced = named(selftest, "forced")
    assert {c["n"] for c in forced} >= set(FORCED) and {c["state"] for c in forced} == set(rsr.STARTS)
    assert any(c["rejected"] > 0 for c in forced)  # the edge start: ret = urngrange is past every range but the widest


def test_second_round_and_long_lists(selftest):
    short = named(selftest, "short")
    assert {c["n"] for c in short} == {46341, 200001, 450408} and all(c["rounds"] == 2 for c in short)
    assert [c["rejected"] for c in sorted(short, key=lambda c: c["n"])] == [1, 6, 27]
    long_ = named(selftest, "long")
    assert long_ and all(c["doubtful"] > 640 and c["rejected"] > 64 for c in long_)  # ten batches of the resolve and more
    prefix = named(selftest, "prefix")
    assert {c["m"] for c in prefix} >= {1, 4634, 20000}


@pytest.mark.parametrize("n,state", [(46341, 1), (50000, rsr.rir.BEFORE_MAX), (1000, 12345), (46340, 1)])
def test_the_door_the_gpu_tests_use(n, state):
    m = max(1, n // 10)
    want, behind, _ = rsr.emul("std", state, n, n)
    assert sorted(want.tolist()) == list(range(n))
    got, st, _ = rsr.emul("serial", state, n, m)
    np.testing.assert_array_equal(got, want[:m])
    assert st == behind
    if n > rsr.PAIR_MAX:
        got, st, fields = rsr.emul("device", state, n, m)
        np.testing.assert_array_equal(got, want[:m])
        assert st == behind and fields["rounds"] == 1


def test_sample_count_is_a_float_product():
    assert rsr.sample_count(450408, 0.1) == 45040 and rsr.sample_count(46341, 0.75) == 34755
    assert rsr.sample_count(4096, 0.1) == 409 and rsr.sample_count(10, 0.05) == 0
    # (float)33554435 is 33554436: the float product truncates to 16777218, the double product to 16777217
    assert rsr.sample_count(33554435, 0.5) == 16777218 != int(33554435 * 0.5)


def test_emulator_is_clean_under_the_host_sanitizers():
    """The emulator as a stand-alone program of its own with AddressSanitizer and UBSan, on the host: the replay indexes lanes,
    ballots, the doubtful and rejected lists and the sorted pairs by hand."""
    exe = rsr.emul_exe(extra_flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "all equal" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
