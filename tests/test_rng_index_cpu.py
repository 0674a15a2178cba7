"""The restatement of the reference's uniform sampler (mcl_3dl_amd/csrc/rng_index.h) against the standard library itself, on the
CPU: tests/cpp/rng_index_emul.cpp replays both kernel forms of rng_index_kernels.h — runs of E attempts per lane, 64-lane ballots,
256-thread passes, the one-work-group form's pass loop and two-segment hand-over, the rounds form's count / scan / emit with
index_attempt_budget — and must reproduce std::default_random_engine + std::uniform_int_distribution<size_t> value for value and in
the engine state behind. tests/rng_index_ref.py, the numpy restatement the GPU tests use as their yardstick, is held against the
same standard-library results."""
import re
import subprocess

import numpy as np
import pytest

import rng_index_ref as rir

E = 8  # rng_polar.h: ATTEMPTS_PER_LANE
SECOND_ROUND = rir.SECOND_ROUND
CASE = re.compile(r"^case (\S+) state=(\d+) range0=(\d+) count0=(\d+)(?: range1=(\d+) count1=(\d+))? rounds=(\d+) attempts=\d+ "
                  r"behind=(\d+) (\w+)$", flags=re.M)


@pytest.fixture(scope="module")
def selftest():
    out = subprocess.run([rir.emul_exe(), "selftest"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout[-3000:]
    return [dict(name=c[0], state=int(c[1]), range0=int(c[2]), count0=int(c[3]), range1=int(c[4] or 0), count1=int(c[5] or 0),
                 rounds=int(c[6]), behind=int(c[7]), verdict=c[8]) for c in CASE.findall(out.stdout)]


def test_both_replayed_forms_equal_the_standard_library(selftest):
    """Every range of {1, 2, 3, 96, 4089, 65 469, 10^6, 1.5 10^9, 2 147 483 645, 2 147 483 646} x every count of {1, 2, 63, 64, 65,
    255, 256, 257, 2 * 256 * E -+ 1, 100 000} from start states that include both edges (next output 1; next output 2^31 - 2): the
    one-work-group form, the rounds form and the standard library agree in every value and in the engine state behind."""
    cases = selftest
    assert cases and all(c["verdict"] == "equal" for c in cases)
    one = [c for c in cases if c["name"] == "one"]
    assert {c["range0"] for c in one} == set(rir.RANGES)
    assert {c["count0"] for c in one} == {1, 2, 63, 64, 65, 255, 256, 257, 2 * 256 * E - 1, 2 * 256 * E + 1, 100000}
    for edge in (rir.A_INV, rir.BEFORE_MAX):
        at_edge = [c for c in one if c["state"] == edge]
        assert {c["range0"] for c in at_edge} == set(rir.RANGES)
    assert {1, 12345, 2 ** 31 - 2, 109} <= {c["state"] for c in one}
    # every (range, count) pair is there from every start (the 100 000-draw stream from two of them)
    assert len({(c["state"], c["range0"], c["count0"]) for c in one}) == 6 * 10 * 10 + 2 * 10


def test_two_segments_hand_over(selftest):
    """Beam first, then the likelihood, on one stream: an empty first segment, an empty second one, a pass boundary inside either,
    a rejected attempt right in front of segment 1's last accepted one, and right behind it an attempt that segment 1's range would
    have rejected (segment 2 judges it by its own)."""
    two = [c for c in selftest if c["name"] == "two"]
    assert any(c["count0"] == 0 and c["count1"] > 0 for c in two) and any(c["count0"] > 0 and c["count1"] == 0 for c in two)
    assert any(c["count0"] + c["count1"] > 2 * 256 * E for c in two)
    assert {(c["count0"], c["count1"]) for c in two} >= {(3, 96), (16, 700), (512, 16384)}
    for name in ("two-rejected-before-last", "two-rejected-behind-last"):
        assert sum(c["name"] == name for c in selftest) >= 2, name


def test_rounds_are_one_mostly_two_sometimes_never_many(selftest):
    rounds = [c["rounds"] for c in selftest]
    assert rounds.count(1) >= 1 and sum(r >= 2 for r in rounds) >= 1 and max(rounds) <= 4, sorted(set(rounds))
    short = {(c["state"], c["range0"], c["count0"]) for c in selftest if c["name"] == "small" and c["rounds"] == 2}
    assert set(SECOND_ROUND) <= short


@pytest.mark.parametrize("state", [1, 12345, 2 ** 31 - 2, 109, rir.A_INV, rir.BEFORE_MAX])
def test_numpy_restatement_equals_the_standard_library(state):
    """tests/rng_index_ref.py against the emulator's `draw std`, per range, and the scan's two-segment order with its empty cases."""
    for n in rir.RANGES:
        for count in (1, 64, 257, 5000):
            want, _, behind, _ = rir.emul("std", state, count, n, 0, 1)
            got, st = rir.draw(state, n, count)
            np.testing.assert_array_equal(got, want)
            assert st == behind, (n, count)
    for n_s, n_lik, n_b, n_beam in ((96, 2893, 3, 1507), (700, 2893, 16, 1507), (96, 2893, 0, 1507), (0, 2893, 3, 1507),
                                    (16384, 1500000000, 512, 1500000000)):
        want_b, want_l, behind, _ = rir.emul("std", state, n_b, n_beam, n_s, n_lik)
        got_l, got_b, st = rir.scan_draws(state, n_s, n_lik, n_b, n_beam)
        np.testing.assert_array_equal(got_l, want_l)
        np.testing.assert_array_equal(got_b, want_b)
        assert st == behind
    # an empty clipped cloud draws nothing, whatever was asked for
    got_l, got_b, st = rir.scan_draws(state, 96, 0, 3, 0)
    assert len(got_l) == 0 and len(got_b) == 0 and st == state


def test_second_round_triples_through_the_numpy_restatement():
    for state, n, count in SECOND_ROUND:
        want, _, behind, rounds = rir.emul("rounds", state, count, n, 0, 1)
        assert rounds == 2
        got, st = rir.draw(state, n, count)
        np.testing.assert_array_equal(got, want)
        assert st == behind


def test_emulator_is_clean_under_the_host_sanitizers():
    """The emulator as a stand-alone program of its own with AddressSanitizer and UBSan, on the host: the replay indexes lanes,
    ballots and output windows by hand."""
    exe = rir.emul_exe(extra_flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "all equal" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
