"""The restatement of the normal-weighted sampler's draw (mcl_3dl_amd/csrc/rng_weighted.h, double_chain.h) against the standard
library itself, on the CPU: tests/cpp/rng_weighted_emul.cpp replays the wavefront's cumulative chain lane by lane against the plain
loop, and both kernel forms of rng_weighted_kernels.h — the per-thread steps the kernels compile, run thread after thread forwards
and backwards — against std::default_random_engine + std::uniform_real_distribution<double> + std::lower_bound +
std::unordered_set<size_t>: ids, their order, the attempts made and the engine state behind must all be equal."""
import re
import subprocess

import numpy as np
import pytest

import rng_weighted_ref as rwr

CHAIN = re.compile(r"^chain (\w+) n=(\d+) passes=(\d+) full=(\d+) serial_blocks=(\d+) (\w+)$", flags=re.M)
CASE = re.compile(r"^case (\S+) kind=(\w+) n=(\d+) num=(\d+) state=(\d+) draws=(\d+) behind=(\d+) rounds=(\d+) single=(\d) (\w+)$",
                  flags=re.M)
TWO = re.compile(r"^case two n0=(\d+) num0=(\d+) n1=(\d+) num1=(\d+) state=(\d+) draws0=(\d+) draws1=(\d+) behind=(\d+) (\w+)$",
                 flags=re.M)


@pytest.fixture(scope="module")
def selftest():
    out = subprocess.run([rwr.emul_exe(), "selftest"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout[-3000:]
    return out.stdout


def test_bucket_table_equals_the_containers(selftest):
    """The committed bucket counts against std::unordered_set<size_t>::bucket_count() while 800 000 ids are inserted one by one (and
    the rehash falls on the insertion that exceeds the count), the rest against the growth policy the container consults."""
    m = re.search(r"^table grown=(\d+) policy=(\d+) (\w+)$", selftest, flags=re.M)
    assert m and m.group(3) == "equal" and int(m.group(1)) >= 17 and int(m.group(1)) + int(m.group(2)) == 28


def test_canonical_and_the_unreachable_branch(selftest):
    """generate_canonical<double, 53> value for value at the engine's edge states; the one predecessor of the largest output is
    where the header says, the largest c of the stream is below 1 and the c >= 1 branch is not reachable."""
    m = re.search(r"^canonical v1_before_max=(\d+) c_max=(\S+) lowest_v1_reaching_one=(\d+) reachable=(\d) (\w+)$", selftest,
                  flags=re.M)
    assert m and m.group(5) == "equal" and m.group(4) == "0"
    v1 = int(m.group(1))
    assert v1 * 16807 % (2 ** 31 - 1) == 2 ** 31 - 2 and float(m.group(2)) < 1.0
    # a v1 within a few hundred of the range WOULD reach it: the branch is dead by the engine's recurrence, not by the arithmetic
    assert 0 < 2 ** 31 - 2 - int(m.group(3)) < 1024 and int(m.group(3)) > v1


def test_chain_equals_the_plain_loop(selftest):
    """All-ones, random weights in [1, 5], forced ties, terms of at least half the sum, negative terms, +-inf, NaN, -0 and a
    denormal, at lengths either side of the serial head, of a pass and far beyond."""
    rows = CHAIN.findall(selftest)
    assert {(k, int(n)) for k, n, *_ in rows} == {(k, n) for k in rwr.KINDS for n in rwr.LENGTHS}
    assert all(r[5] == "equal" for r in rows)
    by = {(k, int(n)): (int(p), int(f), int(s)) for k, n, p, f, s, _ in rows}
    # weights that are all 1.0 stay on the fast path: a pass per 512 terms plus one per binade edge (2^8 .. 2^16)
    passes, full, serial = by[("ones", 70000)]
    assert serial == 0 and full >= 70000 // 512 - 9 and passes <= 70000 // 512 + 10
    # the inputs that must leave it do leave it
    assert by[("ties", 70000)][1] == 0 and by[("ties", 70000)][0] > 1000
    assert by[("special", 70000)][2] > 100 and by[("neg", 70000)][0] > 1000


def test_both_replayed_forms_equal_the_standard_library(selftest):
    cases = [dict(name=c[0], kind=c[1], n=int(c[2]), num=int(c[3]), state=int(c[4]), draws=int(c[5]), rounds=int(c[7]),
                  single=int(c[8]), verdict=c[9]) for c in CASE.findall(selftest)]
    assert cases and all(c["verdict"] == "equal" for c in cases)
    edges = {1, 12, 13, 14, 29, 30, 59, 60, 127, 128}
    for state in (1, 12345, 2 ** 31 - 2):
        assert {c["num"] for c in cases if c["name"] == "edge" and c["state"] == state} == edges
        assert {c["num"] for c in cases if c["name"] == "tight" and c["state"] == state and c["n"] == c["num"] + 1} >= edges
    # n = num + 1: duplicates dominate (several attempts per id), and the rounds form needs more than one round somewhere
    tight = [c for c in cases if c["name"] == "tight" and c["num"] >= 127]
    assert all(c["draws"] > 3 * c["num"] for c in tight) and max(c["rounds"] for c in tight) >= 2
    # either side of the one-work-group cap, and far beyond it
    assert {(c["num"], c["single"]) for c in cases if c["name"] == "cap"} == {(rwr.SINGLE_MAX, 1), (rwr.SINGLE_MAX + 1, 0)}
    assert any(c["num"] == 16384 and c["n"] == 65000 for c in cases)
    assert any(c["kind"] == "ones" for c in cases)


def test_two_segments_hand_over(selftest):
    """Beam first, then the likelihood, on one stream: the second segment starts behind the last attempt the first one MADE; an
    empty first segment, an empty second one, and segments that take several passes."""
    two = [dict(num0=int(c[1]), num1=int(c[3]), draws0=int(c[5]), draws1=int(c[6]), verdict=c[8]) for c in TWO.findall(selftest)]
    assert two and all(c["verdict"] == "equal" for c in two)
    assert any(c["num0"] == 0 and c["num1"] > 0 for c in two) and any(c["num0"] > 0 and c["num1"] == 0 for c in two)
    assert any(c["draws0"] > 1024 and c["draws1"] > 1024 for c in two)
    assert any(c["draws0"] > c["num0"] > 0 for c in two)


def test_command_line_forms_agree():
    """The doors the GPU tests use: weights / cumsum / chain / draw."""
    w = rwr.weights("rand", 3000)
    cum = rwr.cumsum(w)
    np.testing.assert_array_equal(cum, np.cumsum(w))  # (numpy's cumsum is the same sequential loop)
    assert rwr.same_doubles(rwr.cumsum(w, "chain"), cum)
    sp = rwr.weights("special", 513)
    assert np.isnan(rwr.cumsum(sp)[-1]) and rwr.same_doubles(rwr.cumsum(sp, "chain"), rwr.cumsum(sp))
    want = rwr.draw("std", 12345, cum, 700)
    assert len(set(want[0].tolist())) == 700 and want[2] >= 700
    for impl in ("single", "rounds"):
        got = rwr.draw(impl, 12345, cum, 700)
        np.testing.assert_array_equal(got[0], want[0])
        assert got[1:3] == want[1:3]
    ids, behind = rwr.sample(5, cum, 3000, 3000)
    np.testing.assert_array_equal(ids, np.arange(3000))
    assert behind == 5
    ids, behind = rwr.sample(5, cum, 3000, 0)
    assert len(ids) == 0 and behind == 5


def test_emulator_is_clean_under_the_host_sanitizers():
    """The emulator as a stand-alone program of its own with AddressSanitizer and UBSan, on the host: the replay indexes lanes,
    chains, buckets and output windows by hand."""
    exe = rwr.emul_exe(extra_flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "all equal" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
