"""float_prefix.h's wavefront form of the reference's float prefix recurrences (`accum += p.probability_`, pf.h:193-197, and
`pscan += pstep`, pf.h:421), replayed on the CPU lane by lane (tests/cpp/float_prefix_emul.cpp) against the plain loop: EVERY
prefix and the tie flag, bit for bit — normalised weights across the head and pass boundaries, constant terms, constants that are
rounding ties through a whole binade (the lane-0 rule), zeros and -0, large / negative / denormal / NaN / infinite terms, sums
that overflow. The step counts it prints are committed in profiles/resample_resident.txt. The record behind the chain (pstep,
initial_p, engine state) is checked against the reference's known answers of tests/golden/resample.npz."""
import os
import subprocess

import numpy as np
import pytest

import rng_ref

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
GOLD = np.load(os.path.join(HERE, "golden", "resample.npz"))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("float_prefix_emul") / "float_prefix_emul.bin"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", str(path), os.path.join(HERE, "cpp", "float_prefix_emul.cpp")],
                   check=True)
    return str(path)


def test_wavefront_prefixes_equal_the_serial_loop(exe):
    out = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=600).stdout
    print(out)
    assert "all equal" in out and "MISMATCH" not in out and "LANE-0 RULE" not in out, out
    steps = {}
    for line in out.splitlines():
        if line.startswith("steps "):
            name = line[6:line.index(" n=")].strip()
            fields = dict(f.split("=") for f in line[line.index(" n="):].split())
            steps[(name, int(fields["n"]))] = {k: int(v) for k, v in fields.items()}
    # the replay's figures: a dozen steps at 4096 particles, about n / 512 behind that
    assert steps[("weights x3", 4096)]["steps"] <= 20 and steps[("weights x30", 4096)]["steps"] <= 20
    assert steps[("weights x3", 262144)]["steps"] <= 262144 // 512 + 40
    # a constant that ties through a whole binade: 64 terms a step there (the lane-0 rule), never fewer than 16 elsewhere
    tie16 = steps[("tie constant, 16 bits", 200000)]
    assert tie16["min_retired"] >= 16 and tie16["steps"] <= 200000 // 64
    assert tie16["serial64"] >= 65536 // 64 - 256
    tie9 = steps[("tie constant, 9 bits", 3000)]
    assert tie9["serial64"] >= 4 and tie9["min_retired"] >= 16


def test_emulator_is_clean_under_the_host_sanitizers(tmp_path):
    """The emulator as a stand-alone program of its own with AddressSanitizer and UBSan, on the host: the replay indexes lanes
    and rows by hand."""
    path = tmp_path / "float_prefix_emul_san.bin"
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                    str(path), os.path.join(HERE, "cpp", "float_prefix_emul.cpp")], check=True)
    out = subprocess.run([str(path), "selftest"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def record(exe, state, n_out, mode, weights):
    bits = [str(int(b)) for b in np.asarray(weights, F).view(np.uint32)]
    out = subprocess.run([exe, "record", str(state), str(n_out), str(mode), *bits], check=True, capture_output=True, text=True).stdout
    pstep, ip, st, ties, total = (int(x) for x in out.split())
    as_f = lambda b: np.array([b], np.uint32).view(F)[0]
    return as_f(pstep), as_f(ip), st, ties, as_f(total)


def test_record_is_the_references(exe):
    """pstep = accum / (float)n, initial_p = uniform_real_distribution<float>(0, pstep)(engine(12345)): the weights of
    tests/test_gpu_rng_drawn.py::test_uniform_and_seed_are_the_references, the reference's own initial_p."""
    small = F(1.0e-06)
    for name, probs in (("first", [small, 0.2, 0.2, 0.2, F(0.4) - small]), ("last", [0.2, 0.2, 0.2, F(0.4) - small, small])):
        probs = np.array(probs, F)
        acc = F(0)
        for p in probs:
            acc = F(acc + p)
        pstep, ip, st, ties, total = record(exe, 12345, 5, 0, probs)
        assert total == acc and pstep == F(acc / F(5)) and ties == 0
        assert ip == GOLD["kat_initial_p_" + name]
        assert st == rng_ref.minstd_next(12345)
        # resizeParticle: no draw, the engine state as handed in
        pstep1, ip1, st1, _, _ = record(exe, 12345, 7, 1, probs)
        assert pstep1 == F(acc / F(7)) and ip1 == 0 and st1 == 12345
    # the two edges of generate_canonical: next output 1 (c = 0), next output 2^31 - 2 (c rounds to 1: nextafter(1, 0))
    w = np.full(4, 0.25, F)
    pstep, ip, st, _, _ = record(exe, rng_ref.A_INV, 4, 0, w)
    assert (pstep, ip, st) == (F(0.25), F(0), 1)
    pstep, ip, st, _, _ = record(exe, rng_ref.BEFORE_MAX, 4, 0, w)
    assert ip == F(np.nextafter(F(1), F(0)) * F(0.25)) and st == rng_ref.M - 1
    # dead particles raise the tie flag
    assert record(exe, 1, 4, 0, np.array([0.5, 0, 0.25, 0.25], F))[3] == 1
    assert record(exe, 1, 4, 0, np.array([0, 0.5, 0.25, 0.25], F))[3] == 0   # (a dead FIRST particle is no tie: 0 < 0.5)
