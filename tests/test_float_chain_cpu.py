"""float_chain.h's wavefront form of the reference's float recurrences (likelihood.cpp:120-134, pf.h:255-260), replayed on the
CPU lane by lane (tests/cpp/float_chain_emul.cpp) against the plain sequential loop it must reproduce bit for bit: likelihood-like
terms, deliberate rounding ties, wild magnitudes (binade crossings everywhere, denormals, huge terms), equal terms with a carried-in
sum, sign changes / NaN / infinity (the serial fallback), weight-like terms. Its second mode replays the vectors the GPU tests send
through the kernels (tests/float_chain_cases.py) and says what each of them exercises."""
import os
import subprocess

import numpy as np
import pytest

import float_chain_cases as fc
import pf_measure_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))


def test_wavefront_chain_equals_serial_loop(tmp_path):
    exe = tmp_path / "float_chain_emul.bin"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", str(exe), os.path.join(HERE, "cpp", "float_chain_emul.cpp")], check=True)
    out = subprocess.run([str(exe), "120"], check=True, capture_output=True, text=True, timeout=600).stdout
    assert "all equal" in out, out


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    """(exit code, {name: {"terms", "row" | "chunks": dict(equal, serial, emul, passes, clean, trouble, lanes)}}) for every vector of
    tests/float_chain_cases.py, as ONE row (pf_fused_kernel, update_small_kernel, the likelihood row) and as pf_strict_sum_kernel's
    rows of 4096 with the carried sum."""
    tmp = tmp_path_factory.mktemp("float_chain")
    exe, path = tmp / "float_chain_emul.bin", tmp / "cases.bin"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", str(exe), os.path.join(HERE, "cpp", "float_chain_emul.cpp")], check=True)
    cases = fc.all_cases()
    fc.write_cases(str(path), cases)
    run = subprocess.run([str(exe), "--cases", str(path)], capture_output=True, text=True, timeout=600)
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("case ")]
    assert len(lines) == 2 * len(cases), run.stdout[-2000:]
    out = {}
    for k, (name, t) in enumerate(cases):
        for ln in lines[2 * k:2 * k + 2]:
            assert int(ln[1]) == k and int(ln[3]) == len(t)
            out.setdefault(name, {"terms": t})[ln[4]] = dict(
                equal=ln[6] == "1", serial=np.array([int(ln[8], 16)], np.uint32).view(np.float32)[0],
                emul=np.array([int(ln[10], 16)], np.uint32).view(np.float32)[0], passes=int(ln[12]), clean=int(ln[14]),
                trouble=int(ln[16]), lanes=np.array(ln[18:82], np.int64))
    return run.returncode, out


def test_every_adversarial_case_is_the_serial_loop_in_the_replay(replayed):
    """Bit-equal (NaN equal to NaN) in both forms — and the plain C loop is the numpy loop the GPU tests expect."""
    returncode, vectors = replayed
    assert returncode == 0
    for name, r in vectors.items():
        want = fc.serial_sum(r["terms"])
        for form in ("row", "chunks"):
            assert r[form]["equal"], (name, form)
            assert fc.same_bits(r[form]["serial"], want) and fc.same_bits(r[form]["emul"], want), (name, form)


def test_the_gpu_tests_are_not_vacuous(replayed):
    """Conditions on the INPUTS of tests/test_gpu_float_chain_adversarial.py: which vectors reach a wavefront pass, a clean one,
    one with trouble, and every lane as the first one in trouble. A family that misses one is changed, not the condition."""
    replayed = replayed[1]
    for n in fc.SIZES:
        for form in ("row", "chunks"):
            for family in ("weights", "wild"):
                r = replayed["%s/%d" % (family, n)][form]
                if n >= 768:
                    assert r["clean"] >= 1 and r["trouble"] >= 1, (family, n, form, r)
            for family in ("ties", "equal"):
                r = replayed["%s/%d" % (family, n)][form]
                if n >= 768:
                    assert r["trouble"] >= 1, (family, n, form, r)
            if n <= fc.HEAD:
                for name, r in replayed.items():
                    if len(r["terms"]) == n:
                        assert r[form]["passes"] == 0, (name, form)
    # a special value in lane 63 of the first pass reaches a pass at every size that has that term
    for tag, _ in fc.SPECIAL_VALUES:
        pos = fc.HEAD + 8 * 63 + 3
        assert replayed["specials/1000/%s@%d" % (tag, pos)]["row"]["passes"] >= 1
    # every lane is the first one in trouble of some pass: one row of 1000 terms, and the second row of pf_strict_sum_kernel
    for n, form in zip(fc.EVERY_LANE_SIZES, ("row", "chunks")):
        hist = sum(replayed["every_lane/%d/%d" % (n, lane)][form]["lanes"] for lane in range(64))
        assert np.all(hist > 0), (n, form, hist)
        for lane in range(64):   # ... and by construction it is the lane the vector names, then lane 63 - lane
            lanes = replayed["every_lane/%d/%d" % (n, lane)][form]["lanes"]
            assert lanes[lane] >= 1 and lanes[63 - lane] >= 1, (n, lane, lanes)


def test_pf_measure_restatement_restore_rule():
    """tests/pf_measure_ref.py: restore unless the float sum > 0 — 0, a negative sum and NaN restore, +inf does not."""
    w = np.array([0.25, 0.5, 0.25], np.float32)
    for lik, restored in (([0, 0, 0], True), ([1, np.nan, 1], True), ([0.25, -1, 0.25], True), ([1, np.inf, 1], False),
                          ([3e38, 3e38, 3e38], False), ([1, 2, 1], False)):
        m = pr.measure(w, np.array(lik, np.float32))
        assert m["restored"] is restored, lik
        if restored:
            np.testing.assert_array_equal(m["weights"], w)
    m = pr.measure(w, np.array([1, np.inf, 1], np.float32))
    assert m["weights"][0] == 0 and np.isnan(m["weights"][1]) and m["weights"][2] == 0
    m = pr.measure(np.ones(3, np.float32), np.array([3e38, 3e38, 3e38], np.float32))   # finite terms, a sum past the largest float
    assert np.isinf(m["sum"]) and np.all(m["weights"] == 0)
    m = pr.measure(w, np.array([1, 2, 1], np.float32), beam=np.array([2, 1, 2], np.float32), extra=np.array([1, 1, 1], np.float32))
    np.testing.assert_array_equal(m["weights"], np.array([0.25, 0.5, 0.25], np.float32))
    H, bound = pr.entropy(m["wn"], m["sum"])
    assert abs(H - 1.5 * np.log(2.0)) <= bound
