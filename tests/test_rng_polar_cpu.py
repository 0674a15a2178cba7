"""The restatement of the reference's random stream (mcl_3dl_amd/csrc/rng_polar.h) against the standard library itself, on the CPU:
tests/cpp/rng_polar_emul.cpp replays the kernels' decomposition — runs of E attempts per lane, 64-lane ballots, 256-thread
work-groups, the scan, the rounds with attempt_budget — and must reproduce std::default_random_engine +
std::normal_distribution<float> / uniform_real_distribution<float> bit for bit when its logarithm is the host's std::log(float);
with the device's logarithm (double, rounded to float) the decisions and the engine state stay identical and every value lies
within the bound derived in tests/rng_ref.py."""
import re
import subprocess

import numpy as np

import rng_ref


def test_replayed_kernels_equal_the_standard_library():
    """Fresh-per-value with a mean and a sigma, the shared form, the uniform, a rank's window, all 64 zero patterns of the sigmas,
    K in {1, 2, 63, 64, 65, 255, 256, 257, 2 * 256 * E -+ 1, 100 000} from start states that include both edges of canonical (next
    output 1; next output 2^31 - 2), the engine state behind each — and the rounds: one for most, two now and then, never many."""
    out = subprocess.run([rng_ref.emul_exe(), "selftest"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout[-3000:]
    cases = re.findall(r"^case (\S+) state=(\d+) k=(\d+) rounds=(\d+) attempts=\d+ (\w+)$", out.stdout, flags=re.M)
    assert all(c[4] == "equal" for c in cases)
    names = {c[0] for c in cases}
    assert {"fresh", "shared", "uniform", "window", "small"} <= names and sum(n.startswith("sigma") for n in names) == 64
    for edge in (rng_ref.A_INV, rng_ref.BEFORE_MAX):
        assert {c[0] for c in cases if int(c[1]) == edge} >= {"fresh", "shared", "uniform", "window"}
    ks = {int(c[2]) for c in cases if c[0] == "fresh"}
    assert ks == {1, 2, 63, 64, 65, 255, 256, 257, 4095, 4097, 100000}
    rounds = [int(c[3]) for c in cases if c[0] != "uniform"]
    assert rounds.count(1) >= 1 and sum(r >= 2 for r in rounds) >= 1 and max(rounds) <= 4, sorted(set(rounds))
    # the pairs tests/test_gpu_rng_drawn.py runs on the device
    two = {(int(c[1]), int(c[2])) for c in cases if c[0] == "small" and int(c[3]) == 2}
    assert {(109, 1), (704, 2)} <= two


def test_double_logarithm_keeps_decisions_and_stays_within_the_bound():
    """The device's policy on the CPU over a 2 000 000-value stream: same number of attempts, same engine state, every value within
    VALUE_REL of the standard library's. The share of values that are not identical is printed, not asserted (a property of the
    host's libm)."""
    n, state = 2000000, rng_ref.minstd_seed(12345)
    for form in ("fresh", "shared"):
        want, st_want, _ = rng_ref.stream("std", form, state, n)
        host, st_host, _ = rng_ref.stream("host", form, state, n)
        got, st_got, rounds = rng_ref.stream("double", form, state, n)
        np.testing.assert_array_equal(host, want)
        assert st_host == st_want == st_got and rounds <= 4
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        rel = err / np.maximum(np.abs(want.astype(np.float64)), np.finfo(np.float32).tiny)
        print("%s: %.4f %% of %d values differ from std::log(float)'s; largest relative difference %.3f u (bound %.3f u)"
              % (form, 100.0 * np.mean(got != want), n, rel.max() / rng_ref.U, rng_ref.VALUE_REL / rng_ref.U))
        assert np.all(err <= rng_ref.VALUE_REL * np.abs(want.astype(np.float64)))


def test_numpy_generate_noise_equals_the_compiled_header():
    """rng_ref.noise_rows (the yardstick of the GPU tests where the reference cannot be asked) against what the sigma-pattern
    cases of the selftest prove about noise6_to_state13: here only its own consistency — zero sigmas draw nothing."""
    z, _, _ = rng_ref.stream("std", "fresh", 4242, 3 * 5)
    rows, zs = rng_ref.noise_rows(z, [1, 2, 3, 0.1, 0.2, 0.3], [0.5, 0, 0.25, 0, 0, 0.125], 5)
    f = np.float32
    np.testing.assert_array_equal(rows[:, 1], f(2))
    np.testing.assert_array_equal(rows[:, 10:12], 0)
    np.testing.assert_array_equal(rows[:, 0], z.reshape(5, 3)[:, 0] * f(0.5) + f(1))
    np.testing.assert_array_equal(rows[:, 12], (z.reshape(5, 3)[:, 2] * f(0.125) + f(0.3)) - f(0.3))
    np.testing.assert_allclose(np.linalg.norm(rows[:, 3:7], axis=1), 1.0, atol=1e-6)
