"""tests/moments_ref.py against the oracle (the reference's pf.h + state_6dof.h when oracle/_ref is built, the plain-C port
otherwise) before tests/test_gpu_moments_exact.py trusts it, and the precondition of every case that file runs — no GPU needed.

The oracle adds in float, sequentially; the restatement adds the same terms exactly. With n terms the recurrence is off by at most
n * 2^-24 * sum |t| (first order; moments_ref.float_sequential_bound), so the oracle's quotients sum / sum w must lie within
|a| / b * (ea / |a| + eb / b + 2^-23) of the exact ones (the two sums' bounds, the rounding of either sum's exact value to float is
inside them, and the float division). The weights add up to 0.98: pf::expectation(pass_ratio = 1) and pf::covariance stop once
their running sum exceeds 1 (pf.h:280-293, 308-320), which a float recurrence over weights that add up to 1 may do early."""
import numpy as np
import pytest

import moments_ref as mo
from oracle import pyoracle

F, D = mo.F, mo.D


def inputs(n, seed):
    poses = mo.scene_poses(n, seed=seed)
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.2, 1.0, n)
    w = (0.98 * w / w.sum()).astype(F)
    return poses, w, rng.uniform(0.25, 1.0, n).astype(F)


def quotient_bound(a, ea, b, eb):
    return np.abs(a) / b * (ea / np.maximum(np.abs(a), 1e-300) + eb / b + 2.0 ** -23)


def test_one_particle_is_the_oracle_bit_for_bit(oracle_kind):
    o = pyoracle.Oracle(oracle_kind)
    poses, _, bias = inputs(1, 21)
    for w in (F(1.0), F(0.37)):
        for b in (None, bias):
            terms, im, ib = mo.moment_terms(poses, [w], b)
            want, wim, wib = o.expectation(poses, [w], b)
            got, _ = mo.moments_finish(mo.exact_sums(terms))
            np.testing.assert_array_equal(got, want)
            assert (im, ib) == (wim, wib) == (0, 0)
        want_cov, want_mean = o.covariance(poses, [w])
        got = mo.covariance_finish(mo.exact_sums(mo.cov_terms(poses, [w], want_mean, host=True)))
        np.testing.assert_array_equal(got, want_cov)
        assert np.any(want_cov != 0)  # (the mean's rotation is Quat(front, up), not the particle's: the differences are not 0)


@pytest.mark.parametrize("n", [2, 64, 1000])
def test_float_sequential_sums_lie_within_their_bound_of_the_exact_ones(oracle_kind, n):
    o = pyoracle.Oracle(oracle_kind)
    poses, w, bias = inputs(n, 22 + n)
    for b in (None, bias):
        terms, im, ib = mo.moment_terms(poses, w, b)
        want, wim, wib = o.expectation(poses, w, b)
        assert (im, ib) == (wim, wib)
        # the recurrence itself, restated: the same bits (terms and host arithmetic are the reference's)
        np.testing.assert_array_equal(mo.moments_finish(mo.float_sequential_sums(terms))[0], want)
        s, e = mo.exact_sums(terms), mo.float_sequential_bound(terms)
        err = np.abs(want[:3].astype(D) - s[1:4] / s[0])
        bound = quotient_bound(s[1:4], e[1:4], s[0], e[0])
        print("n %d position: error / bound %.3g" % (n, (err / bound).max()))
        assert np.all(err <= bound)
        got, _ = mo.moments_finish(s)
        angle = mo.quat_angle(got[3:], want[3:])
        print("n %d rotation: %.3g rad" % (n, angle))
        assert angle < 5e-4 and abs(np.linalg.norm(got[3:].astype(D)) - 1.0) < 1e-6
    want_cov, want_mean = o.covariance(poses, w)
    terms = mo.cov_terms(poses, w, want_mean, host=True)
    np.testing.assert_array_equal(mo.covariance_finish(mo.float_sequential_sums(terms)), want_cov)
    s, e = mo.exact_sums(terms), mo.float_sequential_bound(terms)
    worst = 0.0
    for i, (j, k) in enumerate(mo.PAIRS):
        err = abs(float(want_cov[j, k]) - s[i] / s[21])
        bound = quotient_bound(s[i], e[i], s[21], e[21])
        worst = max(worst, err / bound)
        assert err <= bound, (j, k, err, bound)
        assert want_cov[k, j] == want_cov[j, k]
    print("n %d covariance: error / bound %.3g" % (n, worst))


def test_arg_maxima_with_ties_and_a_bias_that_moves_the_biased_one(oracle_kind):
    o = pyoracle.Oracle(oracle_kind)
    poses = mo.scene_poses(300, seed=23)
    w = np.full(300, 0.001, F)
    w[[17, 130, 131, 299]] = 0.05  # four equal maxima: the reference keeps the first (strict <)
    bias = np.ones(300, F)
    bias[17] = 0.5                 # maxBiased then moves to the next one
    for b, want in ((None, (17, 17)), (bias, (17, 130))):
        _, im, ib = mo.moment_terms(poses, w, b)
        _, wim, wib = o.expectation(poses, w, b)
        assert (im, ib) == (wim, wib) == want
    bias[[17, 130, 131]] = 0.25    # ... and to the last
    assert mo.moment_terms(poses, w, bias)[1:] == o.expectation(poses, w, bias)[1:] == (17, 299)


def test_the_finish_functions_are_the_library_s_host_arithmetic():
    """mcl3dl_hip_moments_finish / _covariance_finish are pure host functions: the restatement equals them without a GPU."""
    import ctypes as C
    from mcl_3dl_amd import capi
    lib = capi.load_library()
    rng = np.random.default_rng(24)
    for trial in range(200):
        rec = np.zeros(16, D)
        q = rng.normal(0, 1, 4)
        q = (q / np.linalg.norm(q)).astype(F)[None]
        scale = rng.uniform(0.3, 1.0)
        rec[0] = scale
        rec[1:4] = rng.normal(0, 3, 3) * scale
        rec[4:7] = mo.mr.qrot(q, np.array([[1, 0, 0]], F))[0].astype(D) * scale * rng.uniform(0.7, 1.0)
        rec[7:10] = mo.mr.qrot(q, np.array([[0, 0, 1]], F))[0].astype(D) * scale * rng.uniform(0.7, 1.0)
        rec[:10] *= 1.0 + rng.uniform(-1e-9, 1e-9, 10)  # (sums are doubles, not floats)
        rec[10], rec[11], rec[12], rec[13] = 0.5, 7.0, 0.25, 9.0
        mean = np.zeros(7, F)
        total, im, ib = C.c_float(0), C.c_int64(0), C.c_int64(0)
        off = np.array([1000], np.uint64)
        assert lib.mcl3dl_hip_moments_finish(capi._ptr(rec), 1, capi._ptr(off), capi._ptr(mean), C.byref(total), C.byref(im),
                                             C.byref(ib)) == 0
        want, want_total = mo.moments_finish(rec)
        np.testing.assert_array_equal(mean, want)
        assert float(total.value) == want_total and (im.value, ib.value) == (1007, 1009)
        s22 = np.concatenate([rng.normal(0, 1, 21) * scale, [scale]])
        cov = np.zeros((6, 6), F)
        assert lib.mcl3dl_hip_covariance_finish(capi._ptr(s22), capi._ptr(cov)) == 0
        np.testing.assert_array_equal(cov, mo.covariance_finish(s22))


@pytest.mark.parametrize("name,build,moments,covariance", mo.CASES, ids=[c[0] for c in mo.CASES])
def test_sentinel_condition_of_every_gpu_case(name, build, moments, covariance):
    case = build()
    worst = case.check(moments, covariance)
    print("%s: a lost sentinel moves a sum by at least %.3g bounds" % (name, worst))
    assert sorted(case.marks) == mo.sentinels(case.m)
