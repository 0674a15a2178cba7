"""CPU tests of the normal-weighted sampler: mcl3dl_hip_sampler_normal_direction (a pure host function of the library:
setParticleStatistics + the max_weight ladder + fpc_local, point_cloud_sampler_with_normal.h:75-89, 110-129) against numpy, its
error cases, and the numpy oracle of tests/sampler_normal_ref.py against the analytic weights of the upstream test's walls."""
import ctypes as C

import numpy as np
import pytest

import sampler_normal_ref as snr
from mcl_3dl_amd import capi

F = np.float32


def aligned(got, want):
    """`got` with the sign that matches `want` (an eigenvector's sign is arbitrary; the weights use |n . fpc_local|)."""
    got = np.asarray(got, np.float64)
    return got if np.dot(got, want) >= 0 else -got


@pytest.mark.parametrize("params,want_max_weight", snr.UPSTREAM_PARAMETER_SETS)
def test_direction_upstream_parameter_sets(params, want_max_weight):
    mean, cov = snr.upstream_statistics()
    fpc, mw, ratio = capi.sampler_normal_direction(mean, cov, *params)
    want_fpc, want_mw, want_ratio = snr.direction(mean, cov, *params)
    print("ratio %.17g (numpy %.17g), max_weight %.17g (numpy %.17g), fpc_local %s" % (ratio, want_ratio, mw, want_mw, fpc))
    assert abs(ratio - want_ratio) <= 1e-12 * want_ratio
    assert abs(mw - want_mw) <= 1e-12 * want_mw
    # upstream's own comments: 10, 1 and 3 (the covariance is held in floats: the ratio is 5 to 7 digits)
    assert abs(mw - want_max_weight) <= 1e-6
    np.testing.assert_allclose(aligned(fpc, want_fpc), want_fpc, rtol=0, atol=1e-6)
    # the first principal component in the robot's frame is its x axis
    np.testing.assert_allclose(np.abs(fpc), [1.0, 0.0, 0.0], rtol=0, atol=1e-6)


def random_cases():
    """A dozen random covariances with distinct eigenvalues, full 6 x 6 (only the position block matters), random unit
    quaternions and thresholds; the ratio stays 1e-3 away from both thresholds so that the branch is not a coin toss."""
    rng = np.random.default_rng(20260)
    out = []
    while len(out) < 12:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        lam = np.sort(rng.uniform(0.01, 1.0, 3)) * np.array([1.0, 2.0, 6.0])
        cov = np.zeros((6, 6))
        cov[:3, :3] = q @ np.diag(lam) @ q.T
        cov[3:, 3:] = np.diag(rng.uniform(0.01, 0.1, 3))
        cov[:3, 3:] = rng.normal(0, 0.01, (3, 3))
        cov[3:, :3] = cov[:3, 3:].T
        cov = cov.astype(F)
        quat = rng.normal(size=4)
        quat /= np.linalg.norm(quat)
        mean = np.concatenate([rng.uniform(-10, 10, 3), quat]).astype(F)
        low = float(rng.uniform(1.2, 2.5))
        params = (low, low + float(rng.uniform(0.3, 1.5)), float(rng.uniform(2.0, 10.0)))
        _, _, ratio = snr.direction(mean, cov, *params)
        w = np.linalg.eigvalsh(np.tril(np.abs(cov[:3, :3].astype(np.float64))) + np.tril(np.abs(cov[:3, :3].astype(np.float64)), -1).T)
        if min(abs(ratio - params[0]), abs(ratio - params[1])) < 1e-3 or w[0] <= 0 or min(np.diff(w)) < 0.05 * w[2]:
            continue
        out.append((mean, cov, params))
    return out


def test_direction_random_covariances():
    branches = set()
    for mean, cov, params in random_cases():
        fpc, mw, ratio = capi.sampler_normal_direction(mean, cov, *params)
        want_fpc, want_mw, want_ratio = snr.direction(mean, cov, *params)
        branches.add(0 if want_ratio < params[0] else (2 if want_ratio > params[1] else 1))
        assert abs(ratio - want_ratio) <= 1e-12 * want_ratio, (ratio, want_ratio)
        assert abs(mw - want_mw) <= 1e-12 * want_mw, (mw, want_mw)
        np.testing.assert_allclose(aligned(fpc, want_fpc), want_fpc, rtol=0, atol=1e-6)
    assert branches == {0, 1, 2}  # all three rungs of the ladder were taken


def test_direction_reads_the_lower_triangle_and_absolute_values():
    mean, cov = snr.upstream_statistics()
    base = capi.sampler_normal_direction(mean, cov, 2.0, 8.0, 5.0)
    # std::abs of every entry: the sign of the off-diagonal term does not matter
    flipped = cov.copy()
    flipped[0, 1] = -flipped[0, 1]
    flipped[1, 0] = -flipped[1, 0]
    other = capi.sampler_normal_direction(mean, flipped, 2.0, 8.0, 5.0)
    np.testing.assert_array_equal(base[0], other[0])
    assert base[1:] == other[1:]
    # Eigen::SelfAdjointEigenSolver reads the lower triangle only
    upper = cov.copy()
    upper[0, 1] = 123.0
    other = capi.sampler_normal_direction(mean, upper, 2.0, 8.0, 5.0)
    np.testing.assert_array_equal(base[0], other[0])
    assert base[1:] == other[1:]


def test_direction_rejects_null_and_non_finite_arguments():
    lib = capi.load_library()
    mean, cov = snr.upstream_statistics()
    fpc = np.zeros(3, F)
    mw, ratio = C.c_double(0), C.c_double(0)

    def call(m=mean, c=cov, p=(2.0, 4.0, 10.0), out=fpc, pmw=C.byref(mw), pr=C.byref(ratio)):
        return lib.mcl3dl_hip_sampler_normal_direction(capi._ptr(m), capi._ptr(c), p[0], p[1], p[2], capi._ptr(out), pmw, pr)

    assert call() == 0
    assert call(pr=None) == 0                      # the ratio is optional
    assert call(m=None) == -3 and call(c=None) == -3 and call(out=None) == -3 and call(pmw=None) == -3
    for k in (3, 6):
        bad = mean.copy()
        bad[k] = np.nan
        assert call(m=bad) == -3
    for ij in ((0, 0), (2, 1)):
        bad = cov.copy()
        bad[ij] = np.inf
        assert call(c=bad) == -3
    for k in range(3):
        p = [2.0, 4.0, 10.0]
        p[k] = float("nan")
        assert call(p=tuple(p)) == -3
    with pytest.raises(ValueError):
        capi.sampler_normal_direction(mean[:6], cov)


def test_oracle_gives_the_walls_their_analytic_weights():
    cloud = snr.walls()
    assert cloud.shape == (800, 3) and cloud.dtype == F
    ref = snr.oracle(cloud, 0.4)
    # the figures the scene was chosen for: every point has a normal, well separated eigenvalues
    assert (int(ref["count"].min()), int(ref["count"].max())) == (56, 195)
    assert np.nanmin(ref["gap"]) >= 1e-2
    fpc = np.array([0.8, 0.6, 0.0], F)
    w = snr.weights(ref["normal"], fpc, 5.0)
    # the walls' normals are +-x and +-y: c is a component of fpc_local, as the float it is
    w1 = 1 + 4 * (1 - np.arccos(np.float64(fpc[0])) / (np.pi / 2))
    w2 = 1 + 4 * (1 - np.arccos(np.float64(fpc[1])) / (np.pi / 2))
    assert abs(w1 - 3.361338) < 1e-6 and abs(w2 - 2.638662) < 1e-6
    tol = snr.weight_tolerance(5.0)
    assert np.abs(w[:400] - w1).max() <= tol and np.abs(w[400:] - w2).max() <= tol
    assert abs(np.cumsum(w)[-1] - 400 * (w1 + w2)) <= 1e-9
    # along the first wall's normal the sum is 400 x 5 + 400 x 1 exactly
    w = snr.weights(ref["normal"], (1.0, 0.0, 0.0), 5.0)
    assert abs(np.cumsum(w)[-1] - 2400.0) <= 1e-9
