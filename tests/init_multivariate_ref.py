"""Reference side of mcl3dl_hip_noise_transform6 and mcl3dl_hip_group_init_drawn_multivariate (mcl_3dl_amd/csrc/noise_transform.h,
rng_kernels.h: rng_multivariate_state_kernel): the definition of the transform restated in numpy fp64, the stand-alone program
that compiles the header itself (tests/cpp/noise_transform_check.cpp), MultivariateNoiseGenerator::operator() and
State6DOF::generateNoise restated in float32 numpy, and the bound between rows built on the standard library's stream and rows
built on the device's (whose polar logarithm is taken in double). Eigen is no part of any of it: the transform is this project's own
definition, and the six-term product is summed left to right (the kernel's comment).

THE ROW BOUND, term by term, in the manner of tests/rng_ref.py (u = 2^-24; a rounding moves a value v by at most u |v|). Both sides
take the same accept / reject decisions; a value r_j = z_j * 1 + 0 is exact behind z_j, so by rng_ref's VALUE_REL

    |d r_j|           <= 6u |r_j|
    T_ij r_j          one rounding on either side:                                 (6u + 2u) |T_ij r_j| = 8u |T_ij r_j|
    s_i, six terms    five additions, one rounding each on either side, every partial sum at most A_i = sum_j |T_ij r_j|:
                                                                                   8u A_i + 10u A_i = 18u A_i
    org_i = mean_i + s_i   one rounding on either side:                            |d org_i| <= 18u A_i + 2u |org_i|

generateNoise copies org_0..2 to columns 0-2 and 7-9, stores org_3..5 - mean_3..5 in 10-12 (one more rounding on either side:
+ 2u |value|) and forms rot = Quat(rpy) by setRPY, rng_ref's 6 dh + 18u with dh = max |d org_3..5| / 2. All of it times
rng_ref.SECOND_ORDER. With reset_odom_integ columns 7-12 are 0 on both sides: bound 0.

THE T T^T BOUND (transform_bound). With C the float-cast covariance, C = V diag(lambda) V^T up to the fp64 Jacobi's residual
(some 1e-16 |C|_F), and T_ik = V_ik sqrt(lambda_k) (1 + d_ik), |d_ik| <= u (formed in double, rounded to float once):

    (T T^T)_ij - C_ij = sum_k V_ik V_jk lambda_k ((1 + d_ik)(1 + d_jk) - 1)
    |...|            <= (2u + u^2) sum_k |V_ik sqrt(lambda_k)| |V_jk sqrt(lambda_k)| <= (2u + u^2) sqrt(C_ii C_jj)   (Cauchy-Schwarz)

A third u covers u^2, the Jacobi residual and a caller who compares against the double matrix whose diagonal the float cast moved
by u: 3u sqrt(C_ii C_jj). Where an eigenvalue lambda_k in [-2^-23 |C|_F, 0) was set to 0, V diag(lambda') V^T differs from C by
|lambda_k| |V_ik V_jk| <= 2^-23 |C|_F in every entry: that much is added, and only then."""
import os
import subprocess

import numpy as np

import landmark_ref as lr
import rng_ref

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
U = rng_ref.U
SWEEPS = 30

# the mean pose of test_init_drawn_at_a_mean_pose
MEAN_RPY = np.array([[0.3, -0.2, 1.1]], F)
MEAN7 = np.concatenate([[1.5, -2.0, 0.25], rng_ref.set_rpy(MEAN_RPY)[0]]).astype(F)
# the engine state and particle count at which the shared stream of 6 n_p values needs a second round (3 accepted attempts are
# asked of 8: fewer than 3 are accepted behind this state; found by running `stream host shared` over the states from 1 up)
SECOND_ROUND = (318, 1)
# the distribution check: particle count and engine state, the same in the CPU test (the numpy reference on the standard library's
# stream) and in the GPU test
STAT_N = 4096
STAT_STATE = rng_ref.minstd_seed(20241021)


def mean6_of(mean7):
    """host_rng.h: rng_mean6 — Quat::getRPY of the mean's rotation, atan2 / asin in double rounded to float."""
    mean7 = np.asarray(mean7, F)
    t0, t1, t2, t3, t4 = (t.astype(np.float64) for t in lr.rpy_terms(mean7[None, 3:7])[:5])
    return np.concatenate([mean7[:3], [np.arctan2(t3, t4)[0], np.arcsin(t2)[0], np.arctan2(t1, t0)[0]]]).astype(F)


def spd_covariance():
    """A full symmetric positive definite covariance with every entry non-zero: A A^T + a small diagonal."""
    rng = np.random.default_rng(20240611)
    a = rng.normal(0.0, 1.0, (6, 6)) * np.array([0.3, 0.2, 0.1, 0.03, 0.02, 0.08])[:, None]
    return a @ a.T + np.diag([1e-3, 1e-3, 1e-4, 1e-5, 1e-5, 1e-4])


def float_cast(cov36):
    """The matrix the transform is defined on: entries cast to float, the lower triangle mirrored; float64 [6, 6]."""
    with np.errstate(over="ignore"):
        c = np.asarray(cov36, np.float64).reshape(6, 6).astype(F).astype(np.float64)
    return np.tril(c) + np.tril(c, -1).T


def noise_transform_ref(cov36):
    """noise_transform.h restated: (T float32 [6, 6], eigenvalues float64 [6] behind the clamp, number clamped). ValueError where
    the header returns -3."""
    c = np.asarray(cov36, np.float64).reshape(6, 6)
    with np.errstate(over="ignore"):
        finite = np.all(np.isfinite(c.astype(F)))
    if not finite:
        raise ValueError("not finite as floats")
    a = float_cast(c)
    frob = float(np.sqrt(np.sum(a * a)))
    v = np.eye(6)
    for _ in range(SWEEPS):
        if not np.any(a[np.triu_indices(6, 1)]):
            break
        for p in range(5):
            for q in range(p + 1, 6):
                if a[p, q] == 0.0:
                    continue
                with np.errstate(over="ignore"):
                    theta = (a[q, q] - a[p, p]) / (2.0 * a[p, q])
                    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c_ = 1.0 / np.sqrt(t * t + 1.0)
                s_ = t * c_
                a[p, p] -= t * a[p, q]
                a[q, q] += t * a[p, q]
                a[p, q] = a[q, p] = 0.0
                for r in range(6):
                    if r == p or r == q:
                        continue
                    rp, rq = a[r, p], a[r, q]
                    a[r, p] = a[p, r] = c_ * rp - s_ * rq
                    a[r, q] = a[q, r] = s_ * rp + c_ * rq
                vp, vq = v[:, p].copy(), v[:, q].copy()
                v[:, p] = c_ * vp - s_ * vq
                v[:, q] = s_ * vp + c_ * vq
    lam = np.diag(a).copy()
    order = np.argsort(lam, kind="stable")
    lam = lam[order]
    low = -np.ldexp(frob, -23)
    if np.any(lam < low):
        raise ValueError("eigenvalue %g below %g" % (lam.min(), low))
    clamped = int(np.count_nonzero(lam < 0.0))
    lam = np.where(lam < 0.0, 0.0, lam)
    T = np.zeros((6, 6), F)
    for k, col in enumerate(order):
        big = int(np.argmax(np.abs(v[:, col])))  # the first of equal maxima
        sign = -1.0 if v[big, col] < 0.0 else 1.0
        T[:, k] = (sign * v[:, col] * np.sqrt(lam[k])).astype(F)
    return T, lam, clamped


def transform_bound(cov36, clamped):
    """Entrywise bound [6, 6] on |T T^T - float_cast(cov36)| (module docstring)."""
    c = float_cast(cov36)
    d = np.sqrt(np.abs(np.diag(c)))
    b = 3 * U * np.outer(d, d)
    if clamped:
        b = b + 2.0 ** -23 * np.sqrt(np.sum(c * c))
    return b


_exe = None


def check_exe():
    """tests/cpp/noise_transform_check.cpp, compiled once per process the way rng_ref.emul_exe compiles its program."""
    global _exe
    if _exe is None:
        import atexit
        import shutil
        import tempfile
        d = tempfile.mkdtemp(prefix="noise_transform_check_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "noise_transform_check.bin")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "cpp", "noise_transform_check.cpp")],
                       check=True)
        _exe = exe
    return _exe


def transform_program(cov36):
    """The header through the stand-alone program: (rc, T float32 [6, 6] or None, eigenvalues float32 [6] or None, clamped, msg)."""
    exe = check_exe()
    d = os.path.dirname(exe)
    src, out = os.path.join(d, "cov_%d.bin" % os.getpid()), os.path.join(d, "t_%d.bin" % os.getpid())
    np.asarray(cov36, np.float64).reshape(36).tofile(src)
    txt = subprocess.run([exe, "transform", src, out], check=True, capture_output=True, text=True, timeout=60).stdout
    head, msg = txt.strip().split(" msg=", 1)
    fields = dict(kv.split("=") for kv in head.split())
    rc, clamped = int(fields["rc"]), int(fields["clamped"])
    os.remove(src)
    if rc != 0:
        return rc, None, None, clamped, msg
    v = np.fromfile(out, F)
    os.remove(out)
    assert len(v) == 42
    return rc, v[:36].reshape(6, 6), v[36:], clamped, msg


def particles_std(state, n):
    """One std::normal_distribution<float>(0, 1) per particle, called six times, n particles on one engine from `state`:
    (values [6 n], engine state behind)."""
    exe = check_exe()
    out = os.path.join(os.path.dirname(exe), "p_%d.bin" % os.getpid())
    txt = subprocess.run([exe, "particles", str(int(state)), str(int(n)), out], check=True, capture_output=True, text=True,
                         timeout=60).stdout
    v = np.fromfile(out, F)
    os.remove(out)
    assert len(v) == 6 * n
    return v, int(txt.split("=")[1])


def multivariate_rows(z, mean6, T, n, reset):
    """MultivariateNoiseGenerator::operator() and State6DOF::generateNoise over the N(0, 1) values z (6 n of one shared stream) in
    float32, the product summed left to right: rows [n, 13] and A [n, 6], A_i = sum_j |T_ij r_j| (float64)."""
    mean6, T = np.asarray(mean6, F), np.asarray(T, F).reshape(6, 6)
    r = np.asarray(z, F).reshape(n, 6) * F(1.0) + F(0.0)
    org = np.zeros((n, 6), F)
    A = np.zeros((n, 6), np.float64)
    for i in range(6):
        s = T[i, 0] * r[:, 0] + T[i, 1] * r[:, 1]
        for j in range(2, 6):
            s = s + T[i, j] * r[:, j]
        assert s.dtype == F
        org[:, i] = mean6[i] + s
        A[:, i] = np.abs(T[i].astype(np.float64) * r.astype(np.float64)).sum(axis=1)
    rows = np.zeros((n, 13), F)
    rows[:, 0:3] = org[:, 0:3]
    rows[:, 3:7] = rng_ref.set_rpy(org[:, 3:6])
    if not reset:
        rows[:, 7:10] = org[:, 0:3]
        rows[:, 10:13] = org[:, 3:6] - mean6[3:6]
    return rows, A


def row_bounds(rows, A, mean6, reset, same_stream=False):
    """Elementwise bound [n, 13] between a row built on the `std` stream and one built on the device's (module docstring). `rows`
    must come from multivariate_rows with reset = False or True as given. same_stream: both sides use the same values, only the
    double-precision cos / sin of setRPY may round differently: 0 everywhere but 18u on the quaternion (dh = 0)."""
    n = len(rows)
    b = np.zeros((n, 13), np.float64)
    if same_stream:
        b[:, 3:7] = 18 * U * rng_ref.SECOND_ORDER
        return b
    mean6 = np.asarray(mean6, np.float64)
    rows64 = rows.astype(np.float64)
    # org_3..5 from the quaternion-free columns where they exist; with reset they are gone, and |org| <= |mean| + A bounds them
    if reset:
        org = np.concatenate([np.abs(rows64[:, 0:3]), np.abs(mean6[3:6]) + A[:, 3:6]], axis=1)
    else:
        org = np.abs(np.concatenate([rows64[:, 0:3], rows64[:, 10:13] + mean6[3:6]], axis=1))
    dorg = 18 * U * A + 2 * U * org
    b[:, 0:3] = dorg[:, 0:3]
    b[:, 3:7] = (6 * (dorg[:, 3:6].max(axis=1) / 2) + 18 * U)[:, None]
    if not reset:
        b[:, 7:10] = dorg[:, 0:3]
        b[:, 10:13] = dorg[:, 3:6] + 2 * U * np.abs(rows64[:, 10:13])
    return b * rng_ref.SECOND_ORDER


def covariance_within_six_standard_errors(rows, cov36):
    """The distribution check: the sample covariance of (columns 0-2, columns 10-12) about its own mean against the float-cast
    covariance, entry by entry, in units of se_ij = sqrt((c_ii c_jj + c_ij^2) / n). Returns the largest |deviation| / se."""
    x = np.concatenate([rows[:, 0:3], rows[:, 10:13]], axis=1).astype(np.float64)
    n = len(x)
    c = float_cast(cov36)
    x = x - x.mean(axis=0)
    got = x.T @ x / n
    d = np.diag(c)
    se = np.sqrt((np.outer(d, d) + c * c) / n)
    return float(np.max(np.abs(got - c) / se))
