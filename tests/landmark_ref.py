"""A float32 numpy restatement of the two pose-reading models on resident particles (what mcl_3dl_amd/csrc/landmark_kernels.h
and the host side of mcl3dl_hip_group_measure_landmark / _expectation_jump_bias compute), built on tests/motion_ref.py's helpers:

  * jump_bias            bias_func of src/mcl_3dl.cpp:436-451: nl_lin(|pos - prev.pos|) * nl_ang(ang(rot * prev.rot^-1)) + 1e-6
  * landmark_likelihood  cbLandmark's measure_func (src/mcl_3dl.cpp:913-928): NormalLikelihoodNd<float, 6> (nd.h:60-80) over
                         {pos, getRPY(rot)} of s - measured
  * landmark_constants   NormalLikelihoodNd's constructor on the host: sigma(r, c) = float(cov36[6 c + r]), determinant and
                         inverse by LU with partial pivoting in double, each rounded to float once

As in motion_ref, host=True evaluates the transcendentals with the host libm's float functions (what the reference computes on
this box), host=False as the double function rounded to float (what the device computes).

The two bounds (derived, not measured) that tests/test_landmark_cpu.py and tests/test_gpu_landmark_bias.py share are here too.
Both sides of either comparison evaluate faithful functions of the SAME float arguments, so each transcendental differs by at most
one float ulp of its result:
  * landmark: x_3..5 = atan2 / asin / atan2 move by at most spacing(x_k) each, which moves the exponent e = -x^T S x / 2 by
    |((S + S^T) x / 2)_k| spacing(x_k); exp() and the product with a_ add 2^-23 relative; doubled.
  * bias: ang moves by at most one ulp, which moves nl_ang's exponent -ang^2 / sq2 by 2 |ang| / sq2 spacing(ang); two exp() and
    the product add 3 * 2^-23; doubled. (An angle folded by -2 pi carries the ulp of the unfolded value, up to 4.8e-7; with
    sq2_ang >= 2 * 1.03^2 that stays inside the constant term for every angle. The tests use the node's defaults, 2.0 and 1.57.)"""
import numpy as np

import motion_ref as mr

F = mr.F
_cf = mr.ctypes.c_float
mr._libm.asinf.restype, mr._libm.asinf.argtypes = _cf, [_cf]
mr._libm.atan2f.restype, mr._libm.atan2f.argtypes = _cf, [_cf, _cf]


def funcs(host):
    """motion_ref.funcs extended by asin and atan2."""
    fn = mr.funcs(host)
    fn["asin"] = mr._vec("asinf", np.arcsin, host)
    if host:
        fn["atan2"] = lambda y, x: np.array([mr._libm.atan2f(float(a), float(b)) for a, b in zip(np.ravel(y), np.ravel(x))],
                                            F).reshape(np.shape(y))
    else:
        fn["atan2"] = lambda y, x: np.arctan2(np.asarray(y, np.float64), np.asarray(x, np.float64)).astype(F)
    return fn


# ---- the pose-jump bias ------------------------------------------------------------------------------------------------------
def axis_angle(q, host=False):
    """Quat::getAxisAng (quat.h:226-239), the angle only, on [n, 4] float32 {x, y, z, w}."""
    w = np.asarray(q, F)[..., 3]
    zero = np.abs(w.astype(np.float64)) >= 1.0 - 0.000001
    with np.errstate(invalid="ignore"):
        ac = funcs(host)["acos"](np.where(zero, F(0), w).astype(F))
    ang = (ac.astype(np.float64) * 2.0).astype(F)
    fold = ang.astype(np.float64) > np.pi
    ang = np.where(fold, (ang.astype(np.float64) - 2.0 * np.pi).astype(F), ang).astype(F)
    return np.where(zero, F(0), ang).astype(F), fold & ~zero


def jump_bias(state13, prev7, var_dist, var_ang, host=False, parts=False):
    """probability_bias_ per particle; parts=True also returns (lin, ang, folded)."""
    s, prev7 = np.asarray(state13, F), np.asarray(prev7, F)
    lin = mr.vnorm((s[:, :3] - prev7[:3]).astype(F))
    q = mr.qmul(s[:, 3:7], np.broadcast_to(mr.qinv(prev7[3:7]), (len(s), 4)))
    ang, folded = axis_angle(q, host)
    a_l, sq2_l = mr.normal_consts(var_dist)
    a_a, sq2_a = mr.normal_consts(var_ang)
    with np.errstate(under="ignore"):
        prod = (mr.normal_likelihood(a_l, sq2_l, lin, host) * mr.normal_likelihood(a_a, sq2_a, ang, host)).astype(F)
    bias = (prod.astype(np.float64) + 1e-6).astype(F)
    return (bias, lin, ang, folded) if parts else bias


def jump_bias_bound(ang, var_ang):
    """Relative bound per particle (module docstring), in float64 from the restatement's own angles."""
    _, sq2 = mr.normal_consts(var_ang)
    ang = np.asarray(ang, F)
    return 2.0 * (2.0 * np.abs(ang.astype(np.float64)) / float(sq2) * np.spacing(np.abs(ang)).astype(np.float64)
                  + 3.0 * 2.0 ** -23)


# ---- the landmark model --------------------------------------------------------------------------------------------------------
def landmark_constants(cov36):
    """(a_, sigma_inv_ as [6, 6] float32) of NormalLikelihoodNd<float, 6>(sigma), sigma(r, c) = float(cov36[6 c + r]); the LU of
    mcl3dl_hip_group_measure_landmark step by step in Python floats (= C doubles). ValueError where the library returns -3."""
    cov = np.asarray(cov36, np.float64).reshape(36)
    if not np.all(np.isfinite(cov)):
        raise ValueError("non-finite covariance")
    with np.errstate(over="ignore"):
        sig = cov.astype(F)
    if not np.all(np.isfinite(sig)):
        raise ValueError("non-finite covariance")
    A = [[float(sig[6 * c + r]) for c in range(6)] for r in range(6)]
    perm = list(range(6))
    det = 1.0
    for k in range(6):
        p = k
        for i in range(k + 1, 6):
            if abs(A[i][k]) > abs(A[p][k]):
                p = i
        if A[p][k] == 0.0:
            raise ValueError("singular covariance")
        if p != k:
            A[k], A[p] = A[p], A[k]
            perm[k], perm[p] = perm[p], perm[k]
            det = -det
        for i in range(k + 1, 6):
            A[i][k] = A[i][k] / A[k][k]
            for j in range(k + 1, 6):
                A[i][j] = A[i][j] - A[i][k] * A[k][j]
    for k in range(6):
        det = det * A[k][k]
    with np.errstate(over="ignore"):
        det_f = F(det)
    if not det_f > 0:
        raise ValueError("covariance without a positive determinant")
    sinv = np.zeros((6, 6), F)
    for c in range(6):
        y, x = [0.0] * 6, [0.0] * 6
        for i in range(6):
            s = 1.0 if perm[i] == c else 0.0
            for j in range(i):
                s = s - A[i][j] * y[j]
            y[i] = s
        for i in range(5, -1, -1):
            s = y[i]
            for j in range(i + 1, 6):
                s = s - A[i][j] * x[j]
            x[i] = s / A[i][i]
        with np.errstate(over="ignore"):
            sinv[:, c] = np.array(x, np.float64).astype(F)
    if not np.all(np.isfinite(sinv)):
        raise ValueError("non-finite inverse")
    a = F(1.0 / (float((2.0 * np.pi) ** 3.0) * float(np.sqrt(det_f))))  # sqrt of a float is a float; det_f = inf: a = 0
    return a, sinv


def rpy_terms(q):
    """t0 .. t4 of Quat::getRPY (quat.h:191-199), and the unclamped double t2."""
    x, y, z, w = (np.asarray(q, F)[..., k] for k in range(4))
    ysq = (y * y).astype(F)
    d = np.float64
    t0 = (-2.0 * (ysq + z * z).astype(F).astype(d) + 1.0).astype(F)
    t1 = (2.0 * (x * y + w * z).astype(F).astype(d)).astype(F)
    t2d = -2.0 * (x * z - w * y).astype(F).astype(d)
    t2 = np.clip(t2d, -1.0, 1.0).astype(F)
    t3 = (2.0 * (y * z + w * x).astype(F).astype(d)).astype(F)
    t4 = (-2.0 * (x * x + ysq).astype(F).astype(d) + 1.0).astype(F)
    return t0, t1, t2, t3, t4, t2d


def state_minus(state13, measured7):
    """(diff.pos_, diff.rot_) of s - measured (state_6dof.h:262-274)."""
    s, m = np.asarray(state13, F), np.asarray(measured7, F)
    d = (s[:, :3] - m[:3]).astype(F)
    q = mr.qmul(np.broadcast_to(mr.qinv(m[3:7]), (len(s), 4)), s[:, 3:7])
    return d, q


def landmark_x(state13, measured7, host=False):
    """diff_vec of measure_func: {diff.pos_, diff.rot_.getRPY()} as [n, 6] float32."""
    d, q = state_minus(state13, measured7)
    t0, t1, t2, t3, t4, _ = rpy_terms(q)
    fn = funcs(host)
    return np.concatenate([d, np.stack([fn["atan2"](t3, t4), fn["asin"](t2), fn["atan2"](t1, t0)], -1)], -1).astype(F)


def normal_nd(a, sinv, x, host=False):
    """NormalLikelihoodNd::operator() (nd.h:72-75): y = -0.5f x, r = y^T sigma_inv, e = r x, sums sequential in float."""
    x = np.asarray(x, F)
    y = (F(-0.5) * x).astype(F)
    e = None
    for j in range(6):
        r = (y[:, 0] * sinv[0, j]).astype(F)
        for k in range(1, 6):
            r = (r + (y[:, k] * sinv[k, j]).astype(F)).astype(F)
        t = (r * x[:, j]).astype(F)
        e = t if e is None else (e + t).astype(F)
    with np.errstate(under="ignore"):
        return (a * funcs(host)["exp"](e)).astype(F)


def landmark_likelihood(state13, measured7, cov36, host=False):
    a, sinv = landmark_constants(cov36)
    return normal_nd(a, sinv, landmark_x(state13, measured7, host), host)


def landmark_bound(x, sinv):
    """Relative bound per particle (module docstring), in float64 from the restatement's own x."""
    x = np.asarray(x, F)
    S = np.asarray(sinv, np.float64)
    g = np.abs(0.5 * (x.astype(np.float64) @ (S + S.T)))  # |((S + S^T) x / 2)_k| per particle
    sp = np.spacing(np.abs(x)).astype(np.float64)
    return 2.0 * (np.sum(g[:, 3:6] * sp[:, 3:6], axis=1) + 2.0 ** -23)


def pf_measure(w, lik):
    """pf::measure (pf.h:252-279): float products, float sequential sum, restore unless sum > 0."""
    wn = (np.asarray(w, F) * np.asarray(lik, F)).astype(F)
    s = F(0)
    for v in wn:
        s = F(s + v)
    if not s > 0.0:
        return np.asarray(w, F).copy(), True
    return (wn / s).astype(F), False


# ---- upstream's known-answer test (test/src/test_landmark.cpp) ---------------------------------------------------------------
def kat_inputs(n=4096, seed=7):
    """4096 particles with y ~ N(2.0, 1.0), everything else 0, identity rotation; a landmark at y = 2.6 with variance 1.0 and
    1000 * 1000 on the other five axes. Upstream resamples and takes plain moments of the new cloud; the weighted moments under
    the new weights are what that cloud samples."""
    st = np.zeros((n, 13), F)
    st[:, 1] = np.random.default_rng(seed).normal(2.0, 1.0, n)
    st[:, 6] = 1.0
    cov = np.diag([1e6, 1.0, 1e6, 1e6, 1e6, 1e6]).reshape(36)
    return st, np.full(n, 1.0 / n, F), np.array([0, 2.6, 0, 0, 0, 0, 1], F), cov


def weighted_mean_var(y, w):
    y, w = np.asarray(y, np.float64), np.asarray(w, np.float64)
    mean = np.sum(w * y) / np.sum(w)
    return mean, np.sum(w * (y - mean) ** 2) / np.sum(w)
