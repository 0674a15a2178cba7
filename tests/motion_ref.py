"""A float32 numpy restatement of the reference's between-scan models (what mcl_3dl_amd/csrc/motion_kernels.h computes), for
tests/test_motion_cpu.py and tests/test_gpu_resident_motion.py. Every float expression is evaluated in float32 in the reference's
order; a double step is written as one. The transcendentals come in two forms:
  * host=True   — the host libm's float functions through ctypes (acosf / sinf / cosf / expf): what the library's host code and
                  the reference compute on this box;
  * host=False  — the double function rounded to float: what the device computes ("Numerics")."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("acosf", "sinf", "cosf", "expf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]


def _vec(fn_host, fn_dbl, host):
    if host:
        f = getattr(_libm, fn_host)
        return lambda x: np.array([f(float(v)) for v in np.ravel(x)], F).reshape(np.shape(x))
    return lambda x: F(fn_dbl(np.asarray(x, np.float64))) if np.ndim(x) == 0 else fn_dbl(np.asarray(x, np.float64)).astype(F)


def funcs(host):
    return dict(acos=_vec("acosf", np.arccos, host), sin=_vec("sinf", np.sin, host), cos=_vec("cosf", np.cos, host),
                exp=_vec("expf", np.exp, host))


def qmul(a, q):
    """Quat::operator*(Quat) (quat.h:131-138) on [..., 4] float32 arrays {x, y, z, w}."""
    ax, ay, az, aw = (a[..., k] for k in range(4))
    qx, qy, qz, qw = (q[..., k] for k in range(4))
    return np.stack([aw * qx + ax * qw + ay * qz - az * qy,
                     aw * qy + ay * qw + az * qx - ax * qz,
                     aw * qz + az * qw + ax * qy - ay * qx,
                     aw * qw - ax * qx - ay * qy - az * qz], -1).astype(F)


def qrot(q, v):
    """Quat::operator*(Vec3): q (x) (v, 0) (x) conj(q)."""
    qv = np.concatenate([v, np.zeros(v.shape[:-1] + (1,), F)], -1)
    c = np.concatenate([-q[..., :3], q[..., 3:]], -1)
    return qmul(qmul(q, qv), c)[..., :3]


def qdot(q):
    return ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]


def recip(d):
    """float(1.0 / double(d))"""
    return (1.0 / np.asarray(d, np.float64)).astype(F)


def qnormalized(q):
    s = recip(np.sqrt(qdot(q)))
    return (q * s[..., None]).astype(F)


def qinv(q):
    s = recip(qdot(q))
    c = np.concatenate([-q[..., :3], q[..., 3:]], -1)
    return (c * s[..., None]).astype(F)


def vdot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def vnorm(a):
    return np.sqrt(vdot(a, a)).astype(F)


def normal_consts(sigma):
    """NormalLikelihood<float>(sigma) (nd.h:46-48)"""
    sigma = F(sigma)
    a = F(1.0 / np.sqrt(2.0 * np.pi * float(sigma) * float(sigma)))
    sq2 = F(float(F(sigma * sigma)) * 2.0)
    return a, sq2


def normal_likelihood(a, sq2, x, host=False):
    e = ((-x) * x / sq2).astype(F)
    return (a * funcs(host)["exp"](e)).astype(F)


def motion_step(prev7, cur7, time_diff, lin_tc, ang_tc):
    """setOdoms (motion_prediction_model_differential_drive.h:46-54) on the host, + the decay factors."""
    prev7, cur7 = np.asarray(prev7, F), np.asarray(cur7, F)
    pinv = qinv(prev7[3:7])
    t = qrot(pinv, (cur7[:3] - prev7[:3]).astype(F))
    rq = qmul(pinv, cur7[3:7])
    w = rq[3]
    if abs(float(w)) >= 1.0 - 0.000001:
        ang = F(0.0)
    else:
        ang = F(float(funcs(True)["acos"](w)) * 2.0)
        if ang > np.pi:
            ang = F(float(ang) - 2.0 * np.pi)
    td = F(time_diff)
    dl = F(1.0 - float(F(td / F(lin_tc))))
    da = F(1.0 - float(F(td / F(ang_tc))))
    return dict(t=t, rq=rq, t_norm=vnorm(t), ang=ang, decay_lin=dl, decay_ang=da)


def quat_axis_z(ang, host=False):
    fn = funcs(host)
    h = (ang / F(2)).astype(F)
    s, c = fn["sin"](h), fn["cos"](h)
    z = np.zeros_like(s)
    q = np.stack([F(0) * s, F(0) * s, F(1) * s, c], -1).astype(F)
    return qnormalized(q)


def predict(state13, noise4, m, host=False):
    """MotionPredictionModelDifferentialDrive::predict (:56-67) on every particle; returns the new [n, 13] states."""
    s = np.asarray(state13, F)
    nz = np.zeros((len(s), 4), F) if noise4 is None else np.asarray(noise4, F)
    nll, nla, nal, naa = (nz[:, k] for k in range(4))
    f = (1.0 + nll.astype(np.float64)).astype(F)
    diff = (m["t"][None, :] * f[:, None]).astype(F)
    diff = diff + np.stack([nal * m["ang"], np.zeros_like(nal), np.zeros_like(nal)], -1)
    lin = s[:, 7:10] + (diff - m["t"][None, :])
    rot = s[:, 3:7]
    pos = s[:, :3] + qrot(rot, diff)
    yaw = nla * m["t_norm"] + naa * m["ang"]
    r = qnormalized(qmul(qmul(quat_axis_z(yaw, host), rot), np.broadcast_to(m["rq"], rot.shape)))
    ang = s[:, 10:13] + np.stack([np.zeros_like(yaw), np.zeros_like(yaw), yaw], -1)
    lin = lin * m["decay_lin"]
    ang = ang * m["decay_ang"]
    return np.concatenate([pos, r, lin, ang], -1).astype(F)


def state_plus(state13, noise13):
    """State6DOF::operator+ (state_6dof.h:249-260); the result's odometry noise is 0."""
    s, a = np.asarray(state13, F), np.asarray(noise13, F)
    o = (s + a).astype(F)
    o[:, 3:7] = qmul(a[:, 3:7], s[:, 3:7])
    return o


def odom_factor(state13, sigma, host=False):
    a, sq2 = normal_consts(sigma)
    return normal_likelihood(a, sq2, vnorm(np.asarray(state13, F)[:, 7:10]), host)


def imu_likelihood(state13, acc, acc_var, host=False):
    """ImuMeasurementModelGravity::measure (imu_measurement_model_gravity.h:50-56) per particle."""
    s = np.asarray(state13, F)
    acc = np.asarray(acc, F)
    e = qrot(qinv(s[:, 3:7]), np.broadcast_to(np.array([0, 0, 1], F), (len(s), 3)))
    c = (vdot(e, np.broadcast_to(acc, e.shape)) / (vnorm(acc) * vnorm(e))).astype(F)
    with np.errstate(invalid="ignore"):
        diff = funcs(host)["acos"](c)
    a, sq2 = normal_consts(acc_var)
    with np.errstate(invalid="ignore", under="ignore"):
        return normal_likelihood(a, sq2, diff, host)
