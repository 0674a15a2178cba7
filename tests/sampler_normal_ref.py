"""The yardstick of the normal-weighted sampler's tests (mcl_3dl_amd/csrc/api_sampler.inl, sampler_kernels.h): the definition
of DESIGN.md 3.5.1 in plain numpy, the scenes, and a numpy restatement of the sampler's host-side direction / max_weight step.
Shared by tests/test_sampler_normal_cpu.py and tests/test_gpu_sampler_normal.py. pcl::NormalEstimation is not pinned by the
reference (no PCL in its tree, none in oracle/), so nothing here is reference-backed; the definition is restated, not measured.

  oracle      per point: neighbours decided in float32 in the expression order of mcl3dl_hip_radius_search
              (((dx dx) + dy dy) + dz dz < float32(r r), strict, the point itself included, non-finite points nobody's
              neighbour), moments in float64 about the query, numpy.linalg.eigh -> normal, neighbour count, relative gap
  weights     point_cloud_sampler_with_normal.h:142-155 in float64 from those normals
  direction   setParticleStatistics + the max_weight ladder + fpc_local (:75-89, 110-129) with numpy.linalg.eigh
  walls / room / far_pair   the scenes"""
import numpy as np

F = np.float32


def walls():
    """The upstream test's cloud (test_point_cloud_random_sampler_with_normal.cpp:77-105): two 20 x 20 walls at x = 20, the second
    turned about z by pi / 2. 800 points; rows [0, 400) are the first wall."""
    out = []
    ny, nz = np.meshgrid(np.arange(20), np.arange(20), indexing="ij")  # ny outer, nz inner
    base = np.stack([np.full(400, 20.0), (ny.ravel() - 10) * 0.05, (nz.ravel() - 10) * 0.05], axis=1).astype(F).astype(np.float64)
    for ang in (0.0, np.pi / 2):
        c, s = np.cos(ang), np.sin(ang)
        out.append(np.stack([c * base[:, 0] - s * base[:, 1], s * base[:, 0] + c * base[:, 1], base[:, 2]], axis=1).astype(F))
    return np.concatenate(out)


def room():
    """6105 points: a jittered floor, a wall, an oblique wall, a collinear pole, isolated points, a pair, an isotropic blob."""
    r = np.random.default_rng(5)
    g = np.arange(-3, 3, 0.1)
    P = []
    X, Y = np.meshgrid(g, g)
    n = X.size                                                             # floor
    P.append(np.c_[X.ravel() + r.uniform(-.03, .03, n), Y.ravel() + r.uniform(-.03, .03, n), r.normal(0, .005, n)])
    Yw, Zw = np.meshgrid(g, np.arange(0.1, 2, 0.1))
    n = Yw.size                                                            # wall x = 3
    P.append(np.c_[3 + r.normal(0, .005, n), Yw.ravel() + r.uniform(-.03, .03, n), Zw.ravel() + r.uniform(-.03, .03, n)])
    u = Yw.ravel() + r.uniform(-.03, .03, n)
    v = Zw.ravel() + r.uniform(-.03, .03, n)
    d = r.normal(0, .005, n)
    a = 0.6
    P.append(np.c_[np.cos(a) * d - np.sin(a) * u - 1.0, np.sin(a) * d + np.cos(a) * u + 6.0, v])   # oblique wall
    P.append(np.c_[np.full(15, 1.0), np.full(15, -5.0), np.arange(15) * 0.1])                      # pole: collinear
    P.append(np.c_[np.arange(8) * 2.0 + 10, np.full(8, 10.0), np.zeros(8)])                        # isolated points
    P.append(np.array([[30, 30, 0], [30.1, 30, 0.05]]))                                            # a pair: two neighbours
    P.append(r.uniform(-.3, .3, (200, 3)) + np.array([0, -8, 1]))                                  # isotropic blob
    return np.concatenate(P).astype(F)


def far_pair():
    """room plus a copy 7000 m further along x: more than 16 384 cells of 0.404 m along that axis."""
    p = room()
    q = p.copy()
    q[:, 0] = q[:, 0] + F(7000.0)
    return np.concatenate([p, q])


def oracle(cloud, r, chunk=256):
    """-> dict(count int64[n], normal float64[n, 3] (NaN rows where count < 3), gap float64[n] = (l1 - l0) / l2 (NaN there too),
    evals float64[n, 3]). Candidates are narrowed by a window along x that is wider than the radius (a superset); the decision
    itself is the float32 expression."""
    P = np.ascontiguousarray(cloud, F).reshape(-1, 3)
    n = len(P)
    r2 = F(float(r) * float(r))
    count = np.zeros(n, np.int64)
    s1 = np.zeros((n, 3))
    s2 = np.zeros((n, 6))
    fin = np.flatnonzero(np.isfinite(P).all(axis=1))
    order = fin[np.argsort(P[fin, 0], kind="stable")]
    S = P[order]
    S64 = S.astype(np.float64)
    xs = S64[:, 0]
    reach = 1.01 * float(r)
    for a in range(0, len(S), chunk):
        b = min(a + chunk, len(S))
        lo = np.searchsorted(xs, xs[a] - reach, "left")
        hi = np.searchsorted(xs, xs[b - 1] + reach, "right")
        dx = S[None, lo:hi, 0] - S[a:b, None, 0]
        dy = S[None, lo:hi, 1] - S[a:b, None, 1]
        dz = S[None, lo:hi, 2] - S[a:b, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F
        rows, cols = np.nonzero(d2 < r2)
        q = S64[lo + cols] - S64[a + rows]        # exact in float64
        m = b - a
        dst = order[a:b]
        count[dst] = np.bincount(rows, minlength=m)
        for k in range(3):
            s1[dst, k] = np.bincount(rows, weights=q[:, k], minlength=m)
        for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            s2[dst, k] = np.bincount(rows, weights=q[:, i] * q[:, j], minlength=m)
    normal = np.full((n, 3), np.nan)
    gap = np.full(n, np.nan)
    evals = np.full((n, 3), np.nan)
    ok = np.flatnonzero(count >= 3)
    if len(ok):
        k = count[ok].astype(np.float64)
        mean = s1[ok] / k[:, None]
        C = np.empty((len(ok), 3, 3))
        for t, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            C[:, i, j] = C[:, j, i] = s2[ok, t] / k - mean[:, i] * mean[:, j]
        w, v = np.linalg.eigh(C)
        normal[ok] = v[:, :, 0]
        evals[ok] = w
        with np.errstate(invalid="ignore", divide="ignore"):
            gap[ok] = (w[:, 1] - w[:, 0]) / w[:, 2]
    return dict(count=count, normal=normal, gap=gap, evals=evals)


def weights(normal, fpc_local, max_weight):
    """:142-155 in float64: fpc_local's float32 components widened; 1.0 where there is no normal."""
    f = np.asarray(fpc_local, F).astype(np.float64)
    nrm = np.asarray(normal, np.float64)
    c = np.abs((nrm[:, 0] * f[0] + nrm[:, 1] * f[1]) + nrm[:, 2] * f[2])
    has = ~np.isnan(nrm).any(axis=1)
    c = np.where(has, np.minimum(c, 1.0), 0.0)
    w = 1.0 + (float(max_weight) - 1.0) * ((np.pi / 2 - np.arccos(c)) / (np.pi / 2))
    return np.where(has, w, 1.0)


def weight_tolerance(max_weight):
    """the eigenvector moves by ~4e-12 rad with the rounding of the fp64 moments at gap >= 1e-2; the larger term
    is acos of a double dot product, which within 1.5e-8 rad of alignment returns 0 or 1.5e-8: 9.5e-9 (max_weight - 1)."""
    return 1e-7 * max(1.0, float(max_weight) - 1.0)


def direction(mean7, cov36, perform_weighting_ratio, max_weight_ratio, max_weight):
    """-> (fpc_local float64[3] (sign arbitrary), max_weight, eigen_value_ratio): numpy.linalg.eigh over |cov[:3, :3]|, the
    three-way branch of :112-127, the rotation by the inverse of the mean's quaternion in float64."""
    cov = np.abs(np.asarray(cov36, F).reshape(6, 6)[:3, :3].astype(np.float64))
    cov = np.tril(cov) + np.tril(cov, -1).T          # Eigen reads the lower triangle
    w, v = np.linalg.eigh(cov)
    ratio = np.sqrt(w[2] / w[1])
    if ratio < perform_weighting_ratio:
        mw = 1.0
    elif ratio > max_weight_ratio:
        mw = max_weight
    else:
        mw = 1.0 + (max_weight - 1.0) * ((ratio - perform_weighting_ratio) / (max_weight_ratio - perform_weighting_ratio))
    g = v[:, 2].astype(F).astype(np.float64)
    x, y, z, s = (float(t) for t in np.asarray(mean7, F)[3:7])
    nn = x * x + y * y + z * z + s * s
    R = np.array([[1 - 2 * (y * y + z * z) / nn, 2 * (x * y - s * z) / nn, 2 * (x * z + s * y) / nn],
                  [2 * (x * y + s * z) / nn, 1 - 2 * (x * x + z * z) / nn, 2 * (y * z - s * x) / nn],
                  [2 * (x * z - s * y) / nn, 2 * (y * z + s * x) / nn, 1 - 2 * (x * x + y * y) / nn]])
    return R.T @ g, mw, ratio


def upstream_statistics():
    """The upstream test's mean and covariance (:46-75, 107-109): yaw pi / 6 about z, standard deviations 1.0 front / 0.2 side."""
    yaw = np.pi / 6
    vt = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
    xv = vt.T @ np.diag([1.0 ** 2, 0.2 ** 2]) @ vt
    cov = np.zeros((6, 6), F)
    cov[:2, :2] = xv
    # Quat(Vec3(0, 0, 1), yaw): axis-angle
    mean = np.array([3.5, -5.0, 0.0, 0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)], F)
    return mean, cov


UPSTREAM_PARAMETER_SETS = [  # (perform_weighting_ratio, max_weight_ratio, max_weight) -> max_weight in use (:129-137)
    ((2.0, 4.0, 10.0), 10.0),
    ((6.0, 7.0, 10.0), 1.0),
    ((2.0, 8.0, 5.0), 3.0),
]
