"""Writes tests/golden/landmark.npz: what the reference's own headers compute for the pose-jump bias of a scan and for the
landmark update on seeded inputs — the fixture of tests/test_landmark_cpu.py. Run by hand, like make_motion_golden.py, where the
reference's headers are (REFERENCE, default ../reference next to the repository, or MCL3DL_REFERENCE):

    python tests/golden/make_landmark_golden.py [REFERENCE]

A small C++ driver (below) is compiled with g++ -ffp-contract=off against the reference's state_6dof.h, quat.h, vec3.h, nd.h and
pf.h (with oracle/shims for ROS). nd.h's NormalLikelihoodNd needs Eigen::Matrix, which is not on this box: the script writes a
minimal stand-in into its temporary shim directory as <Eigen/LU> — determinant() / inverse() by LU with partial pivoting in double
rounded to float, products summed sequentially. That pins a_'s formula and the exponent's structure to the text of nd.h; Eigen's own
rounding is not pinned by anything here ("What is not reproduced"). build() never runs this."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import landmark_ref as lr  # noqa: E402
import motion_ref as mr  # noqa: E402

EIGEN_LU = r'''
#include <Eigen/Core>
#include <cmath>
namespace Eigen {
template <typename T, int R, int C> class Matrix {
public:
  T v_[R][C];
  Matrix() { for (int r = 0; r < R; ++r) for (int c = 0; c < C; ++c) v_[r][c] = 0; }
  T& operator()(int r, int c) { return v_[r][c]; }
  T operator()(int r, int c) const { return v_[r][c]; }
  Matrix<T, C, R> transpose() const { Matrix<T, C, R> t; for (int r = 0; r < R; ++r) for (int c = 0; c < C; ++c) t(c, r) = v_[r][c]; return t; }
  template <int K> Matrix<T, R, K> operator*(const Matrix<T, C, K>& o) const {
    Matrix<T, R, K> m;
    for (int r = 0; r < R; ++r) for (int k = 0; k < K; ++k) {
      T s = v_[r][0] * o(0, k);
      for (int j = 1; j < C; ++j) s = s + v_[r][j] * o(j, k);
      m(r, k) = s; }
    return m; }
  operator T() const { static_assert(R == 1 && C == 1, "only a 1 x 1 matrix converts to its scalar"); return v_[0][0]; }
  // LU with partial pivoting in double: packed factors in a, row order in perm, returns the sign or 0 when singular
  int factor(double a[R][C], int perm[R]) const {
    static_assert(R == C, "square");
    int sign = 1;
    for (int r = 0; r < R; ++r) { perm[r] = r; for (int c = 0; c < C; ++c) a[r][c] = v_[r][c]; }
    for (int k = 0; k < R; ++k) {
      int p = k;
      for (int i = k + 1; i < R; ++i) if (std::fabs(a[i][k]) > std::fabs(a[p][k])) p = i;
      if (a[p][k] == 0.0) return 0;
      if (p != k) { for (int j = 0; j < C; ++j) { const double t = a[k][j]; a[k][j] = a[p][j]; a[p][j] = t; }
                    const int t = perm[k]; perm[k] = perm[p]; perm[p] = t; sign = -sign; }
      for (int i = k + 1; i < R; ++i) { a[i][k] = a[i][k] / a[k][k]; for (int j = k + 1; j < C; ++j) a[i][j] = a[i][j] - a[i][k] * a[k][j]; } }
    return sign; }
  T determinant() const { double a[R][C]; int perm[R]; double d = factor(a, perm); for (int k = 0; k < R; ++k) d = d * a[k][k]; return static_cast<T>(d); }
  Matrix inverse() const {
    double a[R][C]; int perm[R]; Matrix inv; factor(a, perm);
    for (int c = 0; c < C; ++c) {
      double y[R], x[R];
      for (int i = 0; i < R; ++i) { double s = perm[i] == c ? 1.0 : 0.0; for (int j = 0; j < i; ++j) s = s - a[i][j] * y[j]; y[i] = s; }
      for (int i = R - 1; i >= 0; --i) { double s = y[i]; for (int j = i + 1; j < R; ++j) s = s - a[i][j] * x[j]; x[i] = s / a[i][i]; }
      for (int r = 0; r < R; ++r) inv(r, c) = static_cast<T>(x[r]); }
    return inv; }
};
// a double literal times a float matrix: Eigen converts the literal to the matrix's scalar
template <typename T, int R, int C> Matrix<T, R, C> operator*(double s, const Matrix<T, R, C>& m) {
  Matrix<T, R, C> o; const T f = static_cast<T>(s);
  for (int r = 0; r < R; ++r) for (int c = 0; c < C; ++c) o(r, c) = f * m(r, c);
  return o; }
}
'''

DRIVER = r'''
#include <cstdio>
#include <cstdint>
#include <vector>
#include <mcl_3dl/pf.h>
#include <mcl_3dl/state_6dof.h>
#include <mcl_3dl/nd.h>
using namespace mcl_3dl;
typedef pf::ParticleFilter<State6DOF, float, ParticleWeightedMeanQuat, std::default_random_engine> PF;
static FILE* in; static FILE* out;
static int rd_i() { int32_t v; if (fread(&v, 4, 1, in) != 1) throw 1; return v; }
static std::vector<float> rd_f(size_t n) { std::vector<float> v(n); if (n && fread(v.data(), 4, n, in) != n) throw 1; return v; }
static std::vector<double> rd_d(size_t n) { std::vector<double> v(n); if (n && fread(v.data(), 8, n, in) != n) throw 1; return v; }
static void wr(const float* p, size_t n) { fwrite(p, 4, n, out); }
static State6DOF st(const float* s) { return State6DOF(Vec3(s[0], s[1], s[2]), Quat(s[3], s[4], s[5], s[6])); }
struct Nd : public NormalLikelihoodNd<float, 6> {
  explicit Nd(const Matrix& m) : NormalLikelihoodNd<float, 6>(m) {}
  float a() const { return a_; }
  float inv(int r, int c) const { return sigma_inv_(r, c); }
};
int main(int argc, char** argv) {
  in = fopen(argv[1], "rb"); out = fopen(argv[2], "wb");
  // 1. the pose-jump bias (src/mcl_3dl.cpp:436-451): lin_diff, ang_diff, p_bias per particle
  { const int np = rd_i(); const std::vector<float> prev = rd_f(7), var = rd_f(2), s = rd_f(13 * np);
    const State6DOF state_prev = st(prev.data());
    NormalLikelihood<float> nl_lin(var[0]); NormalLikelihood<float> nl_ang(var[1]);
    for (int i = 0; i < np; ++i) {
      const State6DOF x = st(&s[13 * i]);
      const float lin_diff = (x.pos_ - state_prev.pos_).norm();
      Vec3 axis; float ang_diff;
      (x.rot_ * state_prev.rot_.inv()).getAxisAng(axis, ang_diff);
      const float p_bias = nl_lin(lin_diff) * nl_ang(ang_diff) + 1e-6;
      const float v[3] = { lin_diff, ang_diff, p_bias }; wr(v, 3); } }
  // 2. landmark cases (cbLandmark, src/mcl_3dl.cpp:899-929): s - measured, getRPY, NormalLikelihoodNd, pf::measure
  { const int nc = rd_i();
    for (int c = 0; c < nc; ++c) {
      const int np = rd_i(); const std::vector<float> m7 = rd_f(7); const std::vector<double> cov = rd_d(36);
      const std::vector<float> s = rd_f(13 * np), w = rd_f(np);
      Nd::Matrix sigma;  // Eigen::Matrix<double, 6, 6>(data).cast<float>(): column-major
      for (int r = 0; r < 6; ++r) for (int cc = 0; cc < 6; ++cc) sigma(r, cc) = static_cast<float>(cov[6 * cc + r]);
      Nd nd(sigma);
      const State6DOF measured = st(m7.data());
      float head[37]; head[0] = nd.a();
      for (int r = 0; r < 6; ++r) for (int cc = 0; cc < 6; ++cc) head[1 + 6 * r + cc] = nd.inv(r, cc);
      wr(head, 37);
      const auto measure_func = [&](const State6DOF& x) -> float {
        State6DOF diff = x - measured;
        const Vec3 rpy = diff.rot_.getRPY();
        Nd::Vector v;
        v(0, 0) = diff.pos_.x_; v(1, 0) = diff.pos_.y_; v(2, 0) = diff.pos_.z_; v(3, 0) = rpy.x_; v(4, 0) = rpy.y_; v(5, 0) = rpy.z_;
        return nd(v); };
      PF pf(np, 1);
      int i = 0; for (auto it = pf.begin(); it != pf.end(); ++it, ++i) { it->state_ = st(&s[13 * i]); it->probability_ = w[i]; }
      std::vector<float> lik(np); float sum = 0;
      i = 0; for (auto it = pf.begin(); it != pf.end(); ++it, ++i) {
        const State6DOF diff = it->state_ - measured; const Vec3 rpy = diff.rot_.getRPY();
        const float v[10] = { diff.pos_.x_, diff.pos_.y_, diff.pos_.z_, diff.rot_.x_, diff.rot_.y_, diff.rot_.z_, diff.rot_.w_,
                              rpy.x_, rpy.y_, rpy.z_ };
        wr(v, 10);
        lik[i] = measure_func(it->state_); sum += it->probability_ * lik[i]; }
      pf.measure(measure_func);
      std::vector<float> wo; for (auto it = pf.begin(); it != pf.end(); ++it) wo.push_back(it->probability_);
      const float tail[2] = { sum > 0.0 ? pf.getEntropy() : 0.0f, sum > 0.0 ? 0.0f : 1.0f };
      wr(lik.data(), np); wr(wo.data(), np); wr(tail, 2);
    } }
  fclose(out);
  return 0;
}
'''


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def unit_quats(rng, n, spread):
    q = rng.normal(0.0, spread, (n, 4))
    q[:, 3] += 1.0
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return f32(q)


def rpy_quat(r, p, y):
    """Quat::setRPY (quat.h:202-215) in double."""
    t2, t3, t4, t5, t0, t1 = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.array([t0 * t3 * t4 - t1 * t2 * t5, t0 * t2 * t5 + t1 * t3 * t4, t1 * t2 * t4 - t0 * t3 * t5,
                     t0 * t2 * t4 + t1 * t3 * t5])


def bias_inputs(rng):
    """60 particles about state_prev_: ordinary ones, rotation == prev.rot and == -prev.rot (ang = 0 on both signs of w), and
    negated rotations 2 .. 3 rad away (w < 0 of the product: the - 2 pi fold)."""
    n = 60
    prev = np.concatenate([[1.0, -2.0, 0.3], rpy_quat(0.02, -0.03, 0.8)])
    prev = f32(prev)
    s = np.zeros((n, 13), np.float32)
    s[:, :3] = prev[:3] + rng.normal(0, 1.0, (n, 3))
    s[:, 3:7] = mr.qmul(unit_quats(rng, n, 0.3), np.broadcast_to(prev[3:7], (n, 4)))
    s[0, 3:7] = prev[3:7]
    s[1, 3:7] = -prev[3:7]
    s[2, :3] = prev[:3]  # no jump at all
    s[2, 3:7] = prev[3:7]
    for i in range(3, 13):  # rotations by 2 .. 3 rad about random axes, stored negated
        ax = rng.normal(0, 1, 3)
        ax /= np.linalg.norm(ax)
        a = rng.uniform(2.0, 3.0)
        d = f32(np.concatenate([ax * np.sin(a / 2), [np.cos(a / 2)]]))
        s[i, 3:7] = -mr.qmul(d[None], prev[None, 3:7])[0]
    return prev, f32([2.0, 1.57]), s  # the node's defaults for bias_var_dist / bias_var_ang


def landmark_inputs(rng):
    cases = []
    # 0. an ordinary update: a full (non-diagonal, slightly NON-symmetric: the column-major convention shows) covariance, particles
    #    within about four sigma, pitch within 1e-3 of +-pi/2 among them with rotations a few ulp longer than 1 (the clamp of t2)
    n = 80
    m7 = f32(np.concatenate([[0.5, -1.0, 0.2], rpy_quat(0.05, -0.02, 0.4)]))
    B = rng.normal(0, 1, (6, 6))
    cov = np.diag([0.3, 0.25, 0.2, 0.8, 1.2, 0.9]) + 0.02 * (B @ B.T)
    cov[0, 1] += 0.003  # sigma(1, 0) != sigma(0, 1)
    s = np.zeros((n, 13), np.float32)
    s[:, :3] = m7[:3] + rng.normal(0, 0.4, (n, 3))
    s[:, 3:7] = mr.qmul(np.broadcast_to(m7[3:7], (n, 4)), unit_quats(rng, n, 0.25))
    s[:, 7:] = rng.normal(0, 0.05, (n, 6))  # the odometry-error fields take no part
    for i in range(24):
        sign = 1.0 if i % 2 == 0 else -1.0
        pitch = sign * (np.pi / 2 - (i // 2) * 8e-5)
        d = rpy_quat(rng.uniform(-0.3, 0.3), pitch, rng.uniform(-0.3, 0.3)) * (1.0 + 2e-7 * (1 + i // 2))
        s[i, 3:7] = mr.qmul(m7[None, 3:7], f32(d)[None])[0]
    w = f32(rng.uniform(0.5, 1.5, n))
    cases.append((m7, cov.T.reshape(36).copy(), s, f32(w / w.sum())))  # cov36[6 c + r] = sigma(r, c)
    # 1. every likelihood underflows: a landmark five metres away with a millimetre covariance (restore)
    n = 20
    s = np.zeros((n, 13), np.float32)
    s[:, :3] = rng.normal(0, 0.1, (n, 3))
    s[:, 3:7] = unit_quats(rng, n, 0.05)
    cases.append((f32([5.0, 0, 0, 0, 0, 0, 1]), (np.eye(6) * 1e-6).reshape(36), s, f32(np.full(n, 1.0 / n))))
    # 2. the determinant leaves float range: a_ = 0, every likelihood 0 (restore)
    cases.append((f32([0, 0, 0, 0, 0, 0, 1]), (np.eye(6) * 1e7).reshape(36), s, f32(np.full(n, 1.0 / n))))
    return cases


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MCL3DL_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
    rng = np.random.default_rng(2025)
    prev, var, bs = bias_inputs(rng)
    cases = landmark_inputs(rng)
    with tempfile.TemporaryDirectory() as td:
        src, exe, fin, fout = (os.path.join(td, n) for n in ("driver.cpp", "driver", "in.bin", "out.bin"))
        with open(src, "w") as f:
            f.write(DRIVER)
        os.makedirs(os.path.join(td, "shim", "Eigen"))
        with open(os.path.join(td, "shim", "Eigen", "LU"), "w") as f:
            f.write(EIGEN_LU)
        subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-Wno-deprecated-declarations",
                        "-I" + os.path.join(ROOT, "oracle", "shims"), "-I" + os.path.join(td, "shim"),
                        "-I" + os.path.join(ref, "include"), "-o", exe, src], check=True)
        with open(fin, "wb") as f:
            f.write(struct.pack("<i", len(bs)))
            f.write(prev.tobytes() + var.tobytes() + bs.tobytes())
            f.write(struct.pack("<i", len(cases)))
            for m7, cov, s, w in cases:
                f.write(struct.pack("<i", len(s)))
                f.write(m7.tobytes() + np.ascontiguousarray(cov, np.float64).tobytes() + s.tobytes() + w.tobytes())
        subprocess.run([exe, fin, fout], check=True)
        o = np.fromfile(fout, np.float32)
    pos = 0

    def take(n):
        nonlocal pos
        v = o[pos:pos + n]
        pos += n
        return v
    out = dict(bias_prev=prev, bias_var=var, bias_state=bs)
    out["bias_out"] = take(3 * len(bs)).reshape(-1, 3)  # lin_diff, ang_diff, p_bias
    for c, (m7, cov, s, w) in enumerate(cases):
        n = len(s)
        out["lm%d_measured" % c], out["lm%d_cov" % c], out["lm%d_state" % c], out["lm%d_w" % c] = m7, cov, s, w
        head = take(37)
        out["lm%d_a" % c], out["lm%d_sinv" % c] = head[:1], head[1:].reshape(6, 6)
        out["lm%d_diff" % c] = take(10 * n).reshape(n, 10)  # diff.pos 3, diff.rot 4, rpy 3
        out["lm%d_lik" % c] = take(n)
        out["lm%d_wout" % c] = take(n)
        out["lm%d_tail" % c] = take(2)
    out["lm_cases"] = np.array([len(cases)], np.int32)
    assert pos == len(o), (pos, len(o))
    # every branch the fixture is there for was taken
    ang = out["bias_out"][:, 1]
    _, _, ang_r, folded = lr.jump_bias(bs, prev, var[0], var[1], host=True, parts=True)
    q = mr.qmul(bs[:, 3:7], np.broadcast_to(mr.qinv(prev[3:7]), (len(bs), 4)))
    assert ang[0] == 0.0 and q[0, 3] > 0 and ang[1] == 0.0 and q[1, 3] < 0, "ang = 0 on both signs of w"
    assert folded[3:13].all() and np.all(q[3:13, 3] < 0) and np.all(ang[3:13] < -2.0), "the - 2 pi fold"
    assert np.any(ang[13:] > 0.1)
    t2d = lr.rpy_terms(out["lm0_diff"][:, 3:7])[5]
    pitch = out["lm0_diff"][:, 8]
    assert np.any(t2d > 1.0) and np.any(t2d < -1.0), "the clamp of t2 on both sides"
    assert np.all(pitch[t2d > 1.0] == np.float32(np.pi / 2)) and np.all(pitch[t2d < -1.0] == -np.float32(np.pi / 2))
    assert np.all(np.abs(np.abs(pitch[:24]) - np.pi / 2) < 1e-3)
    assert out["lm0_tail"][1] == 0.0 and np.all(out["lm0_lik"] > 1e-30), "the ordinary case stays in normal floats"
    assert out["lm1_tail"][1] == 1.0 and np.all(out["lm1_lik"] == 0.0) and out["lm1_a"][0] > 0, "the underflow case restores"
    assert out["lm2_tail"][1] == 1.0 and out["lm2_a"][0] == 0.0 and np.all(out["lm2_lik"] == 0.0), "det = inf restores"
    path = os.path.join(HERE, "landmark.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {kk: v.shape for kk, v in out.items()})


if __name__ == "__main__":
    main()
