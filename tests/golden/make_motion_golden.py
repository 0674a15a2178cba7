"""Writes tests/golden/motion.npz: what the reference's own between-scan models compute on seeded inputs — the fixture of
tests/test_motion_cpu.py and tests/test_gpu_resident_motion.py. Run by hand, like make_golden.py, where the reference's headers
are (REFERENCE, default ../reference next to the repository, or MCL3DL_REFERENCE):

    python tests/golden/make_motion_golden.py [REFERENCE]

A small C++ driver (below) is compiled with g++ -ffp-contract=off against the reference's state_6dof.h, pf.h,
motion_prediction_model_differential_drive.h, imu_measurement_model_gravity.h and nd.h (with oracle/shims for ROS / Eigen,
as oracle/Makefile builds the reference) and fed the inputs through a file. build() never runs this."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

DRIVER = r'''
#include <cstdio>
#include <cstdint>
#include <vector>
#include <mcl_3dl/pf.h>
#include <mcl_3dl/state_6dof.h>
#include <mcl_3dl/nd.h>
#include <mcl_3dl/motion_prediction_models/motion_prediction_model_differential_drive.h>
#include <mcl_3dl/imu_measurement_models/imu_measurement_model_gravity.h>
using namespace mcl_3dl;
typedef pf::ParticleFilter<State6DOF, float, ParticleWeightedMeanQuat, std::default_random_engine> PF;
static FILE* in; static FILE* out;
static int rd_i() { int32_t v; if (fread(&v, 4, 1, in) != 1) throw 1; return v; }
static std::vector<float> rd_f(size_t n) { std::vector<float> v(n); if (n && fread(v.data(), 4, n, in) != n) throw 1; return v; }
static void wr(const float* p, size_t n) { fwrite(p, 4, n, out); }
static State6DOF st(const float* s, const float* nz) {
  State6DOF r(Vec3(s[0], s[1], s[2]), Quat(s[3], s[4], s[5], s[6]));
  r.odom_err_integ_lin_ = Vec3(s[7], s[8], s[9]); r.odom_err_integ_ang_ = Vec3(s[10], s[11], s[12]);
  if (nz) { r.noise_ll_ = nz[0]; r.noise_la_ = nz[1]; r.noise_al_ = nz[2]; r.noise_aa_ = nz[3]; }
  return r;
}
static void put(const State6DOF& s) {
  const float v[17] = { s.pos_.x_, s.pos_.y_, s.pos_.z_, s.rot_.x_, s.rot_.y_, s.rot_.z_, s.rot_.w_,
                        s.odom_err_integ_lin_.x_, s.odom_err_integ_lin_.y_, s.odom_err_integ_lin_.z_,
                        s.odom_err_integ_ang_.x_, s.odom_err_integ_ang_.y_, s.odom_err_integ_ang_.z_,
                        s.noise_ll_, s.noise_la_, s.noise_al_, s.noise_aa_ };
  wr(v, 17);
}
int main(int argc, char** argv) {
  in = fopen(argv[1], "rb"); out = fopen(argv[2], "wb");
  // 1. chained predictions (cbOdom, src/mcl_3dl.cpp:227-232) through pf::predict
  { const int np = rd_i(), k = rd_i(); const std::vector<float> tc = rd_f(2), s = rd_f(13 * np), nz = rd_f(4 * np);
    const std::vector<float> steps = rd_f(15 * k);
    PF pf(np, 1);
    int i = 0; for (auto it = pf.begin(); it != pf.end(); ++it, ++i) it->state_ = st(&s[13 * i], &nz[4 * i]);
    MotionPredictionModelDifferentialDrive model(tc[0], tc[1]);
    for (int j = 0; j < k; ++j) {
      const float* o = &steps[15 * j];
      model.setOdoms(State6DOF(Vec3(o[0], o[1], o[2]), Quat(o[3], o[4], o[5], o[6])),
                     State6DOF(Vec3(o[7], o[8], o[9]), Quat(o[10], o[11], o[12], o[13])), o[14]);
      pf.predict([&](State6DOF& x) { model.predict(x); });
      for (auto it = pf.begin(); it != pf.end(); ++it) put(it->state_);
    } }
  // 2. State6DOF::operator+ (pf.h:226-237 adds it to every particle)
  { const int m = rd_i(); const std::vector<float> s = rd_f(13 * m), nz4 = rd_f(4 * m), a = rd_f(13 * m);
    PF pf(m, 1);
    int i = 0; for (auto it = pf.begin(); it != pf.end(); ++it, ++i) it->state_ = st(&s[13 * i], &nz4[4 * i]);
    i = 0; pf.predict([&](State6DOF& x) { x = x + st(&a[13 * i], nullptr); ++i; });
    for (auto it = pf.begin(); it != pf.end(); ++it) put(it->state_); }
  // 3. IMU: pf::measure with ImuMeasurementModelGravity (cbImu, src/mcl_3dl.cpp:997-1002)
  { const int nc = rd_i();
    for (int c = 0; c < nc; ++c) {
      const int np = rd_i(); const std::vector<float> acc = rd_f(4), s = rd_f(13 * np), w = rd_f(np);
      ImuMeasurementModelGravity model(acc[3]);
      model.setAccMeasure(Vec3(acc[0], acc[1], acc[2]));
      PF pf(np, 1);
      int i = 0; for (auto it = pf.begin(); it != pf.end(); ++it, ++i) { it->state_ = st(&s[13 * i], nullptr); it->probability_ = w[i]; }
      std::vector<float> lik(np); float sum = 0;
      i = 0; for (auto it = pf.begin(); it != pf.end(); ++it, ++i) { lik[i] = model.measure(it->state_); sum += it->probability_ * lik[i]; }
      pf.measure([&](const State6DOF& x) { return model.measure(x); });
      std::vector<float> wo; for (auto it = pf.begin(); it != pf.end(); ++it) wo.push_back(it->probability_);
      const float tail[2] = { sum > 0.0 ? pf.getEntropy() : 0.0f, sum > 0.0 ? 0.0f : 1.0f };
      wr(lik.data(), np); wr(wo.data(), np); wr(tail, 2);
    } }
  // 4. the scan update's odometry factor (src/mcl_3dl.cpp:420-423)
  { const int m = rd_i(); const std::vector<float> sg = rd_f(1), lin = rd_f(3 * m);
    NormalLikelihood<float> nd(sg[0]);
    for (int i = 0; i < m; ++i) { const float v = nd(Vec3(lin[3 * i], lin[3 * i + 1], lin[3 * i + 2]).norm()); wr(&v, 1); } }
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


def random_states(rng, n, spread=0.3):
    s = np.zeros((n, 13), np.float32)
    s[:, :3] = rng.uniform(-5, 5, (n, 3))
    s[:, 3:7] = unit_quats(rng, n, spread)
    s[:, 7:] = rng.normal(0.0, 0.05, (n, 6))
    return s


def yaw_quat(yaw):
    return np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)], np.float32)


def make_inputs(seed=2024):
    rng = np.random.default_rng(seed)
    g = {}
    # 1. predict: 37 particles, a 6-step odometry path (a straight step without rotation included: getAxisAng's ang = 0 branch)
    np_p, k = 37, 6
    g["pred_tc"] = f32([10.0, 10.0])
    g["pred_state"] = random_states(rng, np_p)
    g["pred_noise"] = f32(rng.normal(0.0, 1.0, (np_p, 4)) * np.array([0.1, 0.05, 0.05, 0.1]))
    odo, yaw, steps = np.zeros(3), 0.3, []
    for j in range(k):
        dyaw = 0.0 if j == 2 else rng.uniform(-0.2, 0.2)
        prev = np.concatenate([odo, yaw_quat(yaw)])
        odo = odo + np.array([np.cos(yaw), np.sin(yaw), 0.01]) * rng.uniform(0.05, 0.3)
        yaw += dyaw
        cur = np.concatenate([odo, yaw_quat(yaw)])
        steps.append(np.concatenate([prev, cur, [rng.uniform(0.06, 0.2)]]))
    g["pred_steps"] = f32(steps)
    # 2. operator+
    m = 40
    g["plus_state"] = random_states(rng, m)
    g["plus_state_noise4"] = f32(rng.normal(0, 0.1, (m, 4)))  # dropped by operator+: a fresh State6DOF
    a = np.zeros((m, 13), np.float32)
    a[:, :3] = rng.normal(0, 0.5, (m, 3))
    a[:, 3:7] = unit_quats(rng, m, 0.05)
    a[:, 7:] = rng.normal(0, 0.02, (m, 6))
    g["plus_noise"] = a
    # 3. IMU: an ordinary case, one where every likelihood underflows (restore), and one with a NaN (acosf of a ratio > 1)
    cases = []
    s = random_states(rng, 50, 0.1)
    w = f32(rng.uniform(0.5, 1.5, 50))
    w /= w.sum()
    cases.append((f32([0.1, -0.2, 9.8, 0.3]), s, f32(w)))
    s = random_states(rng, 20, 0.1)
    s[:, 3:7] = f32([[0.7071068, 0.0, 0.0, 0.7071068]] * 20)  # rolled by 90 degrees: the angle to gravity is ~pi/2
    cases.append((f32([0.0, 0.0, 9.8, 1e-3]), s, f32(np.full(20, 0.05))))
    s = random_states(rng, 30, 0.1)
    nan_acc = find_nan_acc(rng, s[0, 3:7])
    cases.append((f32(list(nan_acc) + [0.3]), s, f32(np.full(30, 1.0 / 30))))
    g["imu_cases"] = cases
    # 4. odometry factor
    g["odom_sigma"] = f32([0.1])
    g["odom_lin"] = f32(rng.normal(0, 0.08, (60, 3)))
    g["odom_lin"][0] = 0.0
    return g


def find_nan_acc(rng, q):
    """An acceleration for which the gravity model's float ratio dot / (|acc| |acc_estim|) exceeds 1 at rotation q (acosf ->
    NaN): acc parallel to the estimate, its length chosen until rounding pushes the ratio above 1."""
    sys.path.insert(0, os.path.dirname(HERE))
    import motion_ref as mr
    e = mr.qrot(mr.qinv(q[None]), np.array([[0, 0, 1]], np.float32))[0]
    for _ in range(100000):
        acc = (e * np.float32(rng.uniform(5.0, 15.0))).astype(np.float32)
        c = mr.vdot(e, acc) / (mr.vnorm(acc) * mr.vnorm(e))
        if c > np.float32(1.0):
            return acc
    raise RuntimeError("no acceleration with a ratio above 1 found")


def write_inputs(path, g):
    with open(path, "wb") as f:
        def i(v):
            f.write(struct.pack("<i", v))

        def a(x):
            f.write(f32(x).tobytes())
        i(len(g["pred_state"])); i(len(g["pred_steps"]))
        a(g["pred_tc"]); a(g["pred_state"]); a(g["pred_noise"]); a(g["pred_steps"])
        i(len(g["plus_state"]))
        a(g["plus_state"]); a(g["plus_state_noise4"]); a(g["plus_noise"])
        i(len(g["imu_cases"]))
        for acc, s, w in g["imu_cases"]:
            i(len(s)); a(acc); a(s); a(w)
        i(len(g["odom_lin"]))
        a(g["odom_sigma"]); a(g["odom_lin"])


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MCL3DL_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
    g = make_inputs()
    with tempfile.TemporaryDirectory() as td:
        src, exe, fin, fout = (os.path.join(td, n) for n in ("driver.cpp", "driver", "in.bin", "out.bin"))
        with open(src, "w") as f:
            f.write(DRIVER)
        # nd.h includes <Eigen/LU> for NormalLikelihoodNd, which the driver never instantiates: a declaration is enough
        os.makedirs(os.path.join(td, "shim", "Eigen"))
        with open(os.path.join(td, "shim", "Eigen", "LU"), "w") as f:
            f.write("#include <Eigen/Core>\nnamespace Eigen { template <typename T, int R, int C> class Matrix { }; }\n")
        subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-Wno-deprecated-declarations",
                        "-I" + os.path.join(ROOT, "oracle", "shims"), "-I" + os.path.join(td, "shim"),
                        "-I" + os.path.join(ref, "include"), "-o", exe, src], check=True)
        write_inputs(fin, g)
        subprocess.run([exe, fin, fout], check=True)
        o = np.fromfile(fout, np.float32)
    pos = 0

    def take(n):
        nonlocal pos
        v = o[pos:pos + n]
        pos += n
        return v
    np_p, k = len(g["pred_state"]), len(g["pred_steps"])
    out = dict(pred_tc=g["pred_tc"], pred_state=g["pred_state"], pred_noise=g["pred_noise"], pred_steps=g["pred_steps"])
    out["pred_out"] = take(k * np_p * 17).reshape(k, np_p, 17)
    m = len(g["plus_state"])
    out.update(plus_state=g["plus_state"], plus_state_noise4=g["plus_state_noise4"], plus_noise=g["plus_noise"])
    out["plus_out"] = take(m * 17).reshape(m, 17)
    for c, (acc, s, w) in enumerate(g["imu_cases"]):
        n = len(s)
        out["imu%d_acc" % c], out["imu%d_state" % c], out["imu%d_w" % c] = acc, s, w
        out["imu%d_lik" % c] = take(n)
        out["imu%d_wout" % c] = take(n)
        out["imu%d_tail" % c] = take(2)
    out["imu_cases"] = np.array([len(g["imu_cases"])], np.int32)
    out.update(odom_sigma=g["odom_sigma"], odom_lin=g["odom_lin"])
    out["odom_factor"] = take(len(g["odom_lin"]))
    assert pos == len(o), (pos, len(o))
    assert np.isnan(out["imu2_lik"][0]), "the NaN case did not produce a NaN likelihood"
    assert out["imu1_tail"][1] == 1.0, "the underflow case did not restore"
    path = os.path.join(HERE, "motion.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {kk: v.shape for kk, v in out.items()})


if __name__ == "__main__":
    main()
