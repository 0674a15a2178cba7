// motion_kernels.h — what the node does to every RESIDENT particle between two scans (api_group_motion.inl):
//
//   predict_kernel          MotionPredictionModelDifferentialDrive::predict (motion_prediction_model_differential_drive.h:56-67)
//   reset_odom_integ_kernel the node's integ_reset_func (src/mcl_3dl.cpp:190-195)
//   add_noise_kernel        pf::addNoiseUsingNoiseGenerator (pf.h:226-237): State6DOF::operator+ with caller-drawn noise
//   odom_factor_kernel      NormalLikelihood(odom_err_integ_lin_sigma)(|odom_err_integ_lin_|) of the scan update (:420-423)
//   ImuGravity              ImuMeasurementModelGravity::measure (imu_measurement_model_gravity.h:50-56), evaluated inside
//                           pf::measure's partial-sum pass (pf_kernels.h: pf_partial_kernel / pf_fused_kernel)
//
// Every expression is the reference's, in its order and its float / double mix (-ffp-contract=off). The transcendentals are the
// exception: the reference calls glibc's float sinf / cosf / acosf / expf, which are not correctly rounded; here they are
// evaluated in double and rounded to float (within 1 ulp of any faithful libm: DESIGN.md, "Numerics").
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"

#pragma clang fp contract(off)

namespace mcl3dl
{
// (beside device_math.h's quaternion helpers: that file is one of the sources the likelihood / beam counter profiles are pinned to)
// Quat::normalize, quat.h:179-182
__host__ __device__ inline void qnormalize(Quat& q) { q = qnormalized(q); }

// Quat::inv, quat.h:187-190: conj() / dot(*this), the reciprocal formed in double and narrowed to float (operator/)
__host__ __device__ inline Quat qinv(Quat q)
{
  const float d = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
  const float s = static_cast<float>(1.0 / static_cast<double>(d));
  return { -q.x * s, -q.y * s, -q.z * s, q.w * s };
}

// State6DOF::operator+ (state_6dof.h:249-260) of state s and noise a: components 0-2 and 7-12 add, rot = a.rot * s.rot; the
// result is a fresh State6DOF (its odometry noise is 0). Writes o[0..2] and o[7..12], returns the rotation (the caller stores
// it, normalised or not). s and o may be the same array.
__host__ __device__ inline Quat state6dof_plus(const float* s, const float* a, float* o)
{
  const Quat r = qmul(Quat{ a[3], a[4], a[5], a[6] }, Quat{ s[3], s[4], s[5], s[6] });
#pragma unroll
  for (int k = 0; k < 3; ++k)
    o[k] = s[k] + a[k];
#pragma unroll
  for (int k = 7; k < 13; ++k)
    o[k] = s[k] + a[k];
  return r;
}

// NormalLikelihood<float>::operator() (nd.h:50-53): a_ * expf(-x * x / sq2_); a_ and sq2_ come from the host (nd.h:46-48)
__device__ inline float normal_likelihood(float a, float sq2, float x)
{
  const float e = -x * x / sq2;
  return a * static_cast<float>(exp(static_cast<double>(e)));
}

// Quat(Vec3(0, 0, 1), ang): setAxisAng (quat.h:216-225): axis / axis.norm() is (0, 0, 1) exactly, then normalize()
__device__ inline Quat quat_axis_z(float ang)
{
  const float h = ang / 2;
  const float s = static_cast<float>(sin(static_cast<double>(h)));
  const Quat q = { 0.0f * s, 0.0f * s, 1.0f * s, static_cast<float>(cos(static_cast<double>(h))) };
  return qnormalized(q);
}

// MotionPredictionModelDifferentialDrive::setOdoms (:46-54) as the host computes it once per call, + the two decay factors
// (1.0 - time_diff_ / tc): float quotient, double difference, narrowed to float by Vec3::operator*=(float)
struct MotionStep
{
  Vec3f t;          // relative_translation_
  Quat rq;          // relative_quat_
  float t_norm;     // relative_translation_norm_
  float ang;        // relative_angle_
  float decay_lin;  // odom_err_integ_lin_ *= ...
  float decay_ang;  // odom_err_integ_ang_ *= ...
};

// One thread per particle; state13 in place, noise4 = {noise_ll_, noise_la_, noise_al_, noise_aa_} per particle or null (all 0),
// pose7 = the 7-float pose mirror the update and the moments read (written here: it never goes stale).
__global__ void predict_kernel(float* state13, const float* __restrict__ noise4, int n, MotionStep m, float* __restrict__ pose7)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  float* s = state13 + 13 * static_cast<size_t>(i);
  float nll = 0.0f, nla = 0.0f, nal = 0.0f, naa = 0.0f;
  if (noise4)
  {
    const float* z = noise4 + 4 * static_cast<size_t>(i);
    nll = z[0];
    nla = z[1];
    nal = z[2];
    naa = z[3];
  }
  // diff = relative_translation_ * (1.0 + noise_ll_) + Vec3(noise_al_ * relative_angle_, 0, 0)
  const float f = static_cast<float>(1.0 + static_cast<double>(nll));
  const Vec3f diff = vadd(vscale(m.t, f), Vec3f{ nal * m.ang, 0.0f, 0.0f });
  Vec3f lin = vadd(Vec3f{ s[7], s[8], s[9] }, vsub(diff, m.t));
  const Quat rot = { s[3], s[4], s[5], s[6] };
  const Vec3f pos = vadd(Vec3f{ s[0], s[1], s[2] }, qrot(rot, diff));  // the rotation from before this step
  const float yaw = nla * m.t_norm + naa * m.ang;
  Quat r = qmul(qmul(quat_axis_z(yaw), rot), m.rq);  // rot_ = Quat(...) * rot_ * relative_quat_; rot_.normalize()
  qnormalize(r);
  Vec3f ang = vadd(Vec3f{ s[10], s[11], s[12] }, Vec3f{ 0.0f, 0.0f, yaw });
  lin = vscale(lin, m.decay_lin);
  ang = vscale(ang, m.decay_ang);
  const float out[13] = { pos.x, pos.y, pos.z, r.x, r.y, r.z, r.w, lin.x, lin.y, lin.z, ang.x, ang.y, ang.z };
#pragma unroll
  for (int k = 0; k < 13; ++k)
    s[k] = out[k];
  float* p = pose7 + 7 * static_cast<size_t>(i);
#pragma unroll
  for (int k = 0; k < 7; ++k)
    p[k] = out[k];
}

__global__ void reset_odom_integ_kernel(float* __restrict__ state13, int n)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  float* s = state13 + 13 * static_cast<size_t>(i);
#pragma unroll
  for (int k = 7; k < 13; ++k)
    s[k] = 0.0f;
}

// state = state + noise13[i] (no normalize(): pf::noise does not call it), pose mirror written alongside
__global__ void add_noise_kernel(float* state13, const float* __restrict__ noise13, int n, float* __restrict__ pose7)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  float* s = state13 + 13 * static_cast<size_t>(i);
  const Quat r = state6dof_plus(s, noise13 + 13 * static_cast<size_t>(i), s);
  s[3] = r.x;
  s[4] = r.y;
  s[5] = r.z;
  s[6] = r.w;
  float* p = pose7 + 7 * static_cast<size_t>(i);
#pragma unroll
  for (int k = 0; k < 7; ++k)
    p[k] = s[k];
}

// the scan update's odometry factor per resident particle, into the `extra` array pf::measure multiplies in
__global__ void odom_factor_kernel(const float* __restrict__ state13, int n, float a, float sq2, float* __restrict__ extra)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float* s = state13 + 13 * static_cast<size_t>(i);
  const Vec3f lin = { s[7], s[8], s[9] };
  extra[i] = normal_likelihood(a, sq2, sqrtf(vdot(lin, lin)));  // Vec3::norm, vec3.h:153-156
}

// ImuMeasurementModelGravity after setAccMeasure (acc, |acc| from the host) with NormalLikelihood(acc_var)'s constants.
// state13 == null: not an IMU update (the pf kernels read their `lik` array instead).
struct ImuGravity
{
  const float* state13;
  float* lik_out;  // [n] the likelihoods, for the caller
  Vec3f acc;
  float acc_norm, a, sq2;
};
__device__ inline float imu_gravity_likelihood(const ImuGravity& m, int i)
{
  const float* s = m.state13 + 13 * static_cast<size_t>(i);
  const Vec3f e = qrot(qinv(Quat{ s[3], s[4], s[5], s[6] }), Vec3f{ 0.0f, 0.0f, 1.0f });
  const float c = vdot(e, m.acc) / (m.acc_norm * sqrtf(vdot(e, e)));
  const float diff = static_cast<float>(acos(static_cast<double>(c)));  // NaN beyond [-1, 1], as acosf
  const float l = normal_likelihood(m.a, m.sq2, diff);
  m.lik_out[i] = l;
  return l;
}

// resample_apply's companion for the odometry noise (pf.h:211-222): a copied slot keeps its source's noise (the it == end copy
// included), a duplicated one holds a fresh State6DOF's zeros
__global__ void resample_noise_kernel(const float* __restrict__ noise_in, const uint32_t* __restrict__ source,
                                      const uint32_t* __restrict__ noise_slot, int n_out, float* __restrict__ noise_out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out)
    return;
  const bool dup = noise_slot[i] != 0xffffffffu;
  const float* z = noise_in + 4 * static_cast<size_t>(source[i]);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    noise_out[4 * static_cast<size_t>(i) + k] = dup ? 0.0f : z[k];
}
}  // namespace mcl3dl
