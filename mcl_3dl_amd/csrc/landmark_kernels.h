// landmark_kernels.h — the two per-particle models of the node that read a particle's whole pose, on RESIDENT particles
// (api_group_motion.inl, api_group_state.inl):
//
//   JumpBias                    the pose-jump bias of every scan (src/mcl_3dl.cpp:436-451): probability_bias_ =
//                               nl_lin(|pos - prev.pos|) * nl_ang(ang(rot * prev.rot^-1)) + 1e-6, formed INSIDE the moments pass
//                               (pf_kernels.h: pf_moments_body) — expectationBiased / max / maxBiased without a bias array
//   landmark_likelihood_kernel  cbLandmark's measure_func (src/mcl_3dl.cpp:913-928): NormalLikelihoodNd<float, 6> over
//                               s - measured (state_6dof.h:262-274, quat.h:191-201, nd.h:72-75), one lane per particle; the
//                               existing pf::measure launches follow with these likelihoods
//
// The reference's expressions in its order and its float / double mix (-ffp-contract=off); acosf / expf / atan2f / asinf are
// evaluated in double and rounded to float ("Numerics").
#pragma once
#include <hip/hip_runtime.h>

#include "motion_kernels.h"
#include "pf_kernels.h"

#pragma clang fp contract(off)

namespace mcl3dl
{
// Quat::getAxisAng (quat.h:226-239): the angle only
__device__ inline float quat_axis_angle(Quat q)
{
  if (fabs(static_cast<double>(q.w)) >= 1.0 - 0.000001)
    return 0.0f;
  const float ac = static_cast<float>(acos(static_cast<double>(q.w)));
  float ang = static_cast<float>(static_cast<double>(ac) * 2.0);
  if (static_cast<double>(ang) > M_PI)
    ang = static_cast<float>(static_cast<double>(ang) - 2.0 * M_PI);
  return ang;
}

// bias_func of src/mcl_3dl.cpp:440-448 after the host formed NormalLikelihood(bias_var_dist / _ang)'s constants and
// state_prev_.rot_.inv()
struct JumpBias
{
  Vec3f prev_pos;
  Quat prev_rot_inv;
  float a_lin, sq2_lin, a_ang, sq2_ang;
  float* bias_out;  // [n] the biases, for the caller, or null
  __device__ float operator()(const float* ps, int i) const
  {
    const Vec3f dp = vsub(Vec3f{ ps[0], ps[1], ps[2] }, prev_pos);
    const float lin = sqrtf(vdot(dp, dp));  // Vec3::norm, vec3.h:153-156
    const float ang = quat_axis_angle(qmul(Quat{ ps[3], ps[4], ps[5], ps[6] }, prev_rot_inv));
    const float prod = normal_likelihood(a_lin, sq2_lin, lin) * normal_likelihood(a_ang, sq2_ang, ang);
    const float b = static_cast<float>(static_cast<double>(prod) + 1e-6);
    if (bias_out)
      bias_out[i] = b;
    return b;
  }
};

__global__ __launch_bounds__(PF_BLOCK) void pf_moments_jump_bias_kernel(const float* __restrict__ pose7,
                                                                        const float* __restrict__ w, JumpBias bias, int n,
                                                                        double* __restrict__ block_mom /*[grid][MOM_N]*/,
                                                                        ArgMax* __restrict__ block_arg /*[grid][2]*/)
{
  pf_moments_body(pose7, w, bias, n, block_mom, block_arg);
}

// NormalLikelihoodNd<float, 6> after its constructor ran on the host (a_, sigma_inv_: nd.h:67-71) + the measured state
struct LandmarkModel
{
  float a;
  float sinv[36];  // sigma_inv_(i, j) at [6 * i + j]
  Vec3f pos;       // measured.pos_
  Quat rot_inv;    // measured.rot_.inv()
};

__global__ __launch_bounds__(256) void landmark_likelihood_kernel(const float* __restrict__ state13, int n, LandmarkModel m,
                                                                  float* __restrict__ lik)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float* s = state13 + 13 * static_cast<size_t>(i);
  // diff = s - measured (state_6dof.h:262-274): positions subtract, rot = measured.rot.inv() * s.rot; then getRPY with the
  // double functions rounded to float
  const Vec3f d = vsub(Vec3f{ s[0], s[1], s[2] }, m.pos);
  const RpyTerms t = quat_rpy_terms(qmul(m.rot_inv, Quat{ s[3], s[4], s[5], s[6] }));
  const float x[6] = { d.x,
                       d.y,
                       d.z,
                       static_cast<float>(atan2(static_cast<double>(t.t3), static_cast<double>(t.t4))),
                       static_cast<float>(asin(static_cast<double>(t.t2))),
                       static_cast<float>(atan2(static_cast<double>(t.t1), static_cast<double>(t.t0))) };
  // -0.5 * x^T * sigma_inv * x (nd.h:74): y = -0.5f x (exact), r = y^T sigma_inv, e = r x — float, sequential over 0..5
  float e = 0.0f;
#pragma unroll
  for (int j = 0; j < 6; ++j)
  {
    float r = (-0.5f * x[0]) * m.sinv[j];
#pragma unroll
    for (int k = 1; k < 6; ++k)
      r = r + (-0.5f * x[k]) * m.sinv[6 * k + j];
    e = j == 0 ? r * x[0] : e + r * x[j];
  }
  lik[i] = m.a * static_cast<float>(exp(static_cast<double>(e)));
}
}  // namespace mcl3dl
