// rng_kernels.h — the reference's noise draws on the device (rng_polar.h holds the restatement and the attempt policy;
// rng_stream_kernels.h the count and emit kernels, instantiated with PolarPolicy and the sink below; host_rng.h the rounds):
//
//   PolarSink<PAIRS>         what stream_emit_kernel writes for an accepted polar attempt: the values whose rank lies in the
//                            caller's window
//   rng_noise_state_kernel   one lane per particle: DiagonalNoiseGenerator::operator() (value sigma + mean, zero sigmas skipped)
//                            and State6DOF::generateNoise into the 13-float rows add_noise_kernel / resample_apply_kernel read
//   rng_multivariate_state_kernel  one lane per particle: MultivariateNoiseGenerator::operator() (mean + T values, six values of one
//                            shared distribution) and generateNoise into the same rows
//   rng_odom_noise_kernel    update_noise_func's four values per particle, scaled, in set_odom_noise's storage order
#pragma once
#include <hip/hip_runtime.h>

#include "rng_stream_kernels.h"

#pragma clang fp contract(off)

namespace mcl3dl
{
namespace rng
{
// Ranks in [k_begin, k_end) are written to values[rank - k_begin] (PAIRS: values[2 (rank - k_begin)] = y mult, + 1 = x mult).
template <bool PAIRS>
struct PolarSink
{
  unsigned long long k_begin, k_end;
  float* __restrict__ values;
  __device__ void operator()(unsigned long long rank, unsigned long long, const PolarPolicy::Kept& k) const
  {
    if (rank < k_begin || rank >= k_end)
      return;
    const float mult = polar_mult(k.r2, LogDouble());
    if (PAIRS)
    {
      values[2 * (rank - k_begin)] = k.y * mult;
      values[2 * (rank - k_begin) + 1] = k.x * mult;
    }
    else
      values[rank - k_begin] = k.y * mult;
  }
};

struct NoiseGen6
{
  float mean[6], sigma[6];
  int dims;  // number of non-zero sigmas: values per particle
};

// one lane per noise row: row i takes values[dims i ...] (the window starts at the first row's first value)
__global__ void rng_noise_state_kernel(const float* __restrict__ values, NoiseGen6 gen, int n, float* __restrict__ out13)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float* z = values + static_cast<size_t>(gen.dims) * i;
  float v[6], row[13];
  int d = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k)
  {
    if (gen.sigma[k] == 0.0f)
      v[k] = gen.mean[k];  // diagonal_noise_generator.h:69-73: nothing drawn
    else
      v[k] = z[d++] * gen.sigma[k] + gen.mean[k];  // normal_distribution: ret * stddev + mean
  }
  noise6_to_state13(v, gen.mean, row);
  float* o = out13 + 13 * static_cast<size_t>(i);
#pragma unroll
  for (int k = 0; k < 13; ++k)
    o[k] = row[k];
}

// MultivariateNoiseGenerator (multivariate_noise_generator.h) for State6DOF: the mean's six values and norm_transform_, row-major
struct NoiseGenFull6
{
  float mean[6], t[36];
  int reset_odom_integ;  // 1: integ_reset_func behind the draw (src/mcl_3dl.cpp:190-195), columns 7-12 are 0
};

// one lane per particle: operator() (:80-91) and State6DOF::generateNoise behind ONE normal_distribution<float>(0, 1) called six
// times, so row i takes values[6 i ...] of the pairs stream (the window starts at the first row's first value; 24 bytes per lane,
// 8-byte aligned). sample_noise = mean_vec_ + norm_transform_ * random, in float without fused multiply-add, term by term:
//   s_i   = ((((T[i][0] r0 + T[i][1] r1) + T[i][2] r2) + T[i][3] r3) + T[i][4] r4) + T[i][5] r5
//   org_i = mean[i] + s_i
// Eigen's own association of the six-term product is not pinned by the reference (it depends on Eigen's version and vector width:
// DESIGN.md 3.10.1 says the same of the cloud transforms); this left-to-right sum is the definition here.
__global__ void rng_multivariate_state_kernel(const float* __restrict__ values, NoiseGenFull6 gen, int n, float* __restrict__ out13)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float2* z = reinterpret_cast<const float2*>(values) + 3 * static_cast<size_t>(i);
  const float2 z01 = z[0], z23 = z[1], z45 = z[2];
  const float raw[6] = { z01.x, z01.y, z23.x, z23.y, z45.x, z45.y };
  float r[6], org[6], row[13];
#pragma unroll
  for (int k = 0; k < 6; ++k)
    r[k] = raw[k] * 1.0f + 0.0f;  // normal_distribution(0, 1): ret * stddev + mean
#pragma unroll
  for (int k = 0; k < 6; ++k)
  {
    const float* t = gen.t + 6 * k;
    const float s = ((((t[0] * r[0] + t[1] * r[1]) + t[2] * r[2]) + t[3] * r[3]) + t[4] * r[4]) + t[5] * r[5];
    org[k] = gen.mean[k] + s;
  }
  noise6_to_state13(org, gen.mean, row);
  if (gen.reset_odom_integ)
  {
#pragma unroll
    for (int k = 7; k < 13; ++k)
      row[k] = 0.0f;
  }
  float* o = out13 + 13 * static_cast<size_t>(i);
#pragma unroll
  for (int k = 0; k < 13; ++k)
    o[k] = row[k];
}

// values: four per particle in draw order ll, la, aa, al of normal_distribution<float>(0, 1) (ret * 1 + 0); err4 = {lin_lin,
// lin_ang, ang_ang, ang_lin}; noise4 = {ll, la, al, aa}, set_odom_noise's storage order
__global__ void rng_odom_noise_kernel(const float* __restrict__ values, float e_ll, float e_la, float e_aa, float e_al, int n,
                                      float* __restrict__ noise4)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float* z = values + 4 * static_cast<size_t>(i);
  float* o = noise4 + 4 * static_cast<size_t>(i);
  o[0] = (z[0] * 1.0f + 0.0f) * e_ll;
  o[1] = (z[1] * 1.0f + 0.0f) * e_la;
  o[3] = (z[2] * 1.0f + 0.0f) * e_aa;
  o[2] = (z[3] * 1.0f + 0.0f) * e_al;
}
}  // namespace rng
}  // namespace mcl3dl
