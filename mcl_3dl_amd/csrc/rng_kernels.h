// rng_kernels.h — the reference's noise draws on the device (rng_polar.h holds the restatement; api_rng.inl the host rounds):
//
//   rng_polar_count_kernel   one lane per run of E consecutive attempts (one jump, then 2E engine steps); accept flags by
//                            ballot, ONE count per work-group
//   (exclusive scan of the work-group counts: scan_tiles / scan_add_offsets of map_compiler.h, the cloud path's)
//   rng_polar_emit_kernel    the attempts again; rank of an accepted attempt = work-group offset + wavefront offset + mbcnt of
//                            the ballots; writes the values whose rank lies in the caller's window, and the engine state behind
//                            the K-th accepted attempt
//   rng_noise_state_kernel   one lane per particle: DiagonalNoiseGenerator::operator() (value sigma + mean, zero sigmas skipped)
//                            and State6DOF::generateNoise into the 13-float rows add_noise_kernel / resample_apply_kernel read
//   rng_odom_noise_kernel    update_noise_func's four values per particle, scaled, in set_odom_noise's storage order
//
// No work-group waits on another: the unknown length of the stream is handled by rounds on the host.
#pragma once
#include <hip/hip_runtime.h>

#include "rng_polar.h"

#pragma clang fp contract(off)

namespace mcl3dl
{
namespace rng
{
// the E attempts of this lane, from the state 2 E lane engine calls behind x0; attempts at or beyond n_att are not accepted
struct LaneAttempts
{
  float x[ATTEMPTS_PER_LANE], y[ATTEMPTS_PER_LANE], r2[ATTEMPTS_PER_LANE];
  uint32_t state[ATTEMPTS_PER_LANE];  // the engine state behind each attempt's second draw
  uint32_t accepted;                  // bit e: attempt e
};

__device__ inline uint32_t lane_accept_mask(uint32_t x0, const uint32_t* __restrict__ table, unsigned long long n_att,
                                            unsigned long long lane, LaneAttempts* keep)
{
  constexpr int E = ATTEMPTS_PER_LANE;
  const unsigned long long t0 = lane * E;
  uint32_t mask = 0u;
  if (t0 >= n_att)
    return 0u;
  uint32_t x = minstd_jump(x0, 2ull * t0, table);
#pragma unroll
  for (int e = 0; e < E; ++e)
  {
    const uint32_t v1 = minstd_next(x);
    x = minstd_next(v1);
    const Attempt a = polar_attempt(v1, x);
    const bool ok = a.accepted && t0 + e < n_att;
    mask |= ok ? (1u << e) : 0u;
    if (keep)
    {
      keep->x[e] = a.x;
      keep->y[e] = a.y;
      keep->r2[e] = a.r2;
      keep->state[e] = x;
    }
  }
  return mask;
}

__global__ __launch_bounds__(GROUP_THREADS) void rng_polar_count_kernel(uint32_t x0, const uint32_t* __restrict__ table,
                                                                        unsigned long long n_att,
                                                                        uint32_t* __restrict__ group_count)
{
  constexpr int E = ATTEMPTS_PER_LANE;
  __shared__ uint32_t s_wave[GROUP_THREADS / 64];
  const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * GROUP_THREADS + threadIdx.x;
  const uint32_t mask = lane_accept_mask(x0, table, n_att, lane, nullptr);
  uint32_t wave_total = 0u;
#pragma unroll
  for (int e = 0; e < E; ++e)
    wave_total += static_cast<uint32_t>(__popcll(__ballot((mask >> e) & 1u)));
  if ((threadIdx.x & 63) == 0)
    s_wave[threadIdx.x >> 6] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    uint32_t s = 0u;
#pragma unroll
    for (int w = 0; w < GROUP_THREADS / 64; ++w)
      s += s_wave[w];
    group_count[blockIdx.x] = s;
  }
}

// group_offset: the exclusive scan of group_count. rank_base: accepted attempts of earlier rounds. Ranks in [k_begin, k_end)
// (and below k_total) are written to values[rank - k_begin] (PAIRS: values[2 (rank - k_begin)] = y mult, + 1 = x mult). The
// lane holding rank k_total - 1 writes the engine state behind that attempt to *result (0 = not in this round: no state is 0).
template <bool PAIRS>
__global__ __launch_bounds__(GROUP_THREADS) void rng_polar_emit_kernel(uint32_t x0, const uint32_t* __restrict__ table,
                                                                       unsigned long long n_att,
                                                                       const uint32_t* __restrict__ group_offset,
                                                                       unsigned long long rank_base, unsigned long long k_total,
                                                                       unsigned long long k_begin, unsigned long long k_end,
                                                                       float* __restrict__ values, uint32_t* __restrict__ result)
{
  constexpr int E = ATTEMPTS_PER_LANE;
  __shared__ uint32_t s_wave[GROUP_THREADS / 64];
  const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * GROUP_THREADS + threadIdx.x;
  LaneAttempts at;
  const uint32_t mask = lane_accept_mask(x0, table, n_att, lane, &at);
  // accepted attempts of the lower lanes of this wavefront (all their E attempts come first), and of the whole wavefront
  uint32_t before = 0u, wave_total = 0u;
#pragma unroll
  for (int e = 0; e < E; ++e)
  {
    const unsigned long long b = __ballot((mask >> e) & 1u);
    before += __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b), 0u));
    wave_total += static_cast<uint32_t>(__popcll(b));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    s_wave[wave] = wave_total;
  __syncthreads();
  uint32_t wave_offset = 0u;
#pragma unroll
  for (int w = 0; w < GROUP_THREADS / 64; ++w)
    wave_offset += w < wave ? s_wave[w] : 0u;
  unsigned long long rank = rank_base + group_offset[blockIdx.x] + wave_offset + before;
#pragma unroll
  for (int e = 0; e < E; ++e)
  {
    if (!((mask >> e) & 1u))
      continue;
    if (rank < k_total && rank >= k_begin && rank < k_end)
    {
      const float mult = polar_mult(at.r2[e], LogDouble());
      if (PAIRS)
      {
        values[2 * (rank - k_begin)] = at.y[e] * mult;
        values[2 * (rank - k_begin) + 1] = at.x[e] * mult;
      }
      else
        values[rank - k_begin] = at.y[e] * mult;
    }
    if (rank + 1 == k_total)
      *result = at.state[e];
    ++rank;
  }
}

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
