// rng_index_kernels.h — the uniform sampler's index draws on the device (rng_index.h holds the restatement; host_rng.h the
// rounds): integers only, one engine output per attempt.
//
//   rng_index_single_kernel  ONE work-group, no host round: up to two segments (range, count) back to back on one stream. It
//                            walks the attempts in passes of 256 lanes x E attempts — a jump per lane, E engine steps, ballots
//                            and mbcnt ranks as rng_polar_emit_kernel —, carries the pass's start state in LDS, continues with
//                            the second segment from the attempt behind the first one's last accepted attempt, and writes the
//                            engine state behind the last accepted attempt of all
//   rng_index_count_kernel   the rounds form, as rng_polar_count_kernel: ONE count per work-group
//   (exclusive scan of the work-group counts: the cloud path's)
//   rng_index_emit_kernel    the attempts again, as rng_polar_emit_kernel: out[rank] for every rank below k_total, and the
//                            engine state behind the k_total-th accepted attempt
#pragma once
#include <hip/hip_runtime.h>

#include "rng_index.h"

namespace mcl3dl
{
namespace rng
{
// the E attempts of this lane, from the state E lane engine calls behind x0; attempts at or beyond n_att are not accepted.
// v[e]: the engine output of attempt e, which is also the engine state behind it.
__device__ inline uint32_t index_lane_mask(uint32_t x0, const uint32_t* __restrict__ table, const IndexRange& r,
                                           unsigned long long n_att, unsigned long long lane, uint32_t* v)
{
  constexpr int E = ATTEMPTS_PER_LANE;
  const unsigned long long t0 = lane * E;
  uint32_t mask = 0u;
  if (t0 >= n_att)
  {
#pragma unroll
    for (int e = 0; e < E; ++e)
      v[e] = 0u;
    return 0u;
  }
  uint32_t x = minstd_jump(x0, t0, table);
#pragma unroll
  for (int e = 0; e < E; ++e)
  {
    x = minstd_next(x);
    v[e] = x;
    mask |= (index_accepted(r, x) && t0 + e < n_att) ? (1u << e) : 0u;
  }
  return mask;
}

// accepted attempts of the lower lanes of this wavefront (all their E attempts come first), and of the whole wavefront
__device__ inline void index_wave_ranks(uint32_t mask, uint32_t* before, uint32_t* wave_total)
{
  uint32_t b4 = 0u, total = 0u;
#pragma unroll
  for (int e = 0; e < ATTEMPTS_PER_LANE; ++e)
  {
    const unsigned long long b = __ballot((mask >> e) & 1u);
    b4 += __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b), 0u));
    total += static_cast<uint32_t>(__popcll(b));
  }
  *before = b4;
  *wave_total = total;
}

struct IndexSegment
{
  IndexRange r;
  uint32_t count;  // draws of this segment; 0: nothing is drawn, the stream does not move
  uint32_t* out;   // count indices
};

__global__ __launch_bounds__(GROUP_THREADS) void rng_index_single_kernel(uint32_t x0, const uint32_t* __restrict__ table,
                                                                         IndexSegment seg0, IndexSegment seg1,
                                                                         uint32_t* __restrict__ state_out)
{
  constexpr int E = ATTEMPTS_PER_LANE;
  __shared__ uint32_t s_wave[GROUP_THREADS / 64];
  __shared__ uint32_t s_start;  // the engine state the next pass (or the next segment) starts from
  const int tid = threadIdx.x, wave = tid >> 6;
  if (tid == 0)
    s_start = x0;
  __syncthreads();
  for (int s = 0; s < 2; ++s)
  {
    const IndexSegment sg = s ? seg1 : seg0;
    uint32_t accepted = 0u;  // uniform: every lane forms it from the same LDS words
    while (accepted < sg.count)
    {
      const uint32_t start = s_start;
      uint32_t v[E];
      const uint32_t mask = index_lane_mask(start, table, sg.r, static_cast<unsigned long long>(GROUP_THREADS) * E,
                                            static_cast<unsigned long long>(tid), v);
      uint32_t before, wave_total;
      index_wave_ranks(mask, &before, &wave_total);
      if ((tid & 63) == 0)
        s_wave[wave] = wave_total;
      __syncthreads();  // (every lane has read s_start by now)
      uint32_t wave_offset = 0u, pass_total = 0u;
#pragma unroll
      for (int w = 0; w < GROUP_THREADS / 64; ++w)
      {
        wave_offset += w < wave ? s_wave[w] : 0u;
        pass_total += s_wave[w];
      }
      uint32_t rank = accepted + wave_offset + before;
#pragma unroll
      for (int e = 0; e < E; ++e)
      {
        if (!((mask >> e) & 1u))
          continue;
        if (rank < sg.count)
          sg.out[rank] = index_value(sg.r, v[e]);
        if (rank + 1u == sg.count)
          s_start = v[e];  // one lane: the segment ends behind this attempt, whatever the pass evaluated beyond it
        ++rank;
      }
      if (accepted + pass_total < sg.count && tid == GROUP_THREADS - 1)
        s_start = v[E - 1];  // the pass fell short: the next one starts 256 E engine calls on
      accepted += pass_total;
      __syncthreads();  // s_start and s_wave are free again
    }
  }
  if (tid == 0)
    *state_out = s_start;
}

__global__ __launch_bounds__(GROUP_THREADS) void rng_index_count_kernel(uint32_t x0, const uint32_t* __restrict__ table,
                                                                        IndexRange r, unsigned long long n_att,
                                                                        uint32_t* __restrict__ group_count)
{
  constexpr int E = ATTEMPTS_PER_LANE;
  __shared__ uint32_t s_wave[GROUP_THREADS / 64];
  const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * GROUP_THREADS + threadIdx.x;
  uint32_t v[E];
  const uint32_t mask = index_lane_mask(x0, table, r, n_att, lane, v);
  uint32_t before, wave_total;
  index_wave_ranks(mask, &before, &wave_total);
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

// group_offset: the exclusive scan of group_count. rank_base: accepted attempts of earlier rounds. Ranks below k_total are
// written to out[rank]. The lane holding rank k_total - 1 writes the engine state behind that attempt to *result (0 = not in
// this round: no state is 0).
__global__ __launch_bounds__(GROUP_THREADS) void rng_index_emit_kernel(uint32_t x0, const uint32_t* __restrict__ table,
                                                                       IndexRange r, unsigned long long n_att,
                                                                       const uint32_t* __restrict__ group_offset,
                                                                       unsigned long long rank_base, unsigned long long k_total,
                                                                       uint32_t* __restrict__ out, uint32_t* __restrict__ result)
{
  constexpr int E = ATTEMPTS_PER_LANE;
  __shared__ uint32_t s_wave[GROUP_THREADS / 64];
  const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * GROUP_THREADS + threadIdx.x;
  uint32_t v[E];
  const uint32_t mask = index_lane_mask(x0, table, r, n_att, lane, v);
  uint32_t before, wave_total;
  index_wave_ranks(mask, &before, &wave_total);
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
    if (rank < k_total)
      out[rank] = index_value(r, v[e]);
    if (rank + 1 == k_total)
      *result = v[e];
    ++rank;
  }
}
}  // namespace rng
}  // namespace mcl3dl
