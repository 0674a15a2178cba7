// rng_stream_kernels.h — rng_stream.h's attempt stream on the device (256 threads, wave64; host_rng.h holds the rounds):
//
//   stream_count_kernel<Policy>        one lane per run of E consecutive attempts (one jump, then CALLS E engine steps); accept
//                                      flags by ballot, ONE count per work-group
//   (exclusive scan of the work-group counts: scan_tiles / scan_add_offsets of map_compiler.h, the cloud path's)
//   stream_emit_kernel<Policy, Sink>   the attempts again; rank of an accepted attempt = earlier rounds + work-group offset +
//                                      wavefront offset + mbcnt of the ballots; every rank below k_total goes to the sink, and
//                                      the engine state behind the k_total-th accepted attempt to the result word
//
// A SINK is a small struct passed by value with operator()(rank, t, kept): t is the attempt's number in the round. PolarSink is
// in rng_kernels.h, IndexSink in rng_index_kernels.h, DoubtSink in rng_shuffle_kernels.h. No work-group waits on another: the
// unknown length of the stream is handled by rounds on the host.
#pragma once
#include <hip/hip_runtime.h>

#include "rng_stream.h"

#pragma clang fp contract(off)

namespace mcl3dl
{
namespace rng
{
// accepted attempts of the lower lanes of this wavefront (all their E attempts come first), and of the whole wavefront
__device__ inline void wave_ranks(uint32_t mask, uint32_t* before, uint32_t* wave_total)
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

// s_wave: GROUP_THREADS / 64 words of LDS. Accepted attempts of the lower wavefronts of this work-group, and of all of it.
// Holds a barrier; s_wave is read by every lane behind it (a caller that reuses s_wave puts a barrier of its own in between).
__device__ inline void group_ranks(uint32_t wave_total, uint32_t* s_wave, uint32_t* wave_offset, uint32_t* group_total)
{
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    s_wave[wave] = wave_total;
  __syncthreads();
  uint32_t offset = 0u, total = 0u;
#pragma unroll
  for (int w = 0; w < GROUP_THREADS / 64; ++w)
  {
    offset += w < wave ? s_wave[w] : 0u;
    total += s_wave[w];
  }
  *wave_offset = offset;
  *group_total = total;
}

template <typename Policy>
__global__ __launch_bounds__(GROUP_THREADS) void stream_count_kernel(uint32_t x0, const uint32_t* __restrict__ table,
                                                                     Policy policy, unsigned long long n_att,
                                                                     uint32_t* __restrict__ group_count)
{
  __shared__ uint32_t s_wave[GROUP_THREADS / 64];
  const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * GROUP_THREADS + threadIdx.x;
  typename Policy::Kept kept[ATTEMPTS_PER_LANE];
  const uint32_t mask = lane_walk(policy, x0, table, n_att, lane, kept);
  uint32_t before, wave_total, wave_offset, group_total;
  wave_ranks(mask, &before, &wave_total);
  group_ranks(wave_total, s_wave, &wave_offset, &group_total);
  if (threadIdx.x == 0)
    group_count[blockIdx.x] = group_total;
}

// group_offset: the exclusive scan of group_count. rank_base: accepted attempts of earlier rounds. sink(rank, t, kept) for every
// accepted attempt of rank below k_total. The lane holding rank k_total - 1 writes the engine state behind that attempt to
// *result (0 = not in this round: no state is 0).
template <typename Policy, typename Sink>
__global__ __launch_bounds__(GROUP_THREADS) void stream_emit_kernel(uint32_t x0, const uint32_t* __restrict__ table,
                                                                    Policy policy, unsigned long long n_att,
                                                                    const uint32_t* __restrict__ group_offset,
                                                                    unsigned long long rank_base, unsigned long long k_total,
                                                                    Sink sink, uint32_t* __restrict__ result)
{
  __shared__ uint32_t s_wave[GROUP_THREADS / 64];
  const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * GROUP_THREADS + threadIdx.x;
  typename Policy::Kept kept[ATTEMPTS_PER_LANE];
  const uint32_t mask = lane_walk(policy, x0, table, n_att, lane, kept);
  uint32_t before, wave_total, wave_offset, group_total;
  wave_ranks(mask, &before, &wave_total);
  group_ranks(wave_total, s_wave, &wave_offset, &group_total);
  place_accepted(mask, rank_base + group_offset[blockIdx.x] + wave_offset + before,
                 [&](unsigned long long rank, int e)
                 {
                   if (rank < k_total)
                     sink(rank, lane * ATTEMPTS_PER_LANE + e, kept[e]);
                   if (rank + 1 == k_total)
                     *result = Policy::state(kept[e]);
                 });
}
}  // namespace rng
}  // namespace mcl3dl
