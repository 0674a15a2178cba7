// rng_index_kernels.h — the uniform sampler's index draws on the device (rng_index.h holds the restatement and the attempt
// policy; host_rng.h the rounds): integers only, one engine output per attempt.
//
//   rng_index_single_kernel  ONE work-group, no host round: up to two segments (range, count) back to back on one stream. It
//                            walks the attempts in passes of 256 lanes x E attempts with rng_stream.h's lane walk and placement
//                            loop and rng_stream_kernels.h's ranks, carries the pass's start state in LDS, continues with the
//                            second segment from the attempt behind the first one's last accepted attempt, and writes the
//                            engine state behind the last accepted attempt of all
//   IndexSink                the rounds form is rng_stream_kernels.h's count and emit kernels with IndexPolicy and this sink:
//                            out[rank] for every rank below k_total
#pragma once
#include <hip/hip_runtime.h>

#include "rng_index.h"
#include "rng_stream_kernels.h"

namespace mcl3dl
{
namespace rng
{
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
    const IndexPolicy policy{ sg.r };
    uint32_t accepted = 0u;  // uniform: every lane forms it from the same LDS words
    while (accepted < sg.count)
    {
      const uint32_t start = s_start;
      uint32_t v[E];
      const uint32_t mask = lane_walk(policy, start, table, static_cast<unsigned long long>(GROUP_THREADS) * E,
                                      static_cast<unsigned long long>(tid), v);
      uint32_t before, wave_total;
      wave_ranks(mask, &before, &wave_total);
      // group_ranks' step, written out: behind the call the compiler moves `accepted` to scalar registers through
      // v_readfirstlane and the pass loop is 5 % slower
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
      place_accepted(mask, accepted + wave_offset + before,
                     [&](uint32_t rank, int e)
                     {
                       if (rank < sg.count)
                         sg.out[rank] = index_value(sg.r, v[e]);
                       if (rank + 1u == sg.count)
                         s_start = v[e];  // one lane: the segment ends behind this attempt, whatever the pass evaluated beyond it
                     });
      if (accepted + pass_total < sg.count && tid == GROUP_THREADS - 1)
        s_start = v[E - 1];  // the pass fell short: the next one starts 256 E engine calls on
      accepted += pass_total;
      __syncthreads();  // s_start and s_wave are free again
    }
  }
  if (tid == 0)
    *state_out = s_start;
}

struct IndexSink
{
  IndexRange r;
  uint32_t* __restrict__ out;
  __device__ void operator()(unsigned long long rank, unsigned long long, uint32_t v) const { out[rank] = index_value(r, v); }
};
}  // namespace rng
}  // namespace mcl3dl
