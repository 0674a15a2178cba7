// rng_shuffle_kernels.h — the single path of std::shuffle(iota(n), engine_) on the device (rng_shuffle.h holds the restatement
// and says why the pair path, n <= 46340, stays on the host; host_shuffle.h the rounds). Integers only; wave64; no scratch.
//
//   DoubtPolicy, DoubtSink       rng_stream_kernels.h's count and emit kernels with these: the attempts in runs of E per lane
//                                behind one jump, ONE count of doubtful attempts per work-group, the exclusive scan (the cloud
//                                path's), then {attempt number, engine output} of every doubtful attempt, in stream order
//   shuffle_resolve_kernel       ONE wavefront walks the doubtful list in order, 64 entries speculated at a time: every lane judges
//                                its entry as if no entry of the batch in front of it were rejected, the lowest lane that reports a
//                                rejection (or the end of the shuffle) is right, the batch restarts behind it. Leaves the sorted
//                                rejected attempt numbers, their count and whether the evaluated attempts complete the shuffle
//   shuffle_targets_kernel       the attempts a third time: step = 1 + t - (rejections before t), target[step] = j_step
//   (stable radix sort of (j_i, i - 1) by j_i: sort_kernels.h)
//   shuffle_chain_kernel         one lane per p < m walks f(p, n) over the sorted pairs
#pragma once
#include <hip/hip_runtime.h>

#include "rng_shuffle.h"
#include "rng_stream_kernels.h"

namespace mcl3dl
{
namespace rng
{
// {attempt number, engine output} of a doubtful attempt at its rank; the two lists have room for the count pass's total
struct DoubtSink
{
  uint32_t* __restrict__ doubt_t;
  uint32_t* __restrict__ doubt_v;
  __device__ void operator()(unsigned long long rank, unsigned long long t, uint32_t v) const
  {
    doubt_t[rank] = static_cast<uint32_t>(t);  // (the host refuses a stream of 2^32 attempts or more)
    doubt_v[rank] = v;
  }
};

// result[0] = rejections among the steps of the shuffle, result[1] = 1 when the n_att attempts hold all n - 1 steps.
// rejected_t has room for n_doubt entries.
__global__ __launch_bounds__(64) void shuffle_resolve_kernel(const uint32_t* __restrict__ doubt_t,
                                                             const uint32_t* __restrict__ doubt_v, uint32_t n_doubt,
                                                             unsigned long long n, unsigned long long n_att,
                                                             uint32_t* __restrict__ rejected_t, uint32_t* __restrict__ result)
{
  const uint32_t lane = threadIdx.x;
  uint32_t d0 = 0u, rejected = 0u;  // uniform: formed from ballots
  while (d0 < n_doubt)
  {
    const uint32_t d = d0 + lane;
    const bool have = d < n_doubt;
    const uint32_t t = have ? doubt_t[d] : 0u;
    const uint32_t v = have ? doubt_v[d] : 1u;
    const int verdict = have ? shuffle_resolve(t, v, rejected, n) : SHUFFLE_ACCEPTED;
    const unsigned long long events = __ballot(verdict != SHUFFLE_ACCEPTED);
    if (events == 0ull)
    {
      d0 += 64u;
      continue;
    }
    const uint32_t first = static_cast<uint32_t>(__ffsll(events)) - 1u;
    const unsigned long long beyond = __ballot(verdict == SHUFFLE_BEYOND);
    if ((beyond >> first) & 1ull)
      break;  // every attempt from here on lies behind the shuffle
    if (lane == first)
      rejected_t[rejected] = t;
    ++rejected;
    d0 += first + 1u;
  }
  if (lane == 0u)
  {
    result[0] = rejected;
    result[1] = n_att - rejected >= n - 1ull ? 1u : 0u;
  }
}

// n_used = (n - 1) + n_rejected attempts make the shuffle; target[i] = j_i for i in [1, n - 1] (target[0] is not written)
__global__ __launch_bounds__(GROUP_THREADS) void shuffle_targets_kernel(uint32_t x0, const uint32_t* __restrict__ table,
                                                                        unsigned long long n, unsigned long long n_used,
                                                                        const uint32_t* __restrict__ rejected_t,
                                                                        uint32_t n_rejected, uint32_t* __restrict__ target)
{
  constexpr int E = ATTEMPTS_PER_LANE;
  const unsigned long long lane = static_cast<unsigned long long>(blockIdx.x) * GROUP_THREADS + threadIdx.x;
  const unsigned long long t0 = lane * E;
  if (t0 >= n_used)
    return;
  // rejections before t0
  uint32_t rb = 0u, len = n_rejected;
  while (len > 0u)
  {
    const uint32_t half = len >> 1;
    if (rejected_t[rb + half] < t0)
    {
      rb += half + 1u;
      len -= half + 1u;
    }
    else
      len = half;
  }
  uint32_t next_rejected = rb < n_rejected ? rejected_t[rb] : 0xffffffffu;
  uint32_t x = minstd_jump(x0, t0, table);
#pragma unroll
  for (int e = 0; e < E; ++e)
  {
    x = minstd_next(x);
    const unsigned long long t = t0 + e;
    if (t >= n_used)
      break;
    if (t == next_rejected)
    {
      ++rb;
      next_rejected = rb < n_rejected ? rejected_t[rb] : 0xffffffffu;
      continue;
    }
    const unsigned long long step = 1ull + t - rb;
    if (step < n)
      target[step] = shuffle_target(static_cast<uint32_t>(step), x);
  }
}

// keys / steps: the n - 1 pairs (j_i, i - 1) in stable order of j_i; out[p] = a[p] of the shuffled iota for p < m
__global__ __launch_bounds__(256) void shuffle_chain_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ steps,
                                                            const uint32_t* __restrict__ target, uint32_t n, uint32_t m,
                                                            uint32_t* __restrict__ out)
{
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= m)
    return;
  out[p] = shuffle_entry(keys, steps, n, target, p, nullptr);
}
}  // namespace rng
}  // namespace mcl3dl
