// rng_index.h — the reference's uniform sampler restated so that every position of its stream can be evaluated at once
// (rng_stream.h walks it, rng_index_kernels.h holds what the device adds, tests/cpp/rng_index_emul.cpp replays it on the CPU with
// g++: no HIP type appears here).
//
// PINNED TO libstdc++, as rng_polar.h is. PointCloudUniformSampler::sample (point_cloud_uniform_sampler.h:66-71) draws
// std::uniform_int_distribution<size_t>(0, n - 1)(engine) per point, the engine being std::default_random_engine = minstd_rand0:
// min 1, max 2^31 - 2, urngrange = max - min = 2147483645. bits/uniform_int_dist.h, for a range of n values:
//
//   n <= 2147483645  ("fallback case (2 divisions)")   scaling = urngrange / n; past = n scaling;
//                                                      do ret = engine() - 1; while (ret >= past); return ret / scaling;
//   n == 2147483646                                    return engine() - 1;                       (no rejection)
//   n >= 2147483647                                    the up-scaling branch: NOT restated, refused by the callers
//
// The second case is the first with scaling = 1 and past = 2147483646 (ret <= 2147483645 < past always), so one pair
// {scaling, past} describes a range and both fit 32 bits. The stream is a sequence of ATTEMPTS, attempt t using engine output
// t + 1 behind the start state; acceptance is one integer comparison. n == 1 still consumes an engine call per draw (and
// rejects ret == 2147483645). At most n of the 2^31 - 2 outputs are rejected.
#pragma once

#include <cmath>
#include <cstdint>

#include "rng_polar.h"

namespace mcl3dl
{
namespace rng
{
constexpr uint64_t INDEX_URNG_RANGE = 2147483645ull;  // minstd_rand0::max() - min()
constexpr uint64_t INDEX_MAX_RANGE = 2147483646ull;   // the largest range that is restated
// the one-work-group kernel serves a scan whose two models draw at most this many indices together (a starting value, untimed)
constexpr uint32_t INDEX_SINGLE_MAX = 65536u;

struct IndexRange
{
  uint32_t scaling, past;
};

// range in [1, INDEX_MAX_RANGE]
RNG_HD inline IndexRange index_range(uint64_t range)
{
  IndexRange r;
  if (range > INDEX_URNG_RANGE)
  {
    r.scaling = 1u;
    r.past = static_cast<uint32_t>(INDEX_MAX_RANGE);
    return r;
  }
  const uint64_t scaling = INDEX_URNG_RANGE / range;
  r.scaling = static_cast<uint32_t>(scaling);
  r.past = static_cast<uint32_t>(range * scaling);
  return r;
}

// v: one engine output in [1, 2^31 - 2]
RNG_HD inline bool index_accepted(const IndexRange& r, uint32_t v)
{
  return v - 1u < r.past;
}

RNG_HD inline uint32_t index_value(const IndexRange& r, uint32_t v)
{
  return (v - 1u) / r.scaling;
}

// How many attempts one round of the rounds form evaluates to find k more accepted ones: rng_polar.h's attempt_budget with
// pi / 4 replaced by p = past / 2147483646 — ceil(k / p) plus three standard deviations of the accepted count expressed in
// attempts, ceil(3 sqrt(k (1 - p)) / p). p is 1 - n / 2147483646 at worst, so for real clouds the budget is k plus a handful
// and a second round is rare; for ranges near 2^30 and above (p down to 1 / 2) it is the ordinary path now and then.
inline uint64_t index_attempt_budget(uint64_t k_remaining, const IndexRange& r)
{
  const double p = static_cast<double>(r.past) / 2147483646.0;
  const double k = static_cast<double>(k_remaining);
  return static_cast<uint64_t>(std::ceil(k / p)) + static_cast<uint64_t>(std::ceil(3.0 * std::sqrt(k * (1.0 - p)) / p));
}

// rng_stream.h's attempt policy of this stream: one engine call per attempt; the output is also the engine state behind it
struct IndexPolicy
{
  IndexRange r;
  static constexpr int CALLS = 1;
  using Kept = uint32_t;
  RNG_HD bool judge(const uint32_t* v, Kept* k) const
  {
    *k = v[0];
    return index_accepted(r, v[0]);
  }
  RNG_HD static uint32_t state(const Kept& k) { return k; }
  uint64_t budget(uint64_t k_remaining) const { return index_attempt_budget(k_remaining, r); }
};
}  // namespace rng
}  // namespace mcl3dl
