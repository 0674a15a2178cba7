// rng_stream.h — the algorithm the polar, index and shuffle draws share, once (rng_stream_kernels.h runs it on the device, the
// emulators of tests/cpp on the CPU with g++: no HIP type appears here).
//
// A stream of ATTEMPTS behind one engine state, attempt t made of CALLS consecutive engine outputs, accepted or not by a rule
// that reads nothing but those outputs. Lane l walks the E = ATTEMPTS_PER_LANE attempts l E .. l E + E - 1 behind ONE jump and
// leaves an accept mask; the accepted attempts are ranked in stream order (ballots and mbcnt on the device) and handed to a
// sink at their rank. What differs between the families is an ATTEMPT POLICY, a small struct passed by value:
//
//   static constexpr int CALLS                       engine calls one attempt takes
//   struct / using Kept                              what a lane keeps per attempt
//   bool judge(const uint32_t* v, Kept* k) const     v[0 .. CALLS): the attempt's outputs; fills *k, returns the accept rule
//   static uint32_t state(const Kept& k)             the engine state behind the attempt
//   budget(...)                                      how many attempts a round evaluates (host)
//
// PolarPolicy is in rng_polar.h, IndexPolicy in rng_index.h, DoubtPolicy in rng_shuffle.h, beside the restatements they wrap.
#pragma once

#include <cstdint>

#include "rng_polar.h"  // the engine: minstd_next, minstd_jump; E = ATTEMPTS_PER_LANE, GROUP_THREADS, RNG_HD

#if defined(__HIPCC__)
#define RNG_UNROLL _Pragma("unroll")
#else
#define RNG_UNROLL
#endif

namespace mcl3dl
{
namespace rng
{
// The E attempts of `lane`, from the state CALLS E lane engine calls behind x0. Bit e of the result: attempt lane E + e is
// below n_att and accepted. kept[e] is filled for every attempt the lane walks; a lane whose first attempt is at or beyond
// n_att makes no jump and leaves kept alone.
template <typename Policy>
RNG_HD inline uint32_t lane_walk(const Policy& policy, uint32_t x0, const uint32_t* __restrict__ table, uint64_t n_att,
                                 uint64_t lane, typename Policy::Kept* kept)
{
  constexpr int E = ATTEMPTS_PER_LANE;
  const uint64_t t0 = lane * E;
  if (t0 >= n_att)
    return 0u;
  uint32_t mask = 0u;
  uint32_t x = minstd_jump(x0, static_cast<uint64_t>(Policy::CALLS) * t0, table);
  RNG_UNROLL
  for (int e = 0; e < E; ++e)
  {
    uint32_t v[Policy::CALLS];
    RNG_UNROLL
    for (int c = 0; c < Policy::CALLS; ++c)
      v[c] = x = minstd_next(x);
    const bool ok = policy.judge(v, &kept[e]) && t0 + e < n_att;
    mask |= ok ? (1u << e) : 0u;
  }
  return mask;
}

// the accepted attempts of one lane in stream order: sink(rank, e) for every set bit e, rank counting up from `rank`
template <typename Rank, typename Sink>
RNG_HD inline void place_accepted(uint32_t mask, Rank rank, Sink&& sink)
{
  RNG_UNROLL
  for (int e = 0; e < ATTEMPTS_PER_LANE; ++e)
  {
    if (!((mask >> e) & 1u))
      continue;
    sink(rank, e);
    ++rank;
  }
}
}  // namespace rng
}  // namespace mcl3dl
