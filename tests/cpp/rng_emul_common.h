// rng_emul_common.h — what the rng_*_emul.cpp programs share: the door to the standard library's engine state, and the CPU
// stand-in for the device around rng_stream.h. The lane walk, the accept rules and the placement loop are NOT restated here:
// they are the headers the kernels compile (mcl_3dl_amd/csrc/rng_stream.h and the policies of rng_polar.h / rng_index.h /
// rng_shuffle.h). What is replayed is what only the device has: 64-lane ballots and mbcnt, 256-thread work-groups, one count
// per work-group, the exclusive scan, ranks from earlier rounds + group offset + wavefront offset + mbcnt.
#pragma once
#include <cstdint>
#include <random>
#include <sstream>
#include <vector>

#include "../../mcl_3dl_amd/csrc/rng_stream.h"

namespace
{
using namespace mcl3dl::rng;

uint32_t g_table[64];  // minstd_build_table, by main
constexpr int E = ATTEMPTS_PER_LANE;
constexpr int WAVES = GROUP_THREADS / 64;
constexpr uint64_t PER_GROUP = static_cast<uint64_t>(GROUP_THREADS) * E;

inline void set_state(std::default_random_engine& e, uint32_t s)
{
  std::stringstream ss;
  ss << s;
  ss >> e;
}
inline uint32_t get_state(const std::default_random_engine& e)
{
  std::stringstream ss;
  ss << e;
  unsigned long v = 0;
  ss >> v;
  return static_cast<uint32_t>(v);
}

inline uint32_t modpow(uint32_t a, uint64_t k)
{
  uint32_t r = 1;
  for (; k; k >>= 1, a = minstd_mulmod(a, a))
    if (k & 1)
      r = minstd_mulmod(r, a);
  return r;
}

template <typename Policy>
struct Lane
{
  typename Policy::Kept kept[E];
  uint32_t mask;
};

// one work-group's lanes behind wave_ranks: `before` per thread, the total per wavefront
template <typename Policy>
void group_lanes(const Policy& policy, uint32_t x0, uint64_t n_att, uint64_t first_lane, Lane<Policy>* lanes, uint32_t* before,
                 uint32_t* wave_total)
{
  for (int w = 0; w < WAVES; ++w)
  {
    uint64_t ballot[E] = { 0 };
    wave_total[w] = 0;
    for (int l = 0; l < 64; ++l)
    {
      Lane<Policy>& L = lanes[w * 64 + l];
      L = Lane<Policy>{};
      L.mask = lane_walk(policy, x0, g_table, n_att, first_lane + w * 64 + l, L.kept);
      before[w * 64 + l] = 0;
      for (int e = 0; e < E; ++e)
        ballot[e] |= static_cast<uint64_t>((L.mask >> e) & 1u) << l;
    }
    for (int e = 0; e < E; ++e)
    {
      wave_total[w] += static_cast<uint32_t>(__builtin_popcountll(ballot[e]));
      for (int l = 0; l < 64; ++l)  // mbcnt: set bits below lane l
        before[w * 64 + l] += static_cast<uint32_t>(__builtin_popcountll(ballot[e] & ((1ull << l) - 1ull)));
    }
  }
}

// group_ranks for thread t
inline uint32_t wave_offset_of(const uint32_t* wave_total, int t)
{
  uint32_t offset = 0;
  for (int w = 0; w < (t >> 6); ++w)
    offset += wave_total[w];
  return offset;
}

// stream_count_kernel work-group by work-group, then the exclusive scan (n_groups + 1 entries: the last one becomes the total)
template <typename Policy>
std::vector<uint32_t> count_and_scan(const Policy& policy, uint32_t x0, uint64_t n_att)
{
  const uint64_t n_groups = (n_att + PER_GROUP - 1) / PER_GROUP;
  std::vector<uint32_t> counts(n_groups + 1, 0u);
  std::vector<Lane<Policy>> lanes(GROUP_THREADS);
  uint32_t before[GROUP_THREADS], wave_total[WAVES];
  for (uint64_t g = 0; g < n_groups; ++g)
  {
    group_lanes(policy, x0, n_att, g * GROUP_THREADS, lanes.data(), before, wave_total);
    for (int w = 0; w < WAVES; ++w)
      counts[g] += wave_total[w];
  }
  uint32_t run = 0;
  for (uint64_t g = 0; g <= n_groups; ++g)
  {
    const uint32_t c = counts[g];
    counts[g] = run;
    run += c;
  }
  return counts;
}

// stream_emit_kernel work-group by work-group: sink(rank, t, kept) below k_total; returns the result word
template <typename Policy, typename Sink>
uint32_t emit_groups(const Policy& policy, uint32_t x0, uint64_t n_att, const std::vector<uint32_t>& counts, uint64_t rank_base,
                     uint64_t k_total, Sink&& sink)
{
  std::vector<Lane<Policy>> lanes(GROUP_THREADS);
  uint32_t before[GROUP_THREADS], wave_total[WAVES];
  uint32_t result = 0;
  for (uint64_t g = 0; g + 1 < counts.size(); ++g)
  {
    group_lanes(policy, x0, n_att, g * GROUP_THREADS, lanes.data(), before, wave_total);
    for (int t = 0; t < GROUP_THREADS; ++t)
    {
      const Lane<Policy>& L = lanes[t];
      place_accepted(L.mask, rank_base + counts[g] + wave_offset_of(wave_total, t) + before[t],
                     [&](uint64_t rank, int e)
                     {
                       if (rank < k_total)
                         sink(rank, (g * GROUP_THREADS + t) * E + e, L.kept[e]);
                       if (rank + 1 == k_total)
                         result = Policy::state(L.kept[e]);
                     });
    }
  }
  return result;
}

struct Rounds
{
  uint32_t state;     // the engine state behind the k_total-th accepted attempt
  int rounds;
  uint64_t attempts;  // attempts evaluated
};

// host_rng.h: rng_rounds, with the two kernels and the scan replayed
template <typename Policy, typename Sink>
Rounds replay_rounds(const Policy& policy, uint32_t state_in, uint64_t k_total, Sink&& sink)
{
  Rounds res{ state_in, 0, 0 };
  uint32_t x0 = state_in;
  uint64_t accepted = 0;
  while (accepted < k_total)
  {
    ++res.rounds;
    const uint64_t n_att = policy.budget(k_total - accepted);
    res.attempts += n_att;
    const std::vector<uint32_t> counts = count_and_scan(policy, x0, n_att);
    const uint32_t result = emit_groups(policy, x0, n_att, counts, accepted, k_total, sink);
    accepted += counts.back();
    if (accepted >= k_total)
      res.state = result;
    else
      x0 = minstd_jump(x0, Policy::CALLS * n_att, g_table);
  }
  return res;
}
}  // namespace
