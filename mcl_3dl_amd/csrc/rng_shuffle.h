// rng_shuffle.h — std::shuffle(iota(n), engine_) of pf::covariance (pf.h:320-333) restated so that the first m entries of the
// result can be had without running the swaps one after the other (rng_shuffle_kernels.h runs it on the device,
// tests/cpp/rng_shuffle_emul.cpp on the CPU with g++: no HIP type appears here).
//
// PINNED TO libstdc++, as rng_index.h is. The engine is minstd_rand0, R = urngrange = 2147483645. bits/stl_algo.h, std::shuffle
// over n elements: for i = 1 .. n - 1 in order, swap(a[i], a[j_i]) with j_i in [0, i]. The j_i come in one of two ways:
//
//   PAIR PATH    R / n >= n, i.e. n <= 46340. n even: j_1 from uniform_int_distribution<size_t>(0, 1) first. Then ONE draw x from
//                (0, (i + 1)(i + 2) - 1) gives j_i = x / (i + 2) and j_(i+1) = x % (i + 2). Rejection reaches tens of per cent and
//                depends on the step, the path never exceeds 27 000 engine calls (0.1 ms on a core): IT STAYS ON THE HOST
//                (shuffle_serial below), the caller uploads the m indices.
//   SINGLE PATH  n >= 46341: j_i from uniform_int_distribution<size_t>(0, i), which is rng_index.h's range of i + 1 values:
//                scaling_i = R / (i + 1), past_i = (i + 1) scaling_i, reject while ret = engine() - 1 >= past_i, j_i = ret / scaling_i.
//                THE DEVICE PATH. Its two serial dependences both have a parallel form:
//
//   Which step an attempt belongs to. Attempt t uses engine output t + 1 behind the start state. past_i = R - (R mod (i + 1)) >=
//   R - i, so an attempt with ret <= R - n is accepted at whatever step it arrives. Only the attempts with ret > R - n are
//   DOUBTFUL, about n^2 / 2^31 of them (1 at 46 341, 94 at 450 408). They are compacted in stream order and resolved in order:
//   step = 1 + t - (rejected so far), accepted iff ret < past_step (shuffle_resolve). That leaves the sorted list of rejected attempt
//   numbers, every attempt's step is 1 + t - (rejections before t), and the state behind the shuffle is the start state advanced
//   by (n - 1) + rejections: an attempt behind the last accepted one is never consumed.
//
//   The first m entries without the swaps. Position i is untouched before step i. Let f(q, L) be the content of position q after
//   the steps < L (q < L):  some step i with q < i < L has j_i == q: f is the LARGEST such i;  otherwise q == 0: 0;  otherwise
//   j_q == q: q;  otherwise f(j_q, q).  a[p] after the shuffle is f(p, n). The steps that hit a position come from a STABLE sort of
//   the pairs (j_i, i - 1) by j_i, emitted in ascending i: the sorted array is then ascending in (j, i) as a pair, and "the largest
//   i < L that hit q" is one binary search (shuffle_chain_step). The hop q -> j_q halves q on average; the walk ends at q == 0
//   at the latest.
//
// pf::covariance's sample_num (pf.h:326-331, FLT_TYPE = float) is shuffle_sample_count. What this project does NOT restate: the
// early `break` of pf.h:316 once the float weight sum passes pass_ratio — p_num is n, as in every covariance here.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rng_index.h"

namespace mcl3dl
{
namespace rng
{
constexpr uint64_t SHUFFLE_MAX_N = 2147483646ull;  // the largest range rng_index.h restates
// How many standard deviations of the doubtful count one round's attempt budget adds (a starting value, untimed: as
// index_attempt_budget's three).
constexpr double SHUFFLE_BUDGET_SIGMAS = 3.0;

// libstdc++'s test, "(__urngrange >= __urange * __urange) but without wrap issues": n <= 46340
RNG_HD inline bool shuffle_pair_path(uint64_t n)
{
  return INDEX_URNG_RANGE / n >= n;
}

// step i draws from [0, i]: index_range(i + 1) in 32-bit arithmetic (i + 1 <= 2147483646)
RNG_HD inline IndexRange shuffle_step_range(uint32_t i)
{
  const uint32_t range = i + 1u;
  IndexRange r;
  if (range > static_cast<uint32_t>(INDEX_URNG_RANGE))
  {
    r.scaling = 1u;
    r.past = static_cast<uint32_t>(INDEX_MAX_RANGE);
    return r;
  }
  r.scaling = static_cast<uint32_t>(INDEX_URNG_RANGE) / range;
  r.past = range * r.scaling;
  return r;
}

// v: one engine output. An attempt that is not doubtful is accepted at every step of a shuffle over n elements.
RNG_HD inline bool shuffle_doubtful(uint32_t v, uint64_t n)
{
  return static_cast<uint64_t>(v - 1u) + n > INDEX_URNG_RANGE;
}

enum
{
  SHUFFLE_ACCEPTED = 0,
  SHUFFLE_REJECTED = 1,
  SHUFFLE_BEYOND = 2  // the shuffle was complete before this attempt: it is never consumed
};

// doubtful attempt t (engine output v) with `rejected` rejections among the attempts before it
RNG_HD inline int shuffle_resolve(uint64_t t, uint32_t v, uint64_t rejected, uint64_t n)
{
  const uint64_t step = 1u + t - rejected;
  if (step > n - 1u)
    return SHUFFLE_BEYOND;
  return index_accepted(shuffle_step_range(static_cast<uint32_t>(step)), v) ? SHUFFLE_ACCEPTED : SHUFFLE_REJECTED;
}

// j_i of an accepted attempt
RNG_HD inline uint32_t shuffle_target(uint32_t step, uint32_t v)
{
  return index_value(shuffle_step_range(step), v);
}

// How many attempts from the start of the stream a round evaluates when `accepted` of the n - 1 steps are known to lie in the
// `evaluated` attempts behind it: what is missing, plus the expected number of doubtful attempts among them (an upper bound of
// the rejections: each attempt is doubtful with n / 2^31) and SHUFFLE_BUDGET_SIGMAS standard deviations of that (Poisson) count,
// plus one. A second round is rare; it evaluates the longer stream from the start.
inline uint64_t shuffle_attempt_budget(uint64_t evaluated, uint64_t accepted, uint64_t n)
{
  const double k = static_cast<double>(n - 1u - accepted);
  const double d = k * static_cast<double>(n) / 2147483646.0;
  return evaluated + static_cast<uint64_t>(k) + static_cast<uint64_t>(std::ceil(d + SHUFFLE_BUDGET_SIGMAS * std::sqrt(d))) + 1u;
}

// rng_stream.h's attempt policy of the doubtful attempts: "accepted" means doubtful, to be compacted in stream order
struct DoubtPolicy
{
  unsigned long long n;
  static constexpr int CALLS = 1;
  using Kept = uint32_t;
  RNG_HD bool judge(const uint32_t* v, Kept* k) const
  {
    *k = v[0];
    return shuffle_doubtful(v[0], n);
  }
  RNG_HD static uint32_t state(const Kept& k) { return k; }
  uint64_t budget(uint64_t evaluated, uint64_t accepted) const { return shuffle_attempt_budget(evaluated, accepted, n); }
};

// Sorted pairs: keys[k] = j_i ascending, steps[k] = i - 1, ascending within one key (count = n - 1 of them).
// The first position whose pair (j, i) is not below (q, L).
RNG_HD inline uint32_t shuffle_lower_bound(const uint32_t* keys, const uint32_t* steps, uint32_t count, uint32_t q, uint32_t L)
{
  uint32_t lo = 0u, len = count;
  while (len > 0u)
  {
    const uint32_t half = len >> 1;
    const uint32_t k = keys[lo + half];
    if (k < q || (k == q && steps[lo + half] + 1u < L))
    {
      lo += half + 1u;
      len -= half + 1u;
    }
    else
      len = half;
  }
  return lo;
}

// One step of the walk for f(*q, *L). target[i] = j_i, i in [1, n - 1]. true: *value = f; false: (*q, *L) is the next pair.
RNG_HD inline bool shuffle_chain_step(const uint32_t* keys, const uint32_t* steps, uint32_t count, const uint32_t* target,
                                      uint32_t* q, uint32_t* L, uint32_t* value)
{
  const uint32_t pos = shuffle_lower_bound(keys, steps, count, *q, *L);
  // the pair in front of it is the largest (j, i) below (q, L): a hit of q unless it is q's own step or another position's
  if (pos > 0u && keys[pos - 1u] == *q && steps[pos - 1u] + 1u != *q)
  {
    *value = steps[pos - 1u] + 1u;
    return true;
  }
  if (*q == 0u)
  {
    *value = 0u;
    return true;
  }
  const uint32_t j = target[*q];
  if (j == *q)
  {
    *value = *q;
    return true;
  }
  *L = *q;
  *q = j;
  return false;
}

// f(p, n): the walk is bounded by p (q falls with every hop)
RNG_HD inline uint32_t shuffle_entry(const uint32_t* keys, const uint32_t* steps, uint32_t n, const uint32_t* target, uint32_t p,
                                     uint32_t* hops)
{
  uint32_t q = p, L = n, value = 0u, h = 0u;
  while (!shuffle_chain_step(keys, steps, n - 1u, target, &q, &L, &value))
    ++h;
  if (hops)
    *hops = h;
  return value;
}

// ---- the serial forms (host) ---------------------------------------------------------------------------------------------------
// uniform_int_distribution<size_t>(0, range - 1)(engine): bits/uniform_int_dist.h's loop, range in [1, 2147483646]
inline uint32_t shuffle_draw(uint32_t* state, uint64_t range, uint64_t* attempts)
{
  const IndexRange r = index_range(range);
  uint32_t x = *state;
  do
  {
    x = minstd_next(x);
    if (attempts)
      ++*attempts;
  } while (!index_accepted(r, x));
  *state = x;
  return index_value(r, x);
}

// std::shuffle(a, a + n, engine) with a = iota(n): the loop of bits/stl_algo.h, both paths. force_single: the single path
// whatever n is (what the device path computes; libstdc++ takes it from n = 46341 on). *attempts: engine calls made.
inline void shuffle_serial(uint64_t n, uint32_t* state, uint32_t* a, bool force_single, uint64_t* attempts)
{
  for (uint64_t i = 0; i < n; ++i)
    a[i] = static_cast<uint32_t>(i);
  if (attempts)
    *attempts = 0;
  if (n < 2)
    return;
  const auto swap_at = [a](uint64_t i, uint32_t j)
  {
    const uint32_t t = a[i];
    a[i] = a[j];
    a[j] = t;
  };
  if (force_single || !shuffle_pair_path(n))
  {
    for (uint64_t i = 1; i < n; ++i)
      swap_at(i, shuffle_draw(state, i + 1, attempts));
    return;
  }
  uint64_t i = 1;
  if (n % 2 == 0)
  {
    swap_at(i, shuffle_draw(state, 2, attempts));
    ++i;
  }
  while (i < n)
  {
    const uint64_t swap_range = i + 1;
    const uint32_t x = shuffle_draw(state, swap_range * (swap_range + 1), attempts);  // at most 46339 * 46340 < R
    swap_at(i, static_cast<uint32_t>(x / (swap_range + 1)));
    swap_at(i + 1, static_cast<uint32_t>(x % (swap_range + 1)));
    i += 2;
  }
}

// pf.h:326-331 with FLT_TYPE = float: min(p_num, max(size_t(0), static_cast<size_t>(p_num * random_sample_ratio))), a FLOAT
// product, truncated. The caller has refused a NaN or negative ratio (the conversion would be undefined).
inline size_t shuffle_sample_count(size_t n, float ratio)
{
  const float product = static_cast<float>(n) * ratio;
  if (!(product < 18446744073709551616.0f))
    return n;
  const size_t s = static_cast<size_t>(product);
  return s < n ? s : n;
}
}  // namespace rng
}  // namespace mcl3dl
