// rng_weighted.h — the draw of the reference's normal-weighted scan sampler (PointCloudSamplerWithNormal::sample,
// point_cloud_sampler_with_normal.h:159-177) restated so that every attempt of its loop can be evaluated at once
// (rng_weighted_kernels.h runs it on the device, tests/cpp/rng_weighted_emul.cpp on the CPU with g++: no HIP type appears here).
//
// PINNED TO libstdc++, as rng_polar.h and rng_index.h are. Given the cumulative weights cum[0 .. n) (double_chain.h):
//
//   THE DRAW  std::uniform_real_distribution<double>(0, b)(engine), b = cum[n - 1], is generate_canonical<double, 53> over
//     minstd_rand0: range r = max - min + 1 = 2147483646, log2(r) < 31, so m = max(1, ceil(53 / 30)) = 2 engine calls v1, v2 and
//     no rejection:  sum = (double)(v1 - 1); sum += (double)(v2 - 1) * r; c = sum / (r * r); c >= 1 becomes nextafter(1, 0);
//     the value is c * (b - 0) + 0. All of it double arithmetic with contraction off. ATTEMPT t of the sampler's loop uses engine
//     outputs 2t + 1 and 2t + 2, whatever the earlier attempts drew.
//     The c >= 1 branch: the numerator is at most r^2 - 1, and c can round to 1 only when v2 = 2^31 - 2 and v1 is within a few
//     hundred of r. v2 is 16807 v1 mod (2^31 - 1), so v2 = 2^31 - 2 has the single predecessor v1 = 2^31 - 1 - 16807^-1 =
//     739806647 (WEIGHTED_V1_BEFORE_MAX; the CPU test recomputes it), which is 1.4e9 below r: the largest c of the stream is
//     0.99999999969475872, and NO pair of consecutive outputs reaches the branch. It is kept as the library has it.
//   std::lower_bound  the library's bisection (len / half / middle), literally, on the double array: the result is what the
//     library returns whether or not the array is sorted.
//   DUPLICATES  the loop inserts the drawn id into a std::unordered_set<size_t> until it holds `num` ids. An attempt is NEW if no
//     earlier attempt drew its id: first_attempt[id] = min over the attempts that drew id of the attempt's number (atomicMin), new
//     iff it holds that minimum. The k-th new attempt (prefix count) inserts the k-th id; the attempt T that inserts the num-th
//     id is the last one made: 2 (T + 1) engine calls in all. first_attempt persists over passes / rounds (later ones carry
//     larger numbers).
//   CONTAINER ORDER  the sampled cloud is pushed back in the set's ITERATION order. libstdc++'s unordered_set<size_t>: identity
//     hash, max load 1, one singly linked list of all nodes; bucket counts 1 -> 13 -> 29 -> 59 -> ... (WEIGHTED_BUCKETS: the
//     growth policy _M_need_rehash asks _M_next_bkt for max(k, 2 b) — 11 on the first insertion — and gets the next entry of
//     the library's prime list), a rehash BEFORE inserting element k when k exceeds the bucket count. A node entering an empty
//     bucket goes to the front of the whole list, a node entering an occupied bucket to the front of that bucket's run
//     (_M_insert_bucket_begin); a rehash (_M_rehash_aux) re-inserts all nodes in the current iteration order by the same rule.
//     So per PHASE (one bucket count b, m = min(num, b) ids at its end) the arrival sequence is the previous phase's final order
//     followed by the ids inserted during the phase, and the final order sorts by (first arrival of the id's bucket id % b,
//     descending; own arrival, descending). No comparison sort is needed: chains per bucket (an atomic exchange on the bucket's
//     head) give every arrival its bucket's size, first arrival and the number of later arrivals in its bucket; an exclusive
//     scan of the sizes parked at the first arrivals gives the bucket's offset from the back. Integers only, any thread count.
//
// TERMINATION  the loop ends for sure when every weight is finite and >= 1, n > num, and the total is below WEIGHTED_MAX_TOTAL =
// 2^50: cum is then strictly increasing (a term >= 1 is at least half an ulp of any sum below 2^53), every id owns an interval of
// length >= 1, and consecutive attainable draw values are at most b 2^-53 + ulp(b) <= 2^-3 + 2^-2 apart (every double in
// [2^-9, 1) is a c: the canonical grid 1 / r^2 < 2^-61 is finer than the doubles there; below 2^-9 the c are the grid itself),
// so every id is drawn by some engine state pair with positive frequency over the engine's full period.
#pragma once

#include <cmath>
#include <cstdint>

#include "rng_polar.h"

namespace mcl3dl
{
namespace rng
{
constexpr double WEIGHTED_RANGE = 2147483646.0;                // minstd_rand0::max() - min() + 1
constexpr double WEIGHTED_MAX_TOTAL = 1125899906842624.0;      // 2^50
constexpr uint32_t WEIGHTED_V1_BEFORE_MAX = 739806647u;        // the one v1 whose next output is 2^31 - 2
constexpr int WEIGHTED_E = 4;                                  // consecutive attempts one lane walks behind its jump
constexpr uint32_t WEIGHTED_PASS = GROUP_THREADS * WEIGHTED_E;  // attempts of one pass of the one-work-group form
// the one-work-group form serves a segment of at most this many sampled points (its order phases live in LDS; a bucket count, so
// that a phase never exceeds it). A starting value, untimed.
constexpr uint32_t WEIGHTED_SINGLE_MAX = 1109u;
constexpr uint32_t WEIGHTED_NONE = 0xffffffffu;
constexpr uint64_t WEIGHTED_MAX_ATTEMPTS = 0xfffffff0ull;  // attempt numbers are 32-bit words

// bucket counts of std::unordered_set<size_t> grown by single insertions (tests/cpp/rng_weighted_emul.cpp holds it against the
// container's bucket_count())
constexpr int WEIGHTED_N_BUCKETS = 28;
#define MCL3DL_WEIGHTED_BUCKET_LIST                                                                                              \
  {                                                                                                                              \
    13ull, 29ull, 59ull, 127ull, 257ull, 541ull, 1109ull, 2357ull, 5087ull, 10273ull, 20753ull, 42043ull, 85229ull, 172933ull,   \
        351061ull, 712697ull, 1447153ull, 2938679ull, 5967347ull, 12117689ull, 24607243ull, 49969847ull, 101473717ull,           \
        206062531ull, 418451333ull, 849749479ull, 1725587117ull, 3504151727ull                                                  \
  }
RNG_HD inline uint64_t weighted_bucket_count(int phase)
{
  constexpr uint64_t t[WEIGHTED_N_BUCKETS] = MCL3DL_WEIGHTED_BUCKET_LIST;
  return t[phase];
}

// v1, v2: two consecutive engine outputs in [1, 2^31 - 2]
RNG_HD inline double weighted_canonical(uint32_t v1, uint32_t v2)
{
  double sum = static_cast<double>(v1 - 1u);
  sum += static_cast<double>(v2 - 1u) * WEIGHTED_RANGE;
  const double c = sum / (WEIGHTED_RANGE * WEIGHTED_RANGE);
  return c >= 1.0 ? 0x1.fffffffffffffp-1 : c;  // nextafter(1, 0)
}

// uniform_real_distribution<double>(0, b): c * (b - a) + a
RNG_HD inline double weighted_value(double c, double b)
{
  return c * (b - 0.0) + 0.0;
}

// std::lower_bound(cum, cum + n, x) - cum (bits/stl_algobase.h:__lower_bound)
RNG_HD inline uint32_t weighted_lower_bound(const double* cum, uint32_t n, double x)
{
  uint32_t first = 0u, len = n;
  while (len > 0u)
  {
    const uint32_t half = len >> 1;
    const uint32_t middle = first + half;
    if (cum[middle] < x)
    {
      first = middle + 1u;
      len = len - half - 1u;
    }
    else
      len = half;
  }
  return first;
}

// How many attempts one round of the rounds form evaluates when `have` of the `num` ids are there, n points in the cloud: the
// coupon collector's expectation for equal weights, n (H(n - have) - H(n - num)) ~ n log((n - have + 1/2) / (n - num + 1/2)), plus
// a quarter and a pass. A starting value, not a tuned one: weights up to max_weight make duplicates more frequent than that, and
// the next round draws what is missing.
inline uint64_t weighted_attempt_budget(uint64_t have, uint64_t num, uint64_t n)
{
  const double e = static_cast<double>(n) * std::log((static_cast<double>(n - have) + 0.5) / (static_cast<double>(n - num) + 0.5));
  const uint64_t b = static_cast<uint64_t>(std::ceil(1.25 * e)) + WEIGHTED_PASS;
  return b < num - have ? num - have : b;
}

// ---- the steps, written per thread (tid of nthreads): the kernels run them with barriers or launches in between, the CPU
// emulation thread after thread. Atomics: the device's on the device, plain words on the host (one thread at a time there).
#if defined(__HIP_DEVICE_COMPILE__)
#define WEIGHTED_ATOMIC_MIN(p, v) atomicMin((p), (v))
#define WEIGHTED_ATOMIC_EXCH(p, v) atomicExch((p), (v))
// a word other lanes of the launch reached with an atomic: read it where the atomic landed, past this compute unit's cache
#define WEIGHTED_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
inline uint32_t weighted_host_min(uint32_t* p, uint32_t v)
{
  const uint32_t old = *p;
  if (v < old)
    *p = v;
  return old;
}
inline uint32_t weighted_host_exch(uint32_t* p, uint32_t v)
{
  const uint32_t old = *p;
  *p = v;
  return old;
}
#define WEIGHTED_ATOMIC_MIN(p, v) weighted_host_min((p), (v))
#define WEIGHTED_ATOMIC_EXCH(p, v) weighted_host_exch((p), (v))
#define WEIGHTED_LOAD(p) (*(p))
#endif

struct WeightedCloud
{
  const double* cum;  // n cumulative weights
  uint32_t n;
  uint32_t* first;  // n words, WEIGHTED_NONE before the first attempt
};

// attempts [0, n_att) behind engine state x0, numbered t_base + t: att_id[t] = the drawn id, first[id] = min(attempt number).
// An id of n (a value above every cumulative weight: not with the weights the callers admit) is recorded but owns no word.
RNG_HD inline void weighted_step_draw(uint32_t tid, uint32_t nthreads, uint32_t x0, const uint32_t* table, const WeightedCloud& c,
                                      uint32_t t_base, uint32_t n_att, uint32_t* att_id)
{
  const double b = c.cum[c.n - 1u];
  for (uint32_t t0 = tid * WEIGHTED_E; t0 < n_att; t0 += nthreads * WEIGHTED_E)
  {
    uint32_t x = minstd_jump(x0, 2ull * t0, table);
    for (uint32_t e = 0; e < WEIGHTED_E && t0 + e < n_att; ++e)
    {
      const uint32_t v1 = minstd_next(x);
      x = minstd_next(v1);
      const uint32_t id = weighted_lower_bound(c.cum, c.n, weighted_value(weighted_canonical(v1, x), b));
      att_id[t0 + e] = id;
      if (id < c.n)
        WEIGHTED_ATOMIC_MIN(&c.first[id], t_base + t0 + e);
    }
  }
}

// flag[t] = 1 for a new attempt; flag[n_att] = 0 (the exclusive scan leaves the total there)
RNG_HD inline void weighted_step_flag(uint32_t tid, uint32_t nthreads, const WeightedCloud& c, uint32_t t_base, uint32_t n_att,
                                      const uint32_t* att_id, uint32_t* flag)
{
  for (uint32_t t = tid; t <= n_att; t += nthreads)
    flag[t] = (t < n_att && att_id[t] < c.n && WEIGHTED_LOAD(&c.first[att_id[t]]) == t_base + t) ? 1u : 0u;
}

// scanned: the exclusive scan of flag (n_att + 1 words). The new attempt of rank r = have + scanned[t] < num inserts ins[r]; the
// one of rank num - 1 reports result[0] = the engine state behind it and result[1] = the attempts made in all.
RNG_HD inline void weighted_step_emit(uint32_t tid, uint32_t nthreads, uint32_t x0, const uint32_t* table, uint32_t t_base,
                                      uint32_t n_att, const uint32_t* att_id, const uint32_t* scanned, uint32_t have, uint32_t num,
                                      uint32_t* ins, uint32_t* result)
{
  for (uint32_t t = tid; t < n_att; t += nthreads)
  {
    if (scanned[t + 1u] == scanned[t])
      continue;
    const uint32_t r = have + scanned[t];
    if (r < num)
      ins[r] = att_id[t];
    if (r + 1u == num)
    {
      result[0] = minstd_jump(x0, 2ull * t + 2ull, table);
      result[1] = t_base + t + 1u;
    }
  }
}

// One phase of the container's order: b buckets, m arrivals of which the first m_prev are cur[] (the previous phase's order) and
// the rest ins[m_prev .. m) (arrival p >= m_prev IS insertion rank p: m_prev ids were there before).
struct WeightedPhase
{
  uint32_t b, m, m_prev;
  const uint32_t *cur, *ins;
  uint32_t *head /* b */, *link /* m */, *first_of /* m */, *later /* m */, *size_at /* m + 1 */, *next /* m: the new order */;
};

RNG_HD inline uint32_t weighted_arrival(const WeightedPhase& ph, uint32_t p)
{
  return p < ph.m_prev ? ph.cur[p] : ph.ins[p];
}

RNG_HD inline void weighted_phase_clear(uint32_t tid, uint32_t nthreads, const WeightedPhase& ph)
{
  for (uint32_t k = tid; k < ph.b; k += nthreads)
    ph.head[k] = WEIGHTED_NONE;
}

// the arrivals of one bucket as a chain in whatever order the exchanges landed: only sets are read from it
RNG_HD inline void weighted_phase_link(uint32_t tid, uint32_t nthreads, const WeightedPhase& ph)
{
  for (uint32_t p = tid; p < ph.m; p += nthreads)
    ph.link[p] = WEIGHTED_ATOMIC_EXCH(&ph.head[weighted_arrival(ph, p) % ph.b], p);
}

RNG_HD inline void weighted_phase_walk(uint32_t tid, uint32_t nthreads, const WeightedPhase& ph)
{
  for (uint32_t p = tid; p <= ph.m; p += nthreads)
  {
    if (p == ph.m)
    {
      ph.size_at[p] = 0u;
      continue;
    }
    uint32_t size = 0u, first = p, later = 0u;
    for (uint32_t q = ph.head[weighted_arrival(ph, p) % ph.b]; q != WEIGHTED_NONE; q = ph.link[q])
    {
      ++size;
      first = q < first ? q : first;
      later += q > p ? 1u : 0u;
    }
    ph.first_of[p] = first;
    ph.later[p] = later;
    ph.size_at[p] = first == p ? size : 0u;
  }
}

// scanned: the exclusive scan of size_at (m + 1 words). Buckets with a later first arrival come first: m - scanned[first + 1] ids
// stand in front of the bucket whose first arrival is `first`, and inside it the later arrivals.
RNG_HD inline void weighted_phase_place(uint32_t tid, uint32_t nthreads, const WeightedPhase& ph, const uint32_t* scanned)
{
  for (uint32_t p = tid; p < ph.m; p += nthreads)
    ph.next[ph.m - scanned[ph.first_of[p] + 1u] + ph.later[p]] = weighted_arrival(ph, p);
}

// the phases of `num` ids: phase j has weighted_bucket_count(j) buckets and ends with min(num, that) ids
RNG_HD inline int weighted_phase_count(uint64_t num)
{
  int j = 0;
  while (j + 1 < WEIGHTED_N_BUCKETS && weighted_bucket_count(j) < num)
    ++j;
  return j + 1;
}
}  // namespace rng
}  // namespace mcl3dl
