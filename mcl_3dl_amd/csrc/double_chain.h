// double_chain.h — float_chain.h's fp64 sibling: the reference's double recurrence `cumulative_weight[i] = weight +
// cumulative_weight[i - 1]` (point_cloud_sampler_with_normal.h:157) run by a whole wavefront, with the serial loop's bits, and
// with EVERY prefix written out (the sampler bisects the array), not only the total.
//
// The argument is float_chain.h's with 52 for 23: while the running sum s stays inside one binade [2^e, 2^(e+1)) — ulp u =
// 2^(e-52) — it is a multiple of u, and a term t in [0, 2^(e-1)) that is not a rounding tie adds as fl(s + t) = s + RN_u(t)
// EXACTLY, RN_u(t) = (M + t) - M with M = 1.5 * 2^e. 64 lanes take DCHAIN_LANE_TERMS = 8 consecutive terms each, a wave prefix
// sum places every lane's partial behind its predecessors', and ONE pass retires 512 terms: lane l writes the eight prefixes
// s + (partials of lanes < l) + (its own roundings so far), all sums of multiples of u below 2^(e+1), exact in any association.
// (A prefix at or beyond 2^(e+1) may be inexact in the scan, but it is >= 2^(e+1) either way — adding non-negative terms is
// monotone — so the binade test `s + p < top` decides what it must.) What the shortcut cannot decide is left to real adds, in
// order: a rounding tie (|t - RN_u(t)| == u / 2), a term that is not small against s (t >= 2^(e-1)), negative (-0 included),
// NaN or infinite, and the step on which the sum leaves its binade. The first lane with any of these is found by a ballot,
// every lane in front of it is final, its eight terms are added serially (broadcast from its registers), and the next pass
// starts behind them. A sum that is not a positive normal number with room for u / 2 and 2^(e+1) adds the next 64 terms serially.
//
// The serial head: the sum of similar terms crosses a binade at terms 2, 4, 8, ..., and in the low binades ties are FREQUENT —
// a weight in [1, 2) has 52 fraction bits and a sum in [2^k, 2^(k+1)) drops k of them: a tie every 2^k terms or so —, so the
// first DCHAIN_HEAD = 256 terms are added serially (four coalesced loads, 64 broadcasts each). Behind it a pass retires about
// min(512, 2^k) terms. Weights that are all exactly 1.0 never tie and are never large (behind the head s >= 256): they leave
// the fast path only at the ~log2(n) binade edges.
//
// dchain_classify and the binade constants compile for the host too: tests/cpp/rng_weighted_emul.cpp replays the passes lane
// by lane against the plain loop.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DCHAIN_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define DCHAIN_HD
#endif

namespace mcl3dl
{
constexpr int DCHAIN_LANE_TERMS = 8;
constexpr int DCHAIN_PASS = 64 * DCHAIN_LANE_TERMS;
constexpr int DCHAIN_HEAD = 256;

DCHAIN_HD inline uint64_t dchain_bits(double x)
{
  uint64_t u;
  memcpy(&u, &x, sizeof(u));
  return u;
}
DCHAIN_HD inline double dchain_from_bits(uint64_t u)
{
  double x;
  memcpy(&x, &u, sizeof(x));
  return x;
}

struct DChainBinade
{
  double M, small, hu, top;  // 1.5 * 2^e, 2^(e-1), u / 2 = 2^(e-53), 2^(e+1)
};

// false: s is not a positive normal double whose u / 2 and 2^(e+1) are normal doubles (0, tiny, negative, inf, NaN)
DCHAIN_HD inline bool dchain_binade(double s, DChainBinade* b)
{
  const uint64_t bits = dchain_bits(s);
  const uint64_t sb = bits & 0x7ff0000000000000ull;
  if ((bits >> 63) || sb < (60ull << 52) || sb >= (2046ull << 52))
    return false;
  b->M = dchain_from_bits(sb | 0x0008000000000000ull);
  b->small = dchain_from_bits(sb - (1ull << 52));
  b->hu = dchain_from_bits(sb - (53ull << 52));
  b->top = dchain_from_bits(sb + (1ull << 52));
  return true;
}

// one term against the binade constants: its rounding to the ulp, and whether it is decidable without looking at s — in
// [+0, 2^(e-1)) (ONE unsigned compare of the bit pattern: anything negative, infinite or NaN has more) and not a rounding tie
DCHAIN_HD inline bool dchain_classify(double t, const DChainBinade& b, double* r)
{
  *r = (b.M + t) - b.M;
  const double d = t - *r;
  return (dchain_bits(t) < dchain_bits(b.small)) & ((d < 0.0 ? -d : d) < b.hu);
}

#if defined(__HIPCC__)
__device__ inline double dchain_wave_scan(double v, int lane)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const double o = __shfl_up(v, d);
    v = lane >= d ? v + o : v;
  }
  return v;
}

// `count` <= 64 terms from w[at] on, serially: lane k holds term k, every lane follows the sum, lane k keeps prefix k
__device__ inline double dchain_serial(const double* __restrict__ w, double* __restrict__ cum, long long n, long long at,
                                       int count, int lane, double s)
{
  const double v = (lane < count && at + lane < n) ? w[at + lane] : 0.0;
  double mine = 0.0;
  for (int k = 0; k < count && at + k < n; ++k)
  {
    s = s + __shfl(v, k);
    mine = lane == k ? s : mine;
  }
  if (lane < count && at + lane < n)
    cum[at + lane] = mine;
  return s;
}

// cum[i] = w[i] + cum[i - 1] (cum[-1] = 0) for i < n, by ONE wavefront (all 64 lanes converged); returns the total
__device__ inline double dchain_prefix_wave(const double* __restrict__ w, double* __restrict__ cum, long long n, int lane)
{
  double s = 0.0;
  long long q = 0;
  for (; q < DCHAIN_HEAD && q < n; q += 64)
    s = dchain_serial(w, cum, n, q, 64, lane, s);
  while (q < n)
  {
    DChainBinade b;
    if (!dchain_binade(s, &b))
    {
      s = dchain_serial(w, cum, n, q, 64, lane, s);
      q += 64;
      continue;
    }
    const long long mine = q + static_cast<long long>(DCHAIN_LANE_TERMS) * lane;
    double t0 = mine + 0 < n ? w[mine + 0] : 0.0, t1 = mine + 1 < n ? w[mine + 1] : 0.0;
    double t2 = mine + 2 < n ? w[mine + 2] : 0.0, t3 = mine + 3 < n ? w[mine + 3] : 0.0;
    double t4 = mine + 4 < n ? w[mine + 4] : 0.0, t5 = mine + 5 < n ? w[mine + 5] : 0.0;
    double t6 = mine + 6 < n ? w[mine + 6] : 0.0, t7 = mine + 7 < n ? w[mine + 7] : 0.0;
    double r0, r1, r2, r3, r4, r5, r6, r7;
    bool ok = dchain_classify(t0, b, &r0);
    ok &= dchain_classify(t1, b, &r1);
    ok &= dchain_classify(t2, b, &r2);
    ok &= dchain_classify(t3, b, &r3);
    ok &= dchain_classify(t4, b, &r4);
    ok &= dchain_classify(t5, b, &r5);
    ok &= dchain_classify(t6, b, &r6);
    ok &= dchain_classify(t7, b, &r7);
    // the lane's own prefixes (exact while the lane is ok and below top)
    const double a0 = r0, a1 = a0 + r1, a2 = a1 + r2, a3 = a2 + r3, a4 = a3 + r4, a5 = a4 + r5, a6 = a5 + r6, a7 = a6 + r7;
    const double p = dchain_wave_scan(a7, lane);
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(!(ok & (s + p < b.top)));
    const int L = mask ? __builtin_ctzll(mask) : 64;
    if (lane < L)
    {
      const double base = s + (p - a7);  // exact: both are multiples of u below 2^(e+1)
      if (mine + 0 < n) cum[mine + 0] = base + a0;
      if (mine + 1 < n) cum[mine + 1] = base + a1;
      if (mine + 2 < n) cum[mine + 2] = base + a2;
      if (mine + 3 < n) cum[mine + 3] = base + a3;
      if (mine + 4 < n) cum[mine + 4] = base + a4;
      if (mine + 5 < n) cum[mine + 5] = base + a5;
      if (mine + 6 < n) cum[mine + 6] = base + a6;
      if (mine + 7 < n) cum[mine + 7] = base + a7;
    }
    if (L == 64)
    {
      s = s + __shfl(p, 63);
      q += DCHAIN_PASS;
      continue;
    }
    if (L > 0)
      s = s + __shfl(p, L - 1);
    // lane L's eight terms, in order, by real adds
    const long long at = q + static_cast<long long>(DCHAIN_LANE_TERMS) * L;
    const double x0 = __shfl(t0, L), x1 = __shfl(t1, L), x2 = __shfl(t2, L), x3 = __shfl(t3, L);
    const double x4 = __shfl(t4, L), x5 = __shfl(t5, L), x6 = __shfl(t6, L), x7 = __shfl(t7, L);
    const double s0 = s + x0, s1 = s0 + x1, s2 = s1 + x2, s3 = s2 + x3, s4 = s3 + x4, s5 = s4 + x5, s6 = s5 + x6, s7 = s6 + x7;
    if (lane < DCHAIN_LANE_TERMS && at + lane < n)
      cum[at + lane] = lane == 0 ? s0 : lane == 1 ? s1 : lane == 2 ? s2 : lane == 3 ? s3 : lane == 4 ? s4 : lane == 5 ? s5 : lane == 6 ? s6 : s7;
    // (terms behind the row are +0.0 and x + 0.0 == x except for x = -0.0, whose sum is not stored: s7 is the total only if
    // the row ends behind this lane, so take the last real prefix)
    const long long left = n - at;
    s = left >= 8 ? s7 : left == 7 ? s6 : left == 6 ? s5 : left == 5 ? s4 : left == 4 ? s3 : left == 3 ? s2 : left == 2 ? s1 : s0;
    q = at + DCHAIN_LANE_TERMS;
  }
  return s;
}
#endif
}  // namespace mcl3dl
