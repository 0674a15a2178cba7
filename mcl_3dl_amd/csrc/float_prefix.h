// float_prefix.h — dchain_prefix_wave's float sibling: the reference's float recurrence `accum += p.probability_;
// p.accum_probability_ = accum` (include/mcl_3dl/pf.h:193-197 / 401-405) and `pscan += pstep` (pf.h:421) run by a whole
// wavefront, with the serial loop's bits, and with EVERY prefix written out (std::lower_bound searches the array).
// float_chain.h returns the total only and is left as it is.
//
// The argument is float_chain.h's: while the running sum s stays inside one binade [2^e, 2^(e+1)) — ulp u = 2^(e-23) — it is a
// multiple of u, and a term t in [0, 2^(e-1)) that is not a rounding tie adds as fl(s + t) = s + RN_u(t) EXACTLY, RN_u(t) =
// (M + t) - M with M = 1.5 * 2^e. 64 lanes take FPREFIX_LANE_TERMS = 8 consecutive terms each, a wave prefix sum places every
// lane's partial behind its predecessors', and ONE pass retires 512 terms: lane l writes the eight prefixes s + (partials of
// lanes < l) + (its own roundings so far), all sums of multiples of u below 2^(e+1), exact in any association. (A prefix at or
// beyond 2^(e+1) may be inexact in the scan, but it is >= 2^(e+1) either way — adding non-negative terms is monotone — so the
// binade test `s + p < top` decides what it must.) What the shortcut cannot decide is left to real adds, in order: a rounding
// tie (|t - RN_u(t)| == u / 2), a term that is not small against s (t >= 2^(e-1)), negative (-0 included), NaN or infinite, and
// the step on which the sum leaves its binade. The first lane L with any of these is found by a ballot and every lane in front
// of it is final. L >= 1: lane L's eight terms are added serially (broadcast from its registers) and the next pass starts
// behind them, 8 L + 8 terms on. L == 0 — THE LANE-0 RULE: the next 64 terms are added serially instead of eight. A constant
// term whose low k mantissa bits are 1 0...0 is a rounding tie at EVERY step of the binade that drops k bits (pscan += pstep
// meets such a pstep), every pass there finds lane 0 in trouble, and eight terms a pass would make the chain slower than one
// lane; 64 serial adds cost about what a pass costs. A sum that is not a positive normal number with room for u / 2 and 2^(e+1)
// adds the next 64 terms serially too.
//
// The serial head: the sum of similar terms crosses a binade at terms 2, 4, 8, ..., and in the low binades ties are frequent,
// so the first FPREFIX_HEAD = 256 terms are added serially (four coalesced loads, 64 broadcasts each).
//
// The terms are an array (w) or ONE constant (w == nullptr: every term is `c`). The tie flag of the resampling step comes for
// free: a prefix equals its predecessor exactly when the term's rounding is 0 on the fast path, and the serial adds compare.
//
// fprefix_classify and the binade constants compile for the host too: tests/cpp/float_prefix_emul.cpp replays the passes lane
// by lane against the plain loop.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include "float_chain.h"  // wave_scan_add
#define FPREFIX_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define FPREFIX_HD
#endif

namespace mcl3dl
{
constexpr int FPREFIX_LANE_TERMS = 8;
constexpr int FPREFIX_PASS = 64 * FPREFIX_LANE_TERMS;
constexpr int FPREFIX_HEAD = 256;

FPREFIX_HD inline uint32_t fprefix_bits(float x)
{
  uint32_t u;
  memcpy(&u, &x, sizeof(u));
  return u;
}
FPREFIX_HD inline float fprefix_from_bits(uint32_t u)
{
  float x;
  memcpy(&x, &u, sizeof(x));
  return x;
}

struct FPrefixBinade
{
  float M, small, hu, top;  // 1.5 * 2^e, 2^(e-1), u / 2 = 2^(e-24), 2^(e+1)
};

// false: s is not a positive normal float whose u / 2 and 2^(e+1) are normal floats (0, tiny, negative, inf, NaN)
FPREFIX_HD inline bool fprefix_binade(float s, FPrefixBinade* b)
{
  const uint32_t bits = fprefix_bits(s);
  const uint32_t sb = bits & 0x7f800000u;
  if ((bits >> 31) || sb < (40u << 23) || sb >= (254u << 23))
    return false;
  b->M = fprefix_from_bits(sb | 0x00400000u);
  b->small = fprefix_from_bits(sb - (1u << 23));
  b->hu = fprefix_from_bits(sb - (24u << 23));
  b->top = fprefix_from_bits(sb + (1u << 23));
  return true;
}

// one term against the binade constants: its rounding to the ulp, and whether it is decidable without looking at s — in
// [+0, 2^(e-1)) (ONE unsigned compare of the bit pattern: anything negative, infinite or NaN has more) and not a rounding tie
FPREFIX_HD inline bool fprefix_classify(float t, const FPrefixBinade& b, float* r)
{
  *r = (b.M + t) - b.M;
  const float d = t - *r;
  return (fprefix_bits(t) < fprefix_bits(b.small)) & ((d < 0.0f ? -d : d) < b.hu);
}

#if defined(__HIPCC__)
__device__ inline float fprefix_lane(float v, int l)  // l: the same in every lane
{
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// term i of the chain: w[i], or the constant
__device__ inline float fprefix_term(const float* __restrict__ w, float c, long long i, long long n)
{
  return i < n ? (w ? w[i] : c) : 0.0f;
}

// `count` <= 64 terms from `at` on, serially: lane k holds term k, every lane follows the sum, lane k keeps prefix k (the
// loop is the dependent chain: a broadcast, an add and a select per term). *tie_lane |= this lane's prefix, i > 0, is not above
// its predecessor
__device__ inline float fprefix_serial(const float* __restrict__ w, float c, float* __restrict__ cum, long long n, long long at,
                                       int count, int lane, float s, bool* tie_lane)
{
  const float v = lane < count ? fprefix_term(w, c, at + lane, n) : 0.0f;
  const float s_in = s;
  float mine = 0.0f;
  const long long left = n - at;
  const int m = left < count ? static_cast<int>(left) : count;
  if (m == 64)
  {
#pragma unroll 16
    for (int k = 0; k < 64; ++k)
    {
      s = s + fprefix_lane(v, k);
      mine = lane == k ? s : mine;
    }
  }
  else
    for (int k = 0; k < m; ++k)
    {
      s = s + fprefix_lane(v, k);
      mine = lane == k ? s : mine;
    }
  const float up = __shfl_up(mine, 1);
  if (lane < m)
  {
    const float prev = lane == 0 ? s_in : up;
    cum[at + lane] = mine;
    *tie_lane |= (at + lane > 0) & !(prev < mine);
  }
  return s;
}

// cum[i] = fl(cum[i - 1] + term i) (cum[-1] = 0) for i < n, by ONE wavefront (all 64 lanes converged); returns the total, the
// same in every lane. *tie (the same in every lane): some i > 0 has !(cum[i - 1] < cum[i]). w and cum need no more than a
// float's alignment: the quad loads / stores are taken where the pointer is 16-byte aligned, scalar ones elsewhere.
__device__ inline float fprefix_wave(const float* __restrict__ w, float c, float* __restrict__ cum, long long n, int lane,
                                     bool* tie)
{
  float s = 0.0f;
  bool tied_lane = false;  // over this lane's own prefixes
  const bool quads_in = w && (reinterpret_cast<uintptr_t>(w) & 15u) == 0;
  const bool quads_out = (reinterpret_cast<uintptr_t>(cum) & 15u) == 0;
  long long q = 0;
  for (; q < FPREFIX_HEAD && q < n; q += 64)
    s = fprefix_serial(w, c, cum, n, q, 64, lane, s, &tied_lane);
  while (q < n)
  {
    s = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s)));  // (uniform anyway: keeps the constants scalar)
    FPrefixBinade b;
    if (!fprefix_binade(s, &b))
    {
      s = fprefix_serial(w, c, cum, n, q, 64, lane, s, &tied_lane);
      q += 64;
      continue;
    }
    // q is a multiple of 8 (the head is, and every step retires a multiple of 8 terms): the lane's eight terms are two
    // aligned quads wherever the row holds all of them
    const long long mine = q + static_cast<long long>(FPREFIX_LANE_TERMS) * lane;
    const bool whole = mine + FPREFIX_LANE_TERMS <= n;
    float t0, t1, t2, t3, t4, t5, t6, t7;
    if (whole && quads_in)
    {
      const float4 x = *reinterpret_cast<const float4*>(w + mine), y = *reinterpret_cast<const float4*>(w + mine + 4);
      t0 = x.x, t1 = x.y, t2 = x.z, t3 = x.w, t4 = y.x, t5 = y.y, t6 = y.z, t7 = y.w;
    }
    else
    {
      t0 = fprefix_term(w, c, mine + 0, n), t1 = fprefix_term(w, c, mine + 1, n);
      t2 = fprefix_term(w, c, mine + 2, n), t3 = fprefix_term(w, c, mine + 3, n);
      t4 = fprefix_term(w, c, mine + 4, n), t5 = fprefix_term(w, c, mine + 5, n);
      t6 = fprefix_term(w, c, mine + 6, n), t7 = fprefix_term(w, c, mine + 7, n);
    }
    float r0, r1, r2, r3, r4, r5, r6, r7;
    bool ok = fprefix_classify(t0, b, &r0);
    ok &= fprefix_classify(t1, b, &r1);
    ok &= fprefix_classify(t2, b, &r2);
    ok &= fprefix_classify(t3, b, &r3);
    ok &= fprefix_classify(t4, b, &r4);
    ok &= fprefix_classify(t5, b, &r5);
    ok &= fprefix_classify(t6, b, &r6);
    ok &= fprefix_classify(t7, b, &r7);
    // the lane's own prefixes (exact while the lane is ok and below top)
    const float a0 = r0, a1 = a0 + r1, a2 = a1 + r2, a3 = a2 + r3, a4 = a3 + r4, a5 = a4 + r5, a6 = a5 + r6, a7 = a6 + r7;
    const float p = wave_scan_add(a7);
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(!(ok & (s + p < b.top)));
    const int L = mask ? __builtin_ctzll(mask) : 64;
    if (L == 0)
    {
      // the lane-0 rule: nothing is final, the next 64 terms by real adds
      s = fprefix_serial(w, c, cum, n, q, 64, lane, s, &tied_lane);
      q += 64;
      continue;
    }
    if (lane < L)
    {
      const float base = s + (p - a7);  // exact: both are multiples of u below 2^(e+1)
      if (whole && quads_out)
      {
        *reinterpret_cast<float4*>(cum + mine) = make_float4(base + a0, base + a1, base + a2, base + a3);
        *reinterpret_cast<float4*>(cum + mine + 4) = make_float4(base + a4, base + a5, base + a6, base + a7);
        // a prefix stays where its predecessor is exactly when the term rounds to 0 (mine >= FPREFIX_HEAD > 0)
        tied_lane |= (r0 == 0.0f) | (r1 == 0.0f) | (r2 == 0.0f) | (r3 == 0.0f) | (r4 == 0.0f) | (r5 == 0.0f) | (r6 == 0.0f) |
                     (r7 == 0.0f);
      }
      else
      {
        // the row ends inside this lane's eight (terms behind it are +0 and round to 0: not ties), or cum is not quad-aligned
#define FPREFIX_STORE(k)                  \
  if (mine + k < n)                       \
  {                                       \
    cum[mine + k] = base + a##k;          \
    tied_lane |= r##k == 0.0f;            \
  }
        FPREFIX_STORE(0)
        FPREFIX_STORE(1)
        FPREFIX_STORE(2)
        FPREFIX_STORE(3)
        FPREFIX_STORE(4)
        FPREFIX_STORE(5)
        FPREFIX_STORE(6)
        FPREFIX_STORE(7)
#undef FPREFIX_STORE
      }
    }
    if (L == 64)
    {
      s = s + fprefix_lane(p, 63);
      q += FPREFIX_PASS;
      continue;
    }
    s = s + fprefix_lane(p, L - 1);
    // lane L's eight terms, in order, by real adds
    const long long at = q + static_cast<long long>(FPREFIX_LANE_TERMS) * L;
    const float x0 = fprefix_lane(t0, L), x1 = fprefix_lane(t1, L), x2 = fprefix_lane(t2, L), x3 = fprefix_lane(t3, L);
    const float x4 = fprefix_lane(t4, L), x5 = fprefix_lane(t5, L), x6 = fprefix_lane(t6, L), x7 = fprefix_lane(t7, L);
    const float s0 = s + x0, s1 = s0 + x1, s2 = s1 + x2, s3 = s2 + x3, s4 = s3 + x4, s5 = s4 + x5, s6 = s5 + x6, s7 = s6 + x7;
    const long long left = n - at;  // >= 1: a lane behind the row holds zeros and cannot be the first in trouble
    if (lane < FPREFIX_LANE_TERMS && lane < left)
    {
      const float prev = lane == 0 ? s : lane == 1 ? s0 : lane == 2 ? s1 : lane == 3 ? s2 : lane == 4 ? s3 : lane == 5 ? s4 : lane == 6 ? s5 : s6;
      const float cur = lane == 0 ? s0 : lane == 1 ? s1 : lane == 2 ? s2 : lane == 3 ? s3 : lane == 4 ? s4 : lane == 5 ? s5 : lane == 6 ? s6 : s7;
      cum[at + lane] = cur;
      tied_lane |= !(prev < cur);
    }
    // (terms behind the row are +0.0 and x + 0.0 == x except for x = -0.0, whose sum is not stored: s7 is the total only if
    // the row ends behind this lane, so take the last real prefix)
    s = left >= 8 ? s7 : left == 7 ? s6 : left == 6 ? s5 : left == 5 ? s4 : left == 4 ? s3 : left == 3 ? s2 : left == 2 ? s1 : s0;
    q = at + FPREFIX_LANE_TERMS;
  }
  *tie = __builtin_amdgcn_ballot_w64(tied_lane) != 0ull;
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s)));
}
#endif
}  // namespace mcl3dl
