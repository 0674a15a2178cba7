// rng_polar.h — the reference's random stream restated so that every position of it can be evaluated at once
// (rng_stream.h walks it, rng_kernels.h holds what the device adds, tests/cpp/rng_polar_emul.cpp replays it on the CPU with g++:
// no HIP type appears here).
//
// PINNED TO libstdc++, as oracle/_ref is: std::default_random_engine is minstd_rand0 there, x <- 16807 x mod (2^31 - 1),
// seeded with seed mod (2^31 - 1), 0 -> 1. Another standard library uses another engine; this header does not follow it.
//
//   generate_canonical<float, 24> (bits/random.tcc): one engine call v in [1, 2^31 - 2]; c = (float)(v - 1) / 2147483648.0f
//     (the range 2147483646 narrows to that float); c >= 1 becomes nextafterf(1, 0) — (float)2147483645 IS 2^31.
//   normal_distribution<float>(mean, sigma): do { x = 2c1 - 1; y = 2c2 - 1; r2 = x x + y y; } while (r2 > 1 || r2 == 0);
//     mult = sqrt(-2 log(r2) / r2); returns y mult sigma + mean and saves x mult for the next call of the same object.
//   uniform_real_distribution<float>(a, b): c (b - a) + a, one engine call.
//
// The stream is therefore a sequence of ATTEMPTS, attempt t using engine outputs 2t + 1 and 2t + 2, and which attempts are
// accepted depends on nothing but the engine state at the start. A distribution constructed afresh per value
// (DiagonalNoiseGenerator) takes y mult of every accepted attempt; one shared distribution (update_noise_func) takes y mult,
// then x mult. All of it is float arithmetic with contraction off; the logarithm alone comes from a policy: the device takes
// (float)log((double)r2) (the project's rule for transcendentals), the CPU emulation can also take std::log(float) to prove the
// restatement against the standard library itself.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RNG_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define RNG_HD
#endif

namespace mcl3dl
{
namespace rng
{
constexpr uint32_t MINSTD_M = 2147483647u;  // 2^31 - 1
constexpr uint32_t MINSTD_A = 16807u;
constexpr int ATTEMPTS_PER_LANE = 8;        // E of rng_stream.h: consecutive attempts one lane walks behind its jump
constexpr int GROUP_THREADS = 256;

// a b mod (2^31 - 1) for a, b < 2^31 by the Mersenne identity 2^31 = 1: two folds (p < 2^62), one conditional subtract
RNG_HD inline uint32_t minstd_mulmod(uint32_t a, uint32_t b)
{
  const uint64_t p = static_cast<uint64_t>(a) * b;
  uint64_t r = (p & MINSTD_M) + (p >> 31);
  r = (r & MINSTD_M) + (r >> 31);
  return static_cast<uint32_t>(r >= MINSTD_M ? r - MINSTD_M : r);
}

// one engine call: 16807 x < 2^46, so one fold and one conditional subtract
RNG_HD inline uint32_t minstd_next(uint32_t x)
{
  const uint64_t p = static_cast<uint64_t>(x) * MINSTD_A;
  const uint32_t r = static_cast<uint32_t>(p & MINSTD_M) + static_cast<uint32_t>(p >> 31);
  return r >= MINSTD_M ? r - MINSTD_M : r;
}

// engine(seed)'s state
RNG_HD inline uint32_t minstd_seed(uint32_t seed)
{
  const uint32_t x = seed % MINSTD_M;
  return x == 0 ? 1u : x;
}

// table[i] = 16807^(2^i) mod (2^31 - 1), i < 64 (built once on the host)
inline void minstd_build_table(uint32_t* table64)
{
  uint32_t a = MINSTD_A;
  for (int i = 0; i < 64; ++i)
  {
    table64[i] = a;
    a = minstd_mulmod(a, a);
  }
}

// x 16807^k mod (2^31 - 1): the state k engine calls on. Square-and-multiply over the table; no division.
RNG_HD inline uint32_t minstd_jump(uint32_t x, uint64_t k, const uint32_t* table64)
{
  for (int i = 0; k != 0; ++i, k >>= 1)
    if (k & 1u)
      x = minstd_mulmod(x, table64[i]);
  return x;
}

RNG_HD inline float canonical(uint32_t v)
{
  const float c = static_cast<float>(v - 1u) / 2147483648.0f;
  return c >= 1.0f ? 0x1.fffffep-1f : c;  // nextafterf(1, 0)
}

struct Attempt
{
  float x, y, r2;
  bool accepted;
};

// v1, v2: two consecutive engine outputs
RNG_HD inline Attempt polar_attempt(uint32_t v1, uint32_t v2)
{
  Attempt a;
  a.x = 2.0f * canonical(v1) - 1.0f;
  a.y = 2.0f * canonical(v2) - 1.0f;
  a.r2 = a.x * a.x + a.y * a.y;
  a.accepted = !(a.r2 > 1.0f || a.r2 == 0.0f);
  return a;
}

struct LogDouble  // the device's: log in double, rounded to float once
{
  RNG_HD float operator()(float r2) const { return static_cast<float>(log(static_cast<double>(r2))); }
};
#if !defined(__HIPCC__)
struct LogHostFloat  // std::log(float), what libstdc++'s normal_distribution<float> calls
{
  float operator()(float r2) const { return std::log(r2); }
};
#endif

template <typename Log>
RNG_HD inline float polar_mult(float r2, Log lg)
{
  return sqrtf(-2.0f * lg(r2) / r2);
}

// uniform_real_distribution<float>(a, b)(engine): one engine call
inline float uniform_draw(uint32_t* state, float a, float b)
{
  *state = minstd_next(*state);
  return canonical(*state) * (b - a) + a;
}

// How many attempts one round evaluates to find k more accepted ones. An attempt is accepted with p = pi / 4 (up to 2^-24 effects),
// so k accepted ones take k / p attempts on average, and the number accepted among n attempts has the standard deviation
// sqrt(n p (1 - p)). The budget is ceil(k 4 / pi) plus THREE standard deviations of the accepted count, expressed in attempts:
// ceil(3 sqrt(k (1 - p)) / p). A round falls short about once in 750 calls at large k, and once in 450 at k = 1 or 2 (budgets 4
// and 6) — the second round is part of the ordinary path, not an error path.
inline uint64_t attempt_budget(uint64_t k_remaining)
{
  const double p = 0.78539816339744830962;
  const double k = static_cast<double>(k_remaining);
  return static_cast<uint64_t>(std::ceil(k / p)) + static_cast<uint64_t>(std::ceil(3.0 * std::sqrt(k * (1.0 - p)) / p));
}

// rng_stream.h's attempt policy of this stream: two engine calls per attempt
struct PolarPolicy
{
  static constexpr int CALLS = 2;
  struct Kept
  {
    float x, y, r2;
    uint32_t state;  // the engine state behind the attempt's second draw
  };
  RNG_HD bool judge(const uint32_t* v, Kept* k) const
  {
    const Attempt a = polar_attempt(v[0], v[1]);
    k->x = a.x;
    k->y = a.y;
    k->r2 = a.r2;
    k->state = v[1];
    return a.accepted;
  }
  RNG_HD static uint32_t state(const Kept& k) { return k.state; }
  uint64_t budget(uint64_t k_remaining) const { return attempt_budget(k_remaining); }
};

// Quat::setRPY (quat.h:202-215): cos / sin of the float half angles in double, rounded to float (the motion kernels' rule);
// every product of :211-214 kept, in float, left to right
RNG_HD inline void quat_set_rpy(float roll, float pitch, float yaw, float* xyzw)
{
  const float t2 = static_cast<float>(cos(static_cast<double>(roll / 2)));
  const float t3 = static_cast<float>(sin(static_cast<double>(roll / 2)));
  const float t4 = static_cast<float>(cos(static_cast<double>(pitch / 2)));
  const float t5 = static_cast<float>(sin(static_cast<double>(pitch / 2)));
  const float t0 = static_cast<float>(cos(static_cast<double>(yaw / 2)));
  const float t1 = static_cast<float>(sin(static_cast<double>(yaw / 2)));
  xyzw[0] = t0 * t3 * t4 - t1 * t2 * t5;
  xyzw[1] = t0 * t2 * t5 + t1 * t3 * t4;
  xyzw[2] = t1 * t2 * t4 - t0 * t3 * t5;
  xyzw[3] = t0 * t2 * t4 + t1 * t3 * t5;
}

// State6DOF::generateNoise (state_6dof.h:226-248) behind the generator's six values: positions to 0-2 and 7-9, rpy - mean to
// 10-12, rot = Quat(rpy) to 3-6 {x, y, z, w}
RNG_HD inline void noise6_to_state13(const float* values6, const float* mean6, float* out13)
{
  for (int i = 0; i < 3; ++i)
  {
    out13[i] = values6[i];
    out13[i + 7] = values6[i];
    out13[i + 10] = values6[i + 3] - mean6[i + 3];
  }
  quat_set_rpy(values6[3], values6[4], values6[5], out13 + 3);
}
}  // namespace rng
}  // namespace mcl3dl
