// rng_polar_emul.cpp — the device's decomposition of the reference's random stream, replayed on the CPU from the headers the
// kernels compile (mcl_3dl_amd/csrc/rng_stream.h: the lane walk and the placement loop; rng_polar.h: the polar policy): runs of E
// attempts per lane behind one jump, and around them rng_emul_common.h's stand-in for 64-lane ballots, 256-thread work-groups,
// one count per work-group, the exclusive scan, ranks from group offset + wavefront offset + mbcnt, and the host's rounds with
// attempt_budget. Its yardstick is the standard library itself: std::default_random_engine with
// std::normal_distribution<float> / std::uniform_real_distribution<float> (libstdc++).
//
//   rng_polar_emul selftest                                        every case of tests/test_rng_polar_cpu.py, "all equal" at the end
//   rng_polar_emul stream <std|host|double> <fresh|shared> <state> <n> <out.bin>
//        n values of normal_distribution<float>(0, 1) from engine state <state>: by the standard library (std), or by the
//        replayed kernels with std::log(float) (host) or (float)log((double)) (double, the device's policy); prints
//        "state=<engine state behind> rounds=<r> attempts=<a>" and writes the floats
// g++ -O2 -ffp-contract=off.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "rng_emul_common.h"

namespace
{
using Result = Rounds;

// host_rng.h: rng_draw, with rng_kernels.h's PolarSink
template <typename Log>
Result draw(uint32_t state_in, uint64_t k_total, bool pairs, uint64_t k_begin, uint64_t k_end, std::vector<float>& values)
{
  k_end = std::min(k_end, k_total);
  k_begin = std::min(k_begin, k_end);
  values.assign((pairs ? 2 : 1) * (k_end - k_begin), 0.0f);
  return replay_rounds(PolarPolicy{}, state_in, k_total,
                       [&](uint64_t rank, uint64_t, const PolarPolicy::Kept& k)
                       {
                         if (rank < k_begin || rank >= k_end)
                           return;
                         const float mult = polar_mult(k.r2, Log());
                         if (pairs)
                         {
                           values[2 * (rank - k_begin)] = k.y * mult;
                           values[2 * (rank - k_begin) + 1] = k.x * mult;
                         }
                         else
                           values[rank - k_begin] = k.y * mult;
                       });
}

// n values of normal_distribution<float>(0, 1): fresh = one distribution per value, shared = one for all
Result std_stream(uint32_t state, bool shared, size_t n, std::vector<float>& values)
{
  std::default_random_engine eng;
  set_state(eng, state);
  values.resize(n);
  std::normal_distribution<float> one(0.0f, 1.0f);
  for (size_t i = 0; i < n; ++i)
  {
    if (shared)
      values[i] = one(eng);
    else
    {
      std::normal_distribution<float> nd(0.0f, 1.0f);
      values[i] = nd(eng);
    }
  }
  return Result{ get_state(eng), 0, 0 };
}

template <typename Log>
Result emul_stream(uint32_t state, bool shared, size_t n, std::vector<float>& values)
{
  // shared: accepted attempt k yields values 2k and 2k + 1; an odd n still consumes the whole last attempt
  const uint64_t k = shared ? (n + 1) / 2 : n;
  const Result r = draw<Log>(state, k, shared, 0, k, values);
  values.resize(n);
  for (float& v : values)
    v = v * 1.0f + 0.0f;  // ret * stddev + mean
  return r;
}

bool same_bits(const std::vector<float>& a, const std::vector<float>& b)
{
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

int g_fail = 0;
void report(const char* what, uint32_t state, uint64_t k, bool ok, const Result& r)
{
  printf("case %s state=%u k=%llu rounds=%d attempts=%llu %s\n", what, state, static_cast<unsigned long long>(k), r.rounds,
         static_cast<unsigned long long>(r.attempts), ok ? "equal" : "DIFFERENT");
  if (!ok)
    ++g_fail;
}

// rng_kernels.h: rng_noise_state_kernel for row i
void noise_row(const std::vector<float>& values, const float* mean, const float* sigma, int dims, size_t i, float* row13)
{
  const float* z = values.data() + static_cast<size_t>(dims) * i;
  float v[6];
  int d = 0;
  for (int k = 0; k < 6; ++k)
    v[k] = sigma[k] == 0.0f ? mean[k] : z[d++] * sigma[k] + mean[k];
  noise6_to_state13(v, mean, row13);
}

int selftest()
{
  const uint32_t inv = modpow(MINSTD_A, MINSTD_M - 2);  // 16807^-1: the state whose next output is 1 (canonical = 0)
  const uint32_t before_max = minstd_mulmod(MINSTD_M - 1, inv);  // ... whose next output is 2^31 - 2 (the nextafter branch)
  if (minstd_next(inv) != 1u || minstd_next(before_max) != MINSTD_M - 1u || canonical(1u) != 0.0f ||
      canonical(MINSTD_M - 1u) != 0x1.fffffep-1f)
  {
    printf("edge states wrong\n");
    return 1;
  }
  const uint32_t starts[] = { minstd_seed(12345u), minstd_seed(0u), inv, before_max, minstd_seed(777u) };
  const uint64_t per_group = static_cast<uint64_t>(GROUP_THREADS) * E;
  const uint64_t ks[] = { 1, 2, 63, 64, 65, 255, 256, 257, 2 * per_group - 1, 2 * per_group + 1, 100000 };
  std::vector<float> want, got;
  for (uint32_t s : starts)
  {
    // jump-ahead against the engine's own discard
    // (beyond what discard() walks in reasonable time: the group law, and the generator's period 2^31 - 2)
    const uint64_t big = 0x123456789abcdefull;
    if (minstd_jump(minstd_jump(s, big, g_table), 987654321ull, g_table) != minstd_jump(s, big + 987654321ull, g_table) ||
        minstd_jump(s, MINSTD_M - 1u, g_table) != s || minstd_jump(s, big, g_table) != minstd_jump(s, big % (MINSTD_M - 1u), g_table))
    {
      printf("jump %u big DIFFERENT\n", s);
      ++g_fail;
    }
    for (uint64_t k : { 0ull, 1ull, 2ull, 12345ull, 20000000ull })
    {
      std::default_random_engine eng;
      set_state(eng, s);
      eng.discard(k);
      if (get_state(eng) != minstd_jump(s, k, g_table))
      {
        printf("jump %u %llu DIFFERENT\n", s, static_cast<unsigned long long>(k));
        ++g_fail;
      }
    }
    // the uniform
    {
      std::default_random_engine eng;
      set_state(eng, s);
      uint32_t st = s;
      bool ok = true;
      for (int i = 0; i < 1000; ++i)
      {
        const float a = std::uniform_real_distribution<float>(0.0f, 0.37f)(eng);
        const float b = uniform_draw(&st, 0.0f, 0.37f);
        ok = ok && memcmp(&a, &b, 4) == 0 && st == get_state(eng);
      }
      report("uniform", s, 1000, ok, Result{ st, 0, 0 });
    }
    for (uint64_t k : ks)
    {
      // fresh distribution per value, with a mean and a sigma
      {
        std::default_random_engine eng;
        set_state(eng, s);
        want.resize(k);
        for (uint64_t i = 0; i < k; ++i)
        {
          std::normal_distribution<float> nd(0.25f, 0.1f);
          want[i] = nd(eng);
        }
        const Result r = draw<LogHostFloat>(s, k, false, 0, k, got);
        for (float& v : got)
          v = v * 0.1f + 0.25f;
        report("fresh", s, k, same_bits(want, got) && r.state == get_state(eng), r);
      }
      // one shared distribution, 2k values
      {
        const Result w = std_stream(s, true, 2 * k, want);
        const Result r = emul_stream<LogHostFloat>(s, true, 2 * k, got);
        report("shared", s, k, same_bits(want, got) && r.state == w.state, r);
      }
    }
    // a window of the stream, as a rank of a device group emits it
    {
      const uint64_t k = 6000, lo = 1999, hi = 4001;
      const Result w = std_stream(s, false, k, want);
      const Result r = draw<LogHostFloat>(s, k, false, lo, hi, got);
      for (float& v : got)
        v = v * 1.0f + 0.0f;
      const bool ok = got.size() == hi - lo && memcmp(got.data(), want.data() + lo, (hi - lo) * 4) == 0 && r.state == w.state;
      report("window", s, k, ok, r);
    }
  }
  // sigma patterns with zeros in every position: DiagonalNoiseGenerator + State6DOF::generateNoise row by row
  {
    const float mean[6] = { 1.5f, -2.0f, 0.25f, 0.1f, -0.2f, 0.7f };
    const float sig[6] = { 0.1f, 0.2f, 0.05f, 0.01f, 0.02f, 0.05f };
    for (int pat = 0; pat < 64; ++pat)
    {
      float sigma[6];
      int dims = 0;
      for (int k = 0; k < 6; ++k)
      {
        sigma[k] = ((pat >> k) & 1) ? sig[k] : 0.0f;
        dims += sigma[k] != 0.0f;
      }
      const size_t n = 257;
      const uint32_t s = minstd_seed(1000u + pat);
      std::default_random_engine eng;
      set_state(eng, s);
      std::vector<float> rows_want(13 * n), rows_got(13 * n);
      for (size_t i = 0; i < n; ++i)
      {
        float v[6];
        for (int k = 0; k < 6; ++k)
        {
          if (sigma[k] == 0)
          {
            v[k] = mean[k];
            continue;
          }
          std::normal_distribution<float> nd(mean[k], sigma[k]);
          v[k] = nd(eng);
        }
        noise6_to_state13(v, mean, &rows_want[13 * i]);
      }
      const Result r = draw<LogHostFloat>(s, n * dims, false, 0, n * dims, got);
      for (size_t i = 0; i < n; ++i)
        noise_row(got, mean, sigma, dims, i, &rows_got[13 * i]);
      char name[32];
      snprintf(name, sizeof(name), "sigma%02d", pat);
      report(name, s, n * dims, same_bits(rows_want, rows_got) && r.state == get_state(eng), r);
    }
  }
  // small K over many seeds: the budget rule lets a round fall short now and then (the second round is an ordinary path)
  for (uint64_t k : { 1ull, 2ull, 7ull })
    for (uint32_t seed = 1; seed <= 1500; ++seed)
    {
      const uint32_t s = minstd_seed(seed);
      const Result w = std_stream(s, false, k, want);
      const Result r = emul_stream<LogHostFloat>(s, false, k, got);
      const bool ok = same_bits(want, got) && r.state == w.state;
      if (!ok || r.rounds > 1)
        report("small", s, k, ok, r);
    }
  printf(g_fail ? "%d cases DIFFERENT\n" : "all equal\n", g_fail);
  return g_fail ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv)
{
  minstd_build_table(g_table);
  if (argc >= 2 && !strcmp(argv[1], "selftest"))
    return selftest();
  if (argc == 7 && !strcmp(argv[1], "stream"))
  {
    const std::string impl = argv[2];
    const bool shared = !strcmp(argv[3], "shared");
    const uint32_t state = static_cast<uint32_t>(strtoul(argv[4], nullptr, 10));
    const size_t n = strtoull(argv[5], nullptr, 10);
    if (state < 1u || state > MINSTD_M - 1u)
      return 2;
    std::vector<float> values;
    Result r;
    if (impl == "std")
      r = std_stream(state, shared, n, values);
    else if (impl == "host")
      r = emul_stream<LogHostFloat>(state, shared, n, values);
    else if (impl == "double")
      r = emul_stream<LogDouble>(state, shared, n, values);
    else
      return 2;
    FILE* f = fopen(argv[6], "wb");
    if (!f || fwrite(values.data(), sizeof(float), values.size(), f) != values.size())
      return 3;
    fclose(f);
    printf("state=%u rounds=%d attempts=%llu\n", r.state, r.rounds, static_cast<unsigned long long>(r.attempts));
    return 0;
  }
  fprintf(stderr, "usage: %s selftest | stream <std|host|double> <fresh|shared> <state> <n> <out.bin>\n", argv[0]);
  return 2;
}
