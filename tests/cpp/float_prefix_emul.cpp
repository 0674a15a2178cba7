// float_prefix_emul.cpp — mcl_3dl_amd/csrc/float_prefix.h's wavefront chain replayed on the CPU, the 64 lanes one after the
// other, against the plain loop `cum[i] = acc += w[i]` it must reproduce in EVERY prefix, bit for bit. The binade constants and
// the per-term classification are the header's own (fprefix_binade / fprefix_classify); what is replayed is what only the
// device has: the lanes' eight terms, the wave scan, the ballot, the broadcasts, and the lane-0 rule.
//
//   float_prefix_emul selftest                      every input family; prints the step counts and "all equal"
//   float_prefix_emul record STATE N_OUT MODE BITS...  the record resample_prefix_kernel leaves for the weights given as bit patterns
//
// g++ -O2 -ffp-contract=off
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../mcl_3dl_amd/csrc/resample_prefix_kernels.h"

namespace
{
using namespace mcl3dl;

struct Stats
{
  long long steps = 0;        // passes and serial blocks behind the head
  long long full = 0;         // passes that retired all 512 terms
  long long serial64 = 0;     // 64 serial terms: lane 0 in trouble, or a sum outside the normal range
  long long min_retired = -1; // fewest terms a step retired, the last step aside
};

// w == null: every term is c
std::vector<float> chain_emul(const float* w, float c, long long n, bool* tie, Stats* st)
{
  std::vector<float> cum(static_cast<size_t>(n), -12345.0f);
  const auto term = [&](long long i) { return i < n ? (w ? w[i] : c) : 0.0f; };
  float s = 0.0f;
  bool tied = false;
  const auto serial = [&](long long at, int count)
  {
    for (int k = 0; k < count && at + k < n; ++k)
    {
      const float prev = s;
      s = s + term(at + k);
      tied |= (at + k > 0) & !(prev < s);
      cum[at + k] = s;
    }
  };
  const auto retired = [&](long long from, long long to)
  {
    st->steps++;
    if (to < n && (st->min_retired < 0 || to - from < st->min_retired))
      st->min_retired = to - from;
  };
  long long q = 0;
  for (; q < FPREFIX_HEAD && q < n; q += 64)
    serial(q, 64);
  while (q < n)
  {
    FPrefixBinade b;
    if (!fprefix_binade(s, &b))
    {
      serial(q, 64);
      retired(q, q + 64);
      st->serial64++;
      q += 64;
      continue;
    }
    float a[64][FPREFIX_LANE_TERMS], r[64][FPREFIX_LANE_TERMS], p[64];
    bool ok[64];
    for (int l = 0; l < 64; ++l)
    {
      ok[l] = true;
      float run = 0.0f;
      for (int k = 0; k < FPREFIX_LANE_TERMS; ++k)
      {
        ok[l] &= fprefix_classify(term(q + 8LL * l + k), b, &r[l][k]);
        run = k == 0 ? r[l][k] : run + r[l][k];
        a[l][k] = run;
      }
      p[l] = a[l][FPREFIX_LANE_TERMS - 1];
    }
    // wave_scan_add (float_chain.h): inside the rows of 16 by shifts of 1, 2, 4, 8 (a lane without a source adds 0), then
    // row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3
    for (int d = 1; d < 16; d <<= 1)
    {
      float o[64];
      for (int l = 0; l < 64; ++l)
        o[l] = (l & 15) >= d ? p[l - d] : 0.0f;
      for (int l = 0; l < 64; ++l)
        p[l] = p[l] + o[l];
    }
    {
      float o[64];
      for (int l = 0; l < 64; ++l)
        o[l] = ((l >> 4) & 1) ? p[(l & ~15) - 1] : 0.0f;
      for (int l = 0; l < 64; ++l)
        p[l] = p[l] + o[l];
      for (int l = 0; l < 64; ++l)
        o[l] = l >= 32 ? p[31] : 0.0f;
      for (int l = 0; l < 64; ++l)
        p[l] = p[l] + o[l];
    }
    int L = 64;
    for (int l = 63; l >= 0; --l)
      if (!(ok[l] & (s + p[l] < b.top)))
        L = l;
    if (L == 0)
    {
      serial(q, 64);
      retired(q, q + 64);
      st->serial64++;
      q += 64;
      continue;
    }
    for (int l = 0; l < L; ++l)
    {
      const float base = s + (p[l] - a[l][FPREFIX_LANE_TERMS - 1]);
      for (int k = 0; k < FPREFIX_LANE_TERMS; ++k)
      {
        const long long i = q + 8LL * l + k;
        if (i < n)
        {
          cum[i] = base + a[l][k];
          tied |= r[l][k] == 0.0f;
        }
      }
    }
    if (L == 64)
    {
      s = s + p[63];
      retired(q, q + FPREFIX_PASS);
      st->full++;
      q += FPREFIX_PASS;
      continue;
    }
    s = s + p[L - 1];
    const long long at = q + 8LL * L;
    serial(at, FPREFIX_LANE_TERMS);
    retired(q, at + FPREFIX_LANE_TERMS);
    q = at + FPREFIX_LANE_TERMS;
  }
  *tie = tied;
  return cum;
}

std::vector<float> plain(const float* w, float c, long long n, bool* tie)
{
  std::vector<float> cum(static_cast<size_t>(n));
  float acc = 0.0f;
  *tie = false;
  for (long long i = 0; i < n; ++i)
  {
    const float prev = acc;
    acc += w ? w[i] : c;
    *tie = *tie || (i > 0 && !(prev < acc));
    cum[i] = acc;
  }
  return cum;
}

int g_failures = 0;

Stats check(const std::string& name, const float* w, float c, long long n, bool print)
{
  Stats st;
  bool tie_e = false, tie_p = false;
  const std::vector<float> got = chain_emul(w, c, n, &tie_e, &st);
  const std::vector<float> want = plain(w, c, n, &tie_p);
  const bool same = n == 0 || memcmp(got.data(), want.data(), sizeof(float) * static_cast<size_t>(n)) == 0;
  if (!same || tie_e != tie_p)
  {
    ++g_failures;
    long long first = -1;
    for (long long i = 0; i < n && first < 0; ++i)
      if (memcmp(&got[i], &want[i], sizeof(float)) != 0)
        first = i;
    printf("MISMATCH %s n=%lld first=%lld tie %d/%d\n", name.c_str(), n, first, tie_e, tie_p);
  }
  if (print)
    printf("steps %-34s n=%-7lld steps=%-5lld full=%-4lld serial64=%-5lld min_retired=%lld ties=%d\n", name.c_str(), n, st.steps,
           st.full, st.serial64, st.min_retired, tie_p);
  return st;
}

std::vector<float> weights(long long n, float spread, uint32_t seed)
{
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> u(1.0, spread);
  std::vector<double> d(static_cast<size_t>(n));
  double sum = 0;
  for (double& x : d)
    sum += (x = u(g));
  std::vector<float> w(static_cast<size_t>(n));
  for (long long i = 0; i < n; ++i)
    w[i] = static_cast<float>(d[i] / sum);
  return w;
}

// 1 / n with the low `bits` mantissa bits set to 1 0...0
float tie_constant(long long n, int bits)
{
  uint32_t u = fprefix_bits(1.0f / static_cast<float>(n));
  u = (u & ~((1u << bits) - 1u)) | (1u << (bits - 1));
  return fprefix_from_bits(u);
}

int selftest()
{
  const long long sizes[] = { 1, 7, 255, 256, 257, 511, 512, 513, 769, 4097, 70001 };
  for (long long n : sizes)
    for (float spread : { 3.0f, 30.0f })
    {
      const std::vector<float> w = weights(n, spread, static_cast<uint32_t>(n) * 31u + static_cast<uint32_t>(spread));
      check("weights x" + std::to_string(static_cast<int>(spread)), w.data(), 0.f, n, n >= 4097);
    }
  for (long long n : { 4096LL, 262144LL, 600LL, 1000000LL })
    for (float spread : { 3.0f, 30.0f })
    {
      const std::vector<float> w = weights(n, spread, static_cast<uint32_t>(n) + 7u);
      check("weights x" + std::to_string(static_cast<int>(spread)), w.data(), 0.f, n, true);
    }
  for (long long n : sizes)
    check("constant 1/n", nullptr, 1.0f / static_cast<float>(n), n, n >= 4097);
  check("constant 1/n", nullptr, 1.0f / 262144.0f, 262144, true);
  check("constant 1/196608 (resize 3/4)", nullptr, 1.0f / 196608.0f, 196608, true);
  // a constant that is a rounding tie at every step of one binade behind the head
  check("tie constant, 9 bits", nullptr, tie_constant(3000, 9), 3000, true);
  {
    const Stats st = check("tie constant, 16 bits", nullptr, tie_constant(200000, 16), 200000, true);
    // the lane-0 rule: L = 0 retires 64 terms, L >= 1 retires 8 L + 8 >= 16
    if (st.min_retired < 16)
    {
      ++g_failures;
      printf("LANE-0 RULE: a step behind the head retired %lld terms\n", st.min_retired);
    }
  }
  // the same terms as an array (the other load path)
  {
    const std::vector<float> w(3000, tie_constant(3000, 9));
    check("tie constant, 9 bits, as array", w.data(), 0.f, 3000, false);
  }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (long long n : { 1LL, 7LL, 257LL, 513LL, 769LL, 4097LL })
  {
    std::vector<float> z(static_cast<size_t>(n), 0.0f), mz(static_cast<size_t>(n), -0.0f);
    check("zeros", z.data(), 0.f, n, false);
    check("-0", mz.data(), 0.f, n, false);
    check("constant -0", nullptr, -0.0f, n, false);
    check("constant 0", nullptr, 0.0f, n, false);
    std::vector<float> w = weights(n, 3.0f, 5u);
    for (long long i = 0; i < n; i += 3)
      w[i] = (i % 2) ? -0.0f : 0.0f;  // dead particles
    check("weights with zeros and -0", w.data(), 0.f, n, false);
    // a term larger than the running sum, behind the head and at the ends
    for (long long pos : { 0LL, 300LL, n - 1 })
      if (pos < n)
      {
        std::vector<float> big = weights(n, 3.0f, 11u);
        big[pos] = 1000.0f;
        check("large term", big.data(), 0.f, n, false);
        for (float special : { nan, inf, -inf, -0.25f, 1e-41f, 3e38f })
        {
          std::vector<float> x = weights(n, 30.0f, 13u);
          x[pos] = special;
          check("special term", x.data(), 0.f, n, false);
        }
      }
    // negative terms throughout, denormals throughout, a sum that overflows
    std::vector<float> neg = weights(n, 3.0f, 17u), den(static_cast<size_t>(n)), over(static_cast<size_t>(n), 1e37f);
    for (long long i = 0; i < n; ++i)
    {
      if (i % 5 == 2)
        neg[i] = -neg[i];
      den[i] = fprefix_from_bits(1u + static_cast<uint32_t>(i % 977));
    }
    check("negative terms", neg.data(), 0.f, n, false);
    check("denormals", den.data(), 0.f, n, false);
    check("overflow", over.data(), 0.f, n, false);
    check("constant overflow", nullptr, 3e36f, n, false);
    check("constant NaN", nullptr, nan, n, false);
  }
  // wild magnitudes: binade crossings everywhere
  {
    std::mt19937 g(99);
    std::uniform_real_distribution<float> e(-30.f, 10.f);
    std::vector<float> w(20000);
    for (float& x : w)
      x = std::exp2(e(g));
    check("wild magnitudes", w.data(), 0.f, 20000, true);
  }
  if (g_failures)
  {
    printf("%d FAILED\n", g_failures);
    return 1;
  }
  printf("all equal\n");
  return 0;
}

int record(int argc, char** argv)
{
  if (argc < 6)
    return 2;
  const uint32_t state = static_cast<uint32_t>(strtoul(argv[2], nullptr, 10));
  const unsigned long long n_out = strtoull(argv[3], nullptr, 10);
  const int mode = atoi(argv[4]);
  std::vector<float> w;
  for (int i = 5; i < argc; ++i)
    w.push_back(fprefix_from_bits(static_cast<uint32_t>(strtoul(argv[i], nullptr, 10))));
  bool tie = false;
  Stats st;
  const std::vector<float> keys = chain_emul(w.data(), 0.f, static_cast<long long>(w.size()), &tie, &st);
  ResampleRecord rec;
  resample_record_fill(keys.back(), n_out, mode, state, tie, &rec);
  printf("%u %u %u %u %u\n", fprefix_bits(rec.pstep), fprefix_bits(rec.initial_p), rec.state, rec.ties, fprefix_bits(rec.total));
  return 0;
}
}  // namespace

int main(int argc, char** argv)
{
  const std::string mode = argc > 1 ? argv[1] : "selftest";
  if (mode == "selftest")
    return selftest();
  if (mode == "record")
    return record(argc, argv);
  fprintf(stderr, "usage: float_prefix_emul selftest | record STATE N_OUT MODE BITS...\n");
  return 2;
}
