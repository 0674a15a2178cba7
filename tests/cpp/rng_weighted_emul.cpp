// rng_weighted_emul.cpp — the normal-weighted sampler's draw as the device runs it, replayed on the CPU from the headers the
// kernels compile (mcl_3dl_amd/csrc/rng_weighted.h: the draw, lower_bound, the per-thread steps of both kernel forms;
// double_chain.h: the binade constants and the term classification), against the standard library itself:
// std::default_random_engine, std::uniform_real_distribution<double>, std::lower_bound and std::unordered_set<size_t> in the loop
// of PointCloudSamplerWithNormal::sample, and the plain `cum[i] = w[i] + cum[i - 1]` loop.
//
//   rng_weighted_emul selftest                            every case of tests/test_rng_weighted_cpu.py, "all equal" at the end
//   rng_weighted_emul weights <kind> <n> <seed> <out.bin> the test inputs: ones | rand | ties | big | neg | special  (float64)
//   rng_weighted_emul cumsum <w.bin> <out.bin>            the plain loop
//   rng_weighted_emul chain <w.bin> <out.bin>             the wavefront's passes, lane by lane
//   rng_weighted_emul draw <std|single|rounds> <state> <cum.bin> <num> <out.bin>
//        `num` distinct ids of the cloud whose cumulative weights are in cum.bin, in the order of the sampled cloud (uint32);
//        prints "state=<engine state behind> draws=<attempts made> rounds=<r>"
//   rng_weighted_emul drawtime <state> <cum.bin> <num> <reps>
//        the standard library's loop alone, timed in this process: prints "host_ms=<minimum over reps> draws=<attempts made>"
// g++ -O2 (-ffp-contract=off is g++'s default on x86-64 without -march flags; the arithmetic here has no fused form anyway).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../mcl_3dl_amd/csrc/double_chain.h"
#include "../../mcl_3dl_amd/csrc/rng_weighted.h"
#include "rng_emul_common.h"  // g_table, set_state, get_state

using namespace mcl3dl;
using namespace mcl3dl::rng;

namespace
{
bool same_bits(const std::vector<double>& a, const std::vector<double>& b)
{
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

// ---- the cumulative weights ------------------------------------------------------------------------------------------------
std::vector<double> plain_cumsum(const std::vector<double>& w)
{
  std::vector<double> cum(w.size());
  double run = 0.0;  // (0.0 + w[0] is w[0] for every double but -0.0, as in the sampler's own first step)
  for (size_t i = 0; i < w.size(); ++i)
    cum[i] = run = w[i] + run;
  return cum;
}

struct ChainStats
{
  long long passes = 0, full = 0, serial_blocks = 0;
};

// double_chain.h: dchain_prefix_wave, the 64 lanes one after the other
std::vector<double> chain_emul(const std::vector<double>& w, ChainStats* st)
{
  const long long n = static_cast<long long>(w.size());
  std::vector<double> cum(w.size(), -12345.0);
  double s = 0.0;
  const auto serial = [&](long long at, int count)
  {
    for (int k = 0; k < count && at + k < n; ++k)
    {
      s = s + w[at + k];
      cum[at + k] = s;
    }
  };
  long long q = 0;
  for (; q < DCHAIN_HEAD && q < n; q += 64)
    serial(q, 64);
  while (q < n)
  {
    DChainBinade b;
    if (!dchain_binade(s, &b))
    {
      serial(q, 64);
      q += 64;
      st->serial_blocks++;
      continue;
    }
    st->passes++;
    double a[64][DCHAIN_LANE_TERMS], p[64];
    bool ok[64];
    for (int l = 0; l < 64; ++l)
    {
      ok[l] = true;
      double run = 0.0;
      for (int k = 0; k < DCHAIN_LANE_TERMS; ++k)
      {
        const long long i = q + static_cast<long long>(DCHAIN_LANE_TERMS) * l + k;
        const double t = i < n ? w[i] : 0.0;
        double r;
        ok[l] &= dchain_classify(t, b, &r);
        run = k == 0 ? r : run + r;
        a[l][k] = run;
      }
      p[l] = a[l][DCHAIN_LANE_TERMS - 1];
    }
    for (int d = 1; d < 64; d <<= 1)  // dchain_wave_scan: every lane reads its source before anyone writes
    {
      double o[64];
      for (int l = 0; l < 64; ++l)
        o[l] = l >= d ? p[l - d] : 0.0;
      for (int l = 0; l < 64; ++l)
        p[l] = l >= d ? p[l] + o[l] : p[l];
    }
    int L = 64;
    for (int l = 63; l >= 0; --l)
      if (!(ok[l] & (s + p[l] < b.top)))
        L = l;
    for (int l = 0; l < L; ++l)
    {
      const double base = s + (p[l] - a[l][DCHAIN_LANE_TERMS - 1]);
      for (int k = 0; k < DCHAIN_LANE_TERMS; ++k)
      {
        const long long i = q + static_cast<long long>(DCHAIN_LANE_TERMS) * l + k;
        if (i < n)
          cum[i] = base + a[l][k];
      }
    }
    if (L == 64)
    {
      s = s + p[63];
      q += DCHAIN_PASS;
      st->full++;
      continue;
    }
    if (L > 0)
      s = s + p[L - 1];
    const long long at = q + static_cast<long long>(DCHAIN_LANE_TERMS) * L;
    serial(at, DCHAIN_LANE_TERMS);
    q = at + DCHAIN_LANE_TERMS;
  }
  return cum;
}

std::vector<double> make_weights(const std::string& kind, size_t n, uint32_t seed)
{
  std::mt19937_64 g(seed * 7919u + 17u);
  std::uniform_real_distribution<double> u15(1.0, 5.0), u01(0.0, 1.0);
  std::vector<double> w(n);
  double s = 0.0;
  for (size_t i = 0; i < n; ++i)
  {
    double t = u15(g);
    if (kind == "ones")
      t = 1.0;
    else if (kind == "ties" && s >= 4.0 && (g() & 3u) == 0u)
    {
      // a rounding tie against the running sum: an odd multiple of half its ulp
      const double ulp = std::nextafter(s, std::numeric_limits<double>::infinity()) - s;
      t = 1.0 + ulp * (static_cast<double>(g() % 4096u) + 0.5);  // (exact: half an ulp of a sum >= 4 is a multiple of 2^-51)
    }
    else if (kind == "big" && (g() % 53u) == 0u && s < 1e290)
      t = s * (0.5 + 2.0 * u01(g));  // at least half the sum
    else if (kind == "neg" && (g() % 5u) == 0u)
      t = -u15(g) * ((g() & 1u) ? 1.0 : 1e-3);
    else if (kind == "special")
    {
      if (i == 2 * n / 3)
        t = std::numeric_limits<double>::infinity();
      else if (i == 5 * n / 6 && n >= 6)
        t = -std::numeric_limits<double>::infinity();  // inf + -inf: NaN from here on
      else if (i == n / 2 && n >= 64)
        t = -0.0;
      else if (i == n / 3 && n >= 64)
        t = 4.9e-324;
      else if (n < 6 && i == 0)
        t = std::numeric_limits<double>::quiet_NaN();
    }
    w[i] = t;
    s = s + t;
  }
  return w;
}

// ---- the draws -------------------------------------------------------------------------------------------------------------
struct Result
{
  uint32_t state;
  uint64_t draws;
  int rounds;
};

// the yardstick: the sampler's draw loop (point_cloud_sampler_with_normal.h:159-177) built from the standard library's own parts
Result std_draw(uint32_t state, const std::vector<double>& cum, size_t num, std::vector<uint32_t>& out)
{
  std::default_random_engine eng;
  set_state(eng, state);
  std::uniform_real_distribution<double> dist(0, cum.back());
  std::unordered_set<size_t> chosen;
  uint64_t draws = 0;
  do
  {
    const double x = dist(eng);
    ++draws;
    chosen.insert(static_cast<size_t>(std::lower_bound(cum.begin(), cum.end(), x) - cum.begin()));
  } while (chosen.size() < num);
  out.clear();
  for (const size_t id : chosen)
    out.push_back(static_cast<uint32_t>(id));
  return Result{ get_state(eng), draws, 0 };
}

void exclusive_scan(uint32_t* d, uint32_t n)
{
  uint32_t run = 0u;
  for (uint32_t i = 0; i < n; ++i)
  {
    const uint32_t v = d[i];
    d[i] = run;
    run += v;
  }
}

// threads one after the other, forwards or backwards (the steps must not care who wins an atomic)
template <typename F>
void each_thread(uint32_t nthreads, bool backwards, F f)
{
  for (uint32_t k = 0; k < nthreads; ++k)
    f(backwards ? nthreads - 1u - k : k);
}

// one phase with `nthreads` threads; the scan between walk and place is the work-group's / the device scan
void run_phase(const WeightedPhase& ph, uint32_t nthreads, bool backwards)
{
  each_thread(nthreads, backwards, [&](uint32_t t) { weighted_phase_clear(t, nthreads, ph); });
  each_thread(nthreads, backwards, [&](uint32_t t) { weighted_phase_link(t, nthreads, ph); });
  each_thread(nthreads, backwards, [&](uint32_t t) { weighted_phase_walk(t, nthreads, ph); });
  exclusive_scan(ph.size_at, ph.m + 1u);
  each_thread(nthreads, backwards, [&](uint32_t t) { weighted_phase_place(t, nthreads, ph, ph.size_at); });
}

struct Segment
{
  const std::vector<double>* cum;
  uint32_t num;
  std::vector<uint32_t>* out;
};

// rng_weighted_kernels.h: weighted_single_kernel. made[s] = the attempts of segment s
uint32_t single_emul(uint32_t x0, const Segment* segs, int n_seg, bool backwards, uint32_t* made_out)
{
  constexpr uint32_t CAP = WEIGHTED_SINGLE_MAX + 1u;
  constexpr uint32_t T = GROUP_THREADS;
  std::vector<uint32_t> s_ins(CAP), s_cur(CAP), s_next(CAP), s_head(CAP), s_link(CAP), s_first_of(CAP), s_later(CAP), s_size(CAP + 1u);
  uint32_t s_result[2];
  uint32_t x = x0;
  for (int s = 0; s < n_seg; ++s)
  {
    const Segment& sg = segs[s];
    uint32_t made = 0u;
    if (sg.num != 0u)
    {
      if (sg.num > WEIGHTED_SINGLE_MAX || sg.num >= sg.cum->size())
      {
        fprintf(stderr, "single_emul: num %u out of range\n", sg.num);
        exit(2);
      }
      std::vector<uint32_t> first(sg.cum->size(), WEIGHTED_NONE);
      const WeightedCloud cloud{ sg.cum->data(), static_cast<uint32_t>(sg.cum->size()), first.data() };
      uint32_t have = 0u;
      s_result[0] = 0u;
      for (uint32_t pass = 0u; have < sg.num; ++pass)
      {
        uint32_t* att_id = s_link.data();
        uint32_t* flag = s_size.data();
        each_thread(T, backwards, [&](uint32_t t) { weighted_step_draw(t, T, x, g_table, cloud, made, WEIGHTED_PASS, att_id); });
        each_thread(T, backwards, [&](uint32_t t) { weighted_step_flag(t, T, cloud, made, WEIGHTED_PASS, att_id, flag); });
        exclusive_scan(flag, WEIGHTED_PASS + 1u);
        each_thread(T, backwards, [&](uint32_t t)
                    { weighted_step_emit(t, T, x, g_table, made, WEIGHTED_PASS, att_id, flag, have, sg.num, s_ins.data(), s_result); });
        have += flag[WEIGHTED_PASS];
        if (have >= sg.num)
        {
          x = s_result[0];
          made = s_result[1];
        }
        else
        {
          x = minstd_jump(x, 2ull * WEIGHTED_PASS, g_table);
          made += WEIGHTED_PASS;
        }
      }
      const int phases = weighted_phase_count(sg.num);
      uint32_t *cur = s_cur.data(), *next = s_next.data(), m_prev = 0u;
      for (int j = 0; j < phases; ++j)
      {
        const uint32_t b = static_cast<uint32_t>(weighted_bucket_count(j));
        const WeightedPhase ph{ b,           sg.num < b ? sg.num : b, m_prev,         cur,           s_ins.data(), s_head.data(),
                                s_link.data(), s_first_of.data(),       s_later.data(), s_size.data(), next };
        run_phase(ph, T, backwards);
        m_prev = ph.m;
        std::swap(cur, next);
      }
      sg.out->assign(cur, cur + sg.num);
    }
    made_out[s] = made;
  }
  return x;
}

// host_weighted.h: weighted_draw_rounds
Result rounds_emul(uint32_t state_in, const std::vector<double>& cum, uint32_t num, bool backwards, std::vector<uint32_t>& out)
{
  const uint32_t T = 1024u;
  const uint64_t n = cum.size();
  std::vector<uint32_t> first(n, WEIGHTED_NONE), ins(num);
  const WeightedCloud cloud{ cum.data(), static_cast<uint32_t>(n), first.data() };
  uint32_t x = state_in, have = 0u;
  uint64_t made = 0;
  int rounds = 0;
  for (;; ++rounds)
  {
    const uint64_t n_att = std::min<uint64_t>(weighted_attempt_budget(have, num, n), 1ull << 28);
    std::vector<uint32_t> att(n_att), flag(n_att + 3, 0u);
    const uint32_t na = static_cast<uint32_t>(n_att), base = static_cast<uint32_t>(made);
    each_thread(T, backwards, [&](uint32_t t) { weighted_step_draw(t, T, x, g_table, cloud, base, na, att.data()); });
    each_thread(T, backwards, [&](uint32_t t) { weighted_step_flag(t, T, cloud, base, na, att.data(), flag.data()); });
    exclusive_scan(flag.data(), na + 1u);
    each_thread(T, backwards, [&](uint32_t t)
                { weighted_step_emit(t, T, x, g_table, base, na, att.data(), flag.data(), have, num, ins.data(), flag.data() + n_att + 1); });
    if (have + static_cast<uint64_t>(flag[n_att]) >= num)
    {
      x = flag[n_att + 1];
      made = flag[n_att + 2];
      ++rounds;
      break;
    }
    have += flag[n_att];
    x = minstd_jump(x, 2 * n_att, g_table);
    made += n_att;
  }
  const int phases = weighted_phase_count(num);
  const size_t b_last = static_cast<size_t>(weighted_bucket_count(phases - 1));
  std::vector<uint32_t> order[2] = { std::vector<uint32_t>(num), std::vector<uint32_t>(num) };
  std::vector<uint32_t> head(b_last), link(num), first_of(num), later(num), size_at(num + 1u);
  out.assign(num, 0u);
  uint32_t m_prev = 0u;
  int cur = 0;
  for (int j = 0; j < phases; ++j)
  {
    const uint32_t b = static_cast<uint32_t>(weighted_bucket_count(j));
    const WeightedPhase ph{ b,           std::min(num, b), m_prev,       order[cur].data(), ins.data(), head.data(),
                            link.data(), first_of.data(),  later.data(), size_at.data(),    j + 1 == phases ? out.data() : order[cur ^ 1].data() };
    run_phase(ph, T, backwards);
    m_prev = ph.m;
    cur ^= 1;
  }
  return Result{ x, made, rounds };
}

// ---- files -----------------------------------------------------------------------------------------------------------------
template <typename V>
std::vector<V> read_file(const char* path)
{
  FILE* f = fopen(path, "rb");
  if (!f)
  {
    fprintf(stderr, "cannot read %s\n", path);
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<V> v(static_cast<size_t>(bytes) / sizeof(V));
  if (!v.empty() && fread(v.data(), sizeof(V), v.size(), f) != v.size())
    exit(2);
  fclose(f);
  return v;
}
template <typename V>
void write_file(const char* path, const std::vector<V>& v)
{
  FILE* f = fopen(path, "wb");
  if (!f || (!v.empty() && fwrite(v.data(), sizeof(V), v.size(), f) != v.size()))
  {
    fprintf(stderr, "cannot write %s\n", path);
    exit(2);
  }
  fclose(f);
}

// ---- selftest --------------------------------------------------------------------------------------------------------------
int g_bad = 0;

void check_table()
{
  // the real container, grown by single insertions, as far as memory is cheap; beyond that the growth policy object the container
  // itself consults (bits/hashtable_policy.h), asked what _M_need_rehash asks it
  std::unordered_set<size_t> s;
  int phase = -1;
  size_t last = s.bucket_count();
  bool ok = last == 1;
  for (size_t k = 1; k <= 800000; ++k)
  {
    s.insert(k * 2654435761ull);
    if (s.bucket_count() != last)
    {
      last = s.bucket_count();
      ++phase;
      // the rehash happens when element k exceeds the previous bucket count
      const uint64_t prev = phase == 0 ? 0 : weighted_bucket_count(phase - 1);
      ok = ok && phase < WEIGHTED_N_BUCKETS && last == weighted_bucket_count(phase) && k == prev + 1;
    }
  }
  const int grown = phase + 1;
  size_t b = last;
  for (int j = grown; j < WEIGHTED_N_BUCKETS; ++j)
  {
    std::__detail::_Prime_rehash_policy pol;
    b = pol._M_next_bkt(std::max<size_t>(b + 2, 2 * b));
    ok = ok && b == weighted_bucket_count(j);
  }
  printf("table grown=%d policy=%d %s\n", grown, WEIGHTED_N_BUCKETS - grown, ok ? "equal" : "DIFFERENT");
  g_bad += !ok;
}

void check_canonical()
{
  // the one predecessor of the engine's largest output, and the largest c of the stream
  uint64_t inv = 1, base = MINSTD_A, e = MINSTD_M - 2ull;
  for (; e; e >>= 1, base = base * base % MINSTD_M)
    if (e & 1u)
      inv = inv * base % MINSTD_M;
  const uint32_t v1 = static_cast<uint32_t>((MINSTD_M - 1ull) * inv % MINSTD_M);
  const bool pred = v1 == WEIGHTED_V1_BEFORE_MAX && minstd_next(v1) == MINSTD_M - 1u;
  const double c = weighted_canonical(v1, MINSTD_M - 1u);
  // against the library at that state, and at the states in front of the smallest output
  bool lib = true;
  for (uint32_t st : { static_cast<uint32_t>(inv * v1 % MINSTD_M), static_cast<uint32_t>(inv), static_cast<uint32_t>(inv * inv % MINSTD_M), 1u, 2147483646u })
  {
    std::default_random_engine eng;
    set_state(eng, st);
    const double want = std::generate_canonical<double, 53>(eng);
    const uint32_t a = minstd_next(st), b2 = minstd_next(a);
    lib = lib && want == weighted_canonical(a, b2) && get_state(eng) == b2;
  }
  // no v1 at all reaches c >= 1 with the largest v2? (it needs the numerator within ~2^8 of r^2)
  uint32_t lowest_v1_reaching_one = 0u;
  for (uint32_t v = MINSTD_M - 1u; v > MINSTD_M - 100000u; --v)
  {
    double sum = static_cast<double>(v - 1u);
    sum += static_cast<double>(MINSTD_M - 2u) * WEIGHTED_RANGE;
    if (sum / (WEIGHTED_RANGE * WEIGHTED_RANGE) >= 1.0)
      lowest_v1_reaching_one = v;
    else
      break;
  }
  const bool ok = pred && lib && c < 1.0 && (lowest_v1_reaching_one == 0u || lowest_v1_reaching_one > v1);
  printf("canonical v1_before_max=%u c_max=%.17g lowest_v1_reaching_one=%u reachable=%d %s\n", v1, c, lowest_v1_reaching_one,
         (lowest_v1_reaching_one != 0u && v1 >= lowest_v1_reaching_one) ? 1 : 0, ok ? "equal" : "DIFFERENT");
  g_bad += !ok;
}

void chain_case(const std::string& kind, size_t n, uint32_t seed)
{
  const std::vector<double> w = make_weights(kind, n, seed);
  ChainStats st;
  const bool ok = same_bits(chain_emul(w, &st), plain_cumsum(w));
  printf("chain %s n=%zu passes=%lld full=%lld serial_blocks=%lld %s\n", kind.c_str(), n, st.passes, st.full, st.serial_blocks,
         ok ? "equal" : "DIFFERENT");
  g_bad += !ok;
}

void draw_case(const char* name, const std::string& kind, size_t n, uint32_t num, uint32_t state)
{
  const std::vector<double> cum = plain_cumsum(make_weights(kind, n, static_cast<uint32_t>(n) + num));
  std::vector<uint32_t> want, got;
  const Result ref = std_draw(state, cum, num, want);
  bool ok = true;
  int rounds = 0;
  for (int backwards = 0; backwards < 2; ++backwards)
  {
    if (num <= WEIGHTED_SINGLE_MAX)
    {
      const Segment sg{ &cum, num, &got };
      uint32_t made = 0u;
      const uint32_t x = single_emul(state, &sg, 1, backwards != 0, &made);
      ok = ok && got == want && x == ref.state && made == ref.draws;
    }
    const Result r = rounds_emul(state, cum, num, backwards != 0, got);
    ok = ok && got == want && r.state == ref.state && r.draws == ref.draws;
    rounds = r.rounds;
  }
  printf("case %s kind=%s n=%zu num=%u state=%u draws=%llu behind=%u rounds=%d single=%d %s\n", name, kind.c_str(), n, num, state,
         static_cast<unsigned long long>(ref.draws), ref.state, rounds, num <= WEIGHTED_SINGLE_MAX ? 1 : 0, ok ? "equal" : "DIFFERENT");
  g_bad += !ok;
}

void two_case(size_t n0, uint32_t num0, size_t n1, uint32_t num1, uint32_t state)
{
  const std::vector<double> cum0 = plain_cumsum(make_weights("rand", n0, 5u)), cum1 = plain_cumsum(make_weights("rand", n1, 6u));
  std::vector<uint32_t> want0, want1, got0, got1;
  uint32_t st = state;
  uint64_t d0 = 0, d1 = 0;
  if (num0)
  {
    const Result r = std_draw(st, cum0, num0, want0);
    st = r.state;
    d0 = r.draws;
  }
  if (num1)
  {
    const Result r = std_draw(st, cum1, num1, want1);
    st = r.state;
    d1 = r.draws;
  }
  const Segment segs[2] = { { &cum0, num0, &got0 }, { &cum1, num1, &got1 } };
  uint32_t made[2] = { 0u, 0u };
  const uint32_t x = single_emul(state, segs, 2, false, made);
  const bool ok = got0 == want0 && got1 == want1 && x == st && made[0] == d0 && made[1] == d1;
  printf("case two n0=%zu num0=%u n1=%zu num1=%u state=%u draws0=%llu draws1=%llu behind=%u %s\n", n0, num0, n1, num1, state,
         static_cast<unsigned long long>(d0), static_cast<unsigned long long>(d1), st, ok ? "equal" : "DIFFERENT");
  g_bad += !ok;
}

int selftest()
{
  check_table();
  check_canonical();
  for (const char* kind : { "ones", "rand", "ties", "big", "neg", "special" })
    for (size_t n : { 1u, 63u, 64u, 511u, 512u, 513u, 70000u })
      chain_case(kind, n, static_cast<uint32_t>(n));
  for (uint32_t state : { 1u, 12345u, 2147483646u })
    for (uint32_t num : { 1u, 12u, 13u, 14u, 29u, 30u, 59u, 60u, 127u, 128u })
    {
      draw_case("edge", "rand", 600, num, state);
      draw_case("tight", "rand", num + 1u, num, state);
    }
  for (uint32_t num : { 13u, 14u, 128u, 1109u })
    draw_case("ones", "ones", 2000, num, 777u);
  draw_case("tight", "rand", 300, 299, 99u);
  draw_case("tight", "rand", 1110, 1109, 4242u);
  draw_case("cap", "rand", 1500, 1109, 31337u);
  draw_case("cap", "rand", 1500, 1110, 31337u);
  draw_case("cap", "rand", 1111, 1110, 31337u);
  draw_case("large", "rand", 5000, 3000, 2024u);
  draw_case("large", "rand", 65000, 16384, 7u);
  for (uint32_t state : { 1u, 999u })
  {
    two_case(1507, 3, 2893, 96, state);
    two_case(1507, 0, 2893, 96, state);
    two_case(1507, 3, 2893, 0, state);
    two_case(700, 512, 4089, 1109, state);
    two_case(4, 3, 97, 96, state);
  }
  printf(g_bad ? "%d DIFFERENT\n" : "all equal\n", g_bad);
  return g_bad ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv)
{
  minstd_build_table(g_table);
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "selftest")
    return selftest();
  if (cmd == "weights" && argc == 6)
  {
    write_file(argv[5], make_weights(argv[2], strtoull(argv[3], nullptr, 10), static_cast<uint32_t>(strtoul(argv[4], nullptr, 10))));
    return 0;
  }
  if (cmd == "cumsum" && argc == 4)
  {
    write_file(argv[3], plain_cumsum(read_file<double>(argv[2])));
    return 0;
  }
  if (cmd == "chain" && argc == 4)
  {
    ChainStats st;
    write_file(argv[3], chain_emul(read_file<double>(argv[2]), &st));
    printf("passes=%lld full=%lld serial_blocks=%lld\n", st.passes, st.full, st.serial_blocks);
    return 0;
  }
  if (cmd == "draw" && argc == 7)
  {
    const std::string impl = argv[2];
    const uint32_t state = static_cast<uint32_t>(strtoul(argv[3], nullptr, 10));
    const std::vector<double> cum = read_file<double>(argv[4]);
    const uint32_t num = static_cast<uint32_t>(strtoul(argv[5], nullptr, 10));
    if (state < 1u || state > MINSTD_M - 1u || num == 0u || num >= cum.size())
    {
      fprintf(stderr, "draw: state in [1, 2^31 - 2], 0 < num < n\n");
      return 2;
    }
    std::vector<uint32_t> out;
    Result r{ 0u, 0, 0 };
    if (impl == "std")
      r = std_draw(state, cum, num, out);
    else if (impl == "single")
    {
      const Segment sg{ &cum, num, &out };
      uint32_t made = 0u;
      r.state = single_emul(state, &sg, 1, false, &made);
      r.draws = made;
    }
    else if (impl == "rounds")
      r = rounds_emul(state, cum, num, false, out);
    else
      return 2;
    write_file(argv[6], out);
    printf("state=%u draws=%llu rounds=%d\n", r.state, static_cast<unsigned long long>(r.draws), r.rounds);
    return 0;
  }
  if (cmd == "drawtime" && argc == 6)
  {
    const uint32_t state = static_cast<uint32_t>(strtoul(argv[2], nullptr, 10));
    const std::vector<double> cum = read_file<double>(argv[3]);
    const uint32_t num = static_cast<uint32_t>(strtoul(argv[4], nullptr, 10));
    const int reps = atoi(argv[5]);
    if (state < 1u || state > MINSTD_M - 1u || num == 0u || num >= cum.size() || reps < 1)
      return 2;
    double best = 1e300;
    uint64_t draws = 0;
    for (int r = 0; r < reps; ++r)
    {
      std::vector<uint32_t> out;
      const auto t0 = std::chrono::steady_clock::now();
      draws = std_draw(state, cum, num, out).draws;
      best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    printf("host_ms=%.6f draws=%llu\n", best, static_cast<unsigned long long>(draws));
    return 0;
  }
  fprintf(stderr, "usage: see the head of rng_weighted_emul.cpp\n");
  return 2;
}
