// rng_shuffle_emul.cpp — rng_shuffle_kernels.h's form of std::shuffle(iota(n), engine), replayed on the CPU from the headers the
// kernels compile (mcl_3dl_amd/csrc/rng_stream.h: the lane walk and the placement loop; rng_shuffle.h: the doubt policy and the
// rest): runs of E attempts per lane behind one jump, rng_emul_common.h's stand-in for 64-lane ballots and 256-thread
// work-groups for the doubtful attempts (count, exclusive scan, emit in stream order), the one-wavefront resolve that speculates 64
// entries at a time, the step of every attempt from the sorted rejections, the sort's contract (stable, by j_i on the bits of
// n - 1) and one chain walk per entry; around them the host's rounds with shuffle_attempt_budget. Its yardstick is the standard
// library itself: std::shuffle over std::default_random_engine (libstdc++), both of its paths. The header's serial loop — what
// the library runs on the host for n <= 46340 — is held against the same.
//
//   rng_shuffle_emul selftest                     every case of tests/test_rng_shuffle_cpu.py, "all equal" at the end
//   rng_shuffle_emul shuffle <std|serial|device> <state> <n> <m> <out.bin>
//        prints "state=<engine state behind the whole shuffle> rounds=<r> attempts=<a> doubtful=<d> rejected=<j> hops=<h>" and
//        writes the first m entries as uint32
//   rng_shuffle_emul time <state> <n> <repeats>   std::iota + std::shuffle of n size_t, as pf.h:320-324: "ms_per_call=<t>"
// g++ -O2.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../mcl_3dl_amd/csrc/rng_shuffle.h"
#include "rng_emul_common.h"

namespace
{
struct Result
{
  uint32_t state = 0;
  int rounds = 0;
  uint64_t attempts = 0;  // engine calls made (std, serial: by the engine state) / attempts evaluated by the last round (device)
  uint64_t doubtful = 0, rejected = 0;
  uint32_t hops = 0;  // the longest chain walk
};

// the yardstick: pf.h:320-324
Result std_shuffle(uint64_t n, uint32_t state, std::vector<uint32_t>& out)
{
  std::default_random_engine eng;
  set_state(eng, state);
  std::vector<size_t> indices(n);
  std::iota(indices.begin(), indices.end(), 0);
  std::shuffle(indices.begin(), indices.end(), eng);
  out.assign(indices.begin(), indices.end());
  Result r;
  r.state = get_state(eng);
  return r;
}

// rng_shuffle.h's serial loop: what the library runs on the host (force_single = false), or the single path at any n
Result serial_shuffle(uint64_t n, uint32_t state, bool force_single, std::vector<uint32_t>& out)
{
  out.resize(n);
  Result r;
  r.state = state;
  shuffle_serial(n, &r.state, out.data(), force_single, &r.attempts);
  r.rejected = r.attempts - (force_single || !shuffle_pair_path(n) ? n - 1 : n / 2);
  return r;
}

// shuffle_resolve_kernel: one wavefront, 64 entries speculated at a time
void resolve_wave(const std::vector<uint32_t>& doubt_t, const std::vector<uint32_t>& doubt_v, uint64_t n, uint64_t n_att,
                  std::vector<uint32_t>& rejected_t, uint32_t* result)
{
  const uint32_t n_doubt = static_cast<uint32_t>(doubt_t.size());
  rejected_t.assign(n_doubt, 0u);
  uint32_t d0 = 0, rejected = 0;
  while (d0 < n_doubt)
  {
    uint64_t events = 0, beyond = 0;
    uint32_t t_of[64];
    for (uint32_t lane = 0; lane < 64; ++lane)
    {
      const uint32_t d = d0 + lane;
      const bool have = d < n_doubt;
      t_of[lane] = have ? doubt_t[d] : 0u;
      const uint32_t v = have ? doubt_v[d] : 1u;
      const int verdict = have ? shuffle_resolve(t_of[lane], v, rejected, n) : SHUFFLE_ACCEPTED;
      events |= static_cast<uint64_t>(verdict != SHUFFLE_ACCEPTED) << lane;
      beyond |= static_cast<uint64_t>(verdict == SHUFFLE_BEYOND) << lane;
    }
    if (events == 0)
    {
      d0 += 64;
      continue;
    }
    const uint32_t first = static_cast<uint32_t>(__builtin_ffsll(static_cast<long long>(events))) - 1u;
    if ((beyond >> first) & 1ull)
      break;
    rejected_t[rejected] = t_of[first];
    ++rejected;
    d0 += first + 1;
  }
  result[0] = rejected;
  result[1] = n_att - rejected >= n - 1 ? 1u : 0u;
}

// host_shuffle.h: shuffle_prefix_device with its kernels replayed work-group by work-group. short_budget: the first round
// evaluates n - 1 attempts and no more, so that every stream with a rejection takes a second round.
Result device_shuffle(uint64_t n, uint64_t m, uint32_t x0, bool short_budget, std::vector<uint32_t>& out)
{
  Result res;
  uint64_t n_att = 0, accepted = 0;
  uint32_t n_rejected = 0;
  std::vector<uint32_t> rejected_t;
  const DoubtPolicy policy{ n };
  for (;;)
  {
    ++res.rounds;
    n_att = short_budget && res.rounds == 1 ? n - 1 : policy.budget(n_att, accepted);
    const std::vector<uint32_t> counts = count_and_scan(policy, x0, n_att);
    const uint32_t n_doubt = counts.back();
    res.attempts = n_att;
    res.doubtful = n_doubt;
    n_rejected = 0;
    rejected_t.clear();
    if (n_doubt == 0)
      break;
    std::vector<uint32_t> doubt_t(n_doubt, 0u), doubt_v(n_doubt, 0u);
    emit_groups(policy, x0, n_att, counts, 0, n_doubt,
                [&](uint64_t rank, uint64_t t, uint32_t v)  // rng_shuffle_kernels.h: DoubtSink
                {
                  doubt_t.at(rank) = static_cast<uint32_t>(t);
                  doubt_v.at(rank) = v;
                });
    uint32_t home[2];
    resolve_wave(doubt_t, doubt_v, n, n_att, rejected_t, home);
    n_rejected = home[0];
    if (home[1])
      break;
    accepted = n_att - n_rejected;
  }
  res.rejected = n_rejected;
  const uint64_t n_used = (n - 1) + n_rejected;
  // shuffle_targets_kernel, lane by lane
  std::vector<uint32_t> target(n, 0xffffffffu);
  for (uint64_t lane = 0; lane * E < n_used; ++lane)
  {
    const uint64_t t0 = lane * E;
    uint32_t rb = 0, len = n_rejected;
    while (len > 0)
    {
      const uint32_t half = len >> 1;
      if (rejected_t[rb + half] < t0)
      {
        rb += half + 1;
        len -= half + 1;
      }
      else
        len = half;
    }
    uint32_t next_rejected = rb < n_rejected ? rejected_t[rb] : 0xffffffffu;
    uint32_t x = minstd_jump(x0, t0, g_table);
    for (int e = 0; e < E; ++e)
    {
      x = minstd_next(x);
      const uint64_t t = t0 + e;
      if (t >= n_used)
        break;
      if (t == next_rejected)
      {
        ++rb;
        next_rejected = rb < n_rejected ? rejected_t[rb] : 0xffffffffu;
        continue;
      }
      const uint64_t step = 1 + t - rb;
      if (step < n)
        target.at(step) = shuffle_target(static_cast<uint32_t>(step), x);
    }
  }
  // the sort's contract: pairs (target[i], i - 1), stable, by the key's low bits_for(n - 1) bits
  int bits = 1;
  while (bits < 64 && ((n - 1) >> bits))
    ++bits;
  const uint32_t mask = bits >= 32 ? 0xffffffffu : ((1u << bits) - 1u);
  std::vector<uint32_t> order(n - 1);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return (target[a + 1] & mask) < (target[b + 1] & mask); });
  std::vector<uint32_t> keys(n - 1), steps(n - 1);
  for (uint64_t k = 0; k + 1 < n; ++k)
  {
    keys[k] = target[order[k] + 1];
    steps[k] = order[k];
  }
  // shuffle_chain_kernel: one lane per entry
  out.resize(m);
  for (uint64_t p = 0; p < m; ++p)
  {
    uint32_t hops = 0;
    out[p] = shuffle_entry(keys.data(), steps.data(), static_cast<uint32_t>(n), target.data(), static_cast<uint32_t>(p), &hops);
    res.hops = std::max(res.hops, hops);
  }
  res.state = minstd_jump(x0, n_used, g_table);
  return res;
}

int g_fail = 0;

void report(const char* what, uint64_t n, uint64_t m, uint32_t state, const Result& r, uint32_t behind, bool ok)
{
  printf("case %s n=%llu m=%llu state=%u rounds=%d attempts=%llu doubtful=%llu rejected=%llu hops=%u behind=%u %s\n", what,
         static_cast<unsigned long long>(n), static_cast<unsigned long long>(m), state, r.rounds,
         static_cast<unsigned long long>(r.attempts), static_cast<unsigned long long>(r.doubtful),
         static_cast<unsigned long long>(r.rejected), r.hops, behind, ok ? "equal" : "DIFFERENT");
  if (!ok)
    ++g_fail;
}

bool prefix_equal(const std::vector<uint32_t>& whole, const std::vector<uint32_t>& prefix)
{
  return prefix.size() <= whole.size() && std::equal(prefix.begin(), prefix.end(), whole.begin());
}

int selftest()
{
  const uint32_t inv = modpow(MINSTD_A, MINSTD_M - 2);           // the state whose next output is 1 (ret = 0)
  const uint32_t before_max = minstd_mulmod(MINSTD_M - 1, inv);  // ... whose next output is 2^31 - 2 (ret = urngrange)
  if (minstd_next(inv) != 1u || minstd_next(before_max) != MINSTD_M - 1u)
  {
    printf("edge states wrong\n");
    return 1;
  }
  // the threshold between the library's two paths, and the 32-bit step range against rng_index.h's
  if (!shuffle_pair_path(46340) || shuffle_pair_path(46341) || !shuffle_pair_path(1))
  {
    printf("shuffle_pair_path DIFFERENT\n");
    ++g_fail;
  }
  for (uint64_t i : { 1ull, 2ull, 95ull, 46340ull, 450407ull, 1499999999ull, 2147483644ull, 2147483645ull })
  {
    const IndexRange a = shuffle_step_range(static_cast<uint32_t>(i)), b = index_range(i + 1);
    if (a.scaling != b.scaling || a.past != b.past)
    {
      printf("shuffle_step_range %llu DIFFERENT\n", static_cast<unsigned long long>(i));
      ++g_fail;
    }
  }
  // pf.h:326-331 in float: 450408 * 0.1f is 45040.8 in double and in float; 46341 * 0.7f = 32438.7 in either; a product whose
  // float rounding reaches the next integer: 200001 * 0.75f = 150000.75 -> float 150000.75 (exact), 16777217 * 1.0f - handled by
  // ratio >= 1. (float)n * ratio with n = 33554435 (rounds to 33554436) and ratio 0.5f gives 16777218, the double product 16777217.
  {
    const struct
    {
      size_t n;
      float ratio;
      size_t want;
    } counts[] = { { 450408, 0.1f, 45040 }, { 46341, 0.75f, 34755 }, { 200001, 0.75f, 150000 }, { 4096, 0.1f, 409 },
                   { 33554435, 0.5f, 16777218 }, { 10, 0.05f, 0 }, { 7, 0.99999994f, 6 } };
    for (const auto& c : counts)
      if (shuffle_sample_count(c.n, c.ratio) != c.want)
      {
        printf("shuffle_sample_count(%zu, %g) = %zu DIFFERENT\n", c.n, static_cast<double>(c.ratio),
               shuffle_sample_count(c.n, c.ratio));
        ++g_fail;
      }
  }
  const uint32_t starts[] = { minstd_seed(1u), minstd_seed(12345u), minstd_seed(2147483646u), inv, before_max };
  std::vector<uint32_t> want, ser, dev;
  // the library's single path: the standard library, the header's serial loop and the replayed kernels
  for (uint64_t n : { 46341ull, 46342ull, 50000ull, 65537ull, 200001ull, 450408ull })
    for (uint32_t s : starts)
    {
      const Result w = std_shuffle(n, s, want);
      const Result a = serial_shuffle(n, s, false, ser);
      const Result b = device_shuffle(n, n, s, false, dev);
      const bool ok = want == ser && want == dev && w.state == a.state && w.state == b.state && a.rejected == b.rejected;
      report("single", n, n, s, b, w.state, ok);
    }
  // the library's pair path, both parities of n and the threshold: the standard library and the header's serial loop
  for (uint64_t n : { 1ull, 2ull, 3ull, 4ull, 5ull, 7ull, 8ull, 100ull, 101ull, 1000ull, 46339ull, 46340ull })
    for (uint32_t s : starts)
    {
      const Result w = std_shuffle(n, s, want);
      Result a = serial_shuffle(n, s, false, ser);
      a.rounds = 0;
      report("pair", n, n, s, a, w.state, want == ser && w.state == a.state);
    }
  // the single path forced at sizes around a wavefront, a work-group's 2048 attempts and two of them: the header's serial loop
  // with the same path forced and the replayed kernels
  for (uint64_t n : { 2ull, 3ull, 64ull, 65ull, 257ull, 2048ull, 2049ull, 2050ull, 4097ull })
    for (uint32_t s : starts)
    {
      const Result a = serial_shuffle(n, s, true, ser);
      const Result b = device_shuffle(n, n, s, false, dev);
      report("forced", n, n, s, b, a.state, ser == dev && a.state == b.state && a.rejected == b.rejected);
    }
  // a first round that falls short: n - 1 attempts and not one more
  for (uint64_t n : { 46341ull, 200001ull, 450408ull })
  {
    const uint32_t s = starts[0];
    const Result w = std_shuffle(n, s, want);
    const Result b = device_shuffle(n, n, s, true, dev);
    report("short", n, n, s, b, w.state, want == dev && w.state == b.state);
  }
  // a doubtful list of several batches of 64 with hundreds of rejections inside
  {
    const uint64_t n = 2000001;
    const uint32_t s = starts[1];
    const Result w = std_shuffle(n, s, want);
    const Result b = device_shuffle(n, n / 10, s, false, dev);
    report("long", n, n / 10, s, b, w.state, prefix_equal(want, dev) && w.state == b.state);
  }
  // a prefix alone
  for (uint64_t n : { 46341ull, 200001ull })
    for (uint64_t m : { static_cast<uint64_t>(1), n / 10 })
    {
      const uint32_t s = starts[0];
      const Result w = std_shuffle(n, s, want);
      const Result b = device_shuffle(n, m, s, false, dev);
      report("prefix", n, m, s, b, w.state, dev.size() == m && prefix_equal(want, dev) && w.state == b.state);
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
  if (argc == 7 && !strcmp(argv[1], "shuffle"))
  {
    const std::string impl = argv[2];
    const uint32_t state = static_cast<uint32_t>(strtoul(argv[3], nullptr, 10));
    const uint64_t n = strtoull(argv[4], nullptr, 10), m = strtoull(argv[5], nullptr, 10);
    if (state < 1u || state > MINSTD_M - 1u || n < 1 || n > SHUFFLE_MAX_N || m > n)
      return 2;
    std::vector<uint32_t> out;
    Result r;
    if (impl == "std")
      r = std_shuffle(n, state, out);
    else if (impl == "serial")
      r = serial_shuffle(n, state, false, out);
    else if (impl == "device" && n >= 2 && m >= 1)
      r = device_shuffle(n, m, state, false, out);
    else
      return 2;
    out.resize(m);
    FILE* f = fopen(argv[6], "wb");
    if (!f || fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size())
      return 3;
    fclose(f);
    printf("state=%u rounds=%d attempts=%llu doubtful=%llu rejected=%llu hops=%u\n", r.state, r.rounds,
           static_cast<unsigned long long>(r.attempts), static_cast<unsigned long long>(r.doubtful),
           static_cast<unsigned long long>(r.rejected), r.hops);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "time"))
  {
    const uint32_t state = static_cast<uint32_t>(strtoul(argv[2], nullptr, 10));
    const uint64_t n = strtoull(argv[3], nullptr, 10);
    const int repeats = atoi(argv[4]);
    if (state < 1u || state > MINSTD_M - 1u || n < 1 || n > SHUFFLE_MAX_N || repeats < 1)
      return 2;
    std::default_random_engine eng;
    set_state(eng, state);
    size_t sink = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < repeats; ++k)
    {
      std::vector<size_t> indices(n);
      std::iota(indices.begin(), indices.end(), 0);
      std::shuffle(indices.begin(), indices.end(), eng);
      sink += indices[0];
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("ms_per_call=%.4f sink=%zu\n", ms / repeats, sink);
    return 0;
  }
  fprintf(stderr, "usage: %s selftest | shuffle <std|serial|device> <state> <n> <m> <out.bin> | time <state> <n> <repeats>\n",
          argv[0]);
  return 2;
}
