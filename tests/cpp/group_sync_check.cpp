// group_sync_check.cpp — stand-alone CPU check of mcl_3dl_amd/csrc/host_group_sync.h (tests/test_group_sync_cpu.py builds it
// plain, with ThreadSanitizer and with AddressSanitizer + UBSan): the worker pool, the vote barrier and the round by which a
// device group's ranks enter a collective together, with fake ranks whose "GPU work" is a counter.
#include "host_group_sync.h"

#include <cstdio>
#include <cstdlib>

namespace
{
int failures = 0;

#define CHECK(cond)                                                          \
  do                                                                         \
  {                                                                          \
    if (!(cond))                                                             \
    {                                                                        \
      ++failures;                                                            \
      std::printf("FAILED %s:%d (N = %d): %s\n", __FILE__, __LINE__, n_ranks, #cond); \
    }                                                                        \
  } while (0)

// a group as mcl3dl_hip_group_create sets it up: worker threads only for more than one rank
struct FakeGroup
{
  explicit FakeGroup(int n) : n(n)
  {
    if (n > 1)
      pool.start(n);
    vote.resize(n);
  }
  ~FakeGroup()
  {
    pool.stop();
  }
  int n;
  WorkerPool pool;
  VoteBarrier vote;
  // what each rank did in the last round (written by the rank's own thread, read behind run_all)
  int phase_a[ROUND_MAX_RANKS], collective[ROUND_MAX_RANKS], phase_b[ROUND_MAX_RANKS], code[ROUND_MAX_RANKS];

  // fail_a / fail_c: bit r set = rank r fails ahead of the first vote / cannot enqueue its collective
  RoundVerdict round(unsigned fail_a, unsigned fail_c, int work_ms = 0)
  {
    for (int r = 0; r < n; ++r)
      phase_a[r] = collective[r] = phase_b[r] = code[r] = 0;
    return run_round(pool, vote, n,
                     [&](int r, RoundRank& rank) -> int
                     {
                       ++phase_a[r];
                       if (work_ms)
                         std::this_thread::sleep_for(std::chrono::milliseconds(work_ms));
                       const int rc_a = rank.enter((fail_a >> r) & 1u ? -100 - r : 0);
                       if (rc_a != 0)
                         return code[r] = rc_a;
                       ++collective[r];
                       const int rc_c = rank.enqueued((fail_c >> r) & 1u ? -200 - r : 0);
                       if (rc_c != 0)
                         return code[r] = rc_c;
                       ++phase_b[r];
                       return code[r] = 0;
                     });
  }
};

void check_ok(FakeGroup& g, const RoundVerdict& v)
{
  const int n_ranks = g.n;
  CHECK(v.rc == 0 && !v.behind_first_vote);
  for (int r = 0; r < g.n; ++r)
    CHECK(g.phase_a[r] == 1 && g.collective[r] == 1 && g.phase_b[r] == 1 && g.code[r] == 0);
}

// `bad` (the lowest failing rank) failed ahead of the first vote
void check_failed_first(FakeGroup& g, const RoundVerdict& v, int bad, unsigned fail_a)
{
  const int n_ranks = g.n;
  CHECK(v.rc == -100 - bad && v.rank == bad && !v.behind_first_vote);
  for (int r = 0; r < g.n; ++r)
  {
    CHECK(g.phase_a[r] == 1 && g.collective[r] == 0 && g.phase_b[r] == 0);
    CHECK(g.code[r] == ((fail_a >> r) & 1u ? -100 - r : RC_ABANDONED));
  }
}

// `bad` (the lowest failing rank) could not enqueue its collective
void check_failed_second(FakeGroup& g, const RoundVerdict& v, int bad, unsigned fail_c)
{
  const int n_ranks = g.n;
  CHECK(v.rc == -200 - bad && v.rank == bad && v.behind_first_vote);
  for (int r = 0; r < g.n; ++r)
  {
    CHECK(g.phase_a[r] == 1 && g.collective[r] == 1 && g.phase_b[r] == 0);
    CHECK(g.code[r] == ((fail_c >> r) & 1u ? -200 - r : RC_ABANDONED));
  }
}

void check_group(int n)
{
  const int failures_before = failures;
  FakeGroup g(n);
  // 1. every rank ok
  check_ok(g, g.round(0, 0));
  // 2. / 3. each rank as the one that fails, at either vote
  for (int bad = 0; bad < n; ++bad)
  {
    check_failed_first(g, g.round(1u << bad, 0), bad, 1u << bad);
    check_failed_second(g, g.round(0, 1u << bad), bad, 1u << bad);
    check_ok(g, g.round(0, 0));
  }
  // 4. two ranks fail at once: the lower one is reported
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b)
    {
      const unsigned both = (1u << a) | (1u << b);
      check_failed_first(g, g.round(both, 0), a, both);
      check_failed_second(g, g.round(0, both), a, both);
      // (one ahead of the first vote, one that would have failed behind it: the collective is never reached)
      check_failed_first(g, g.round(1u << b, 1u << a), b, 1u << b);
    }
  // 5. rounds back to back: the barrier's generations and the pool's hand-over are reused without a pause
  for (int k = 0; k < 2000; ++k)
  {
    const int bad = k % n;
    switch (k % 3)
    {
      case 0:
        check_ok(g, g.round(0, 0));
        break;
      case 1:
        check_failed_first(g, g.round(1u << bad, 0), bad, 1u << bad);
        break;
      default:
        check_failed_second(g, g.round(0, 1u << bad), bad, 1u << bad);
        break;
    }
  }
  // 6. the workers have gone to sleep behind a pause: the round wakes them; and a round whose ranks work for longer than the
  // caller spins puts the caller to sleep
  for (int k = 0; k < 3; ++k)
  {
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
    check_ok(g, g.round(0, 0));
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
    check_failed_first(g, g.round(1u << (k % n), 0), k % n, 1u << (k % n));
  }
  check_ok(g, g.round(0, 0, 4));
  check_failed_second(g, g.round(0, 1u << (n - 1), 4), n - 1, 1u << (n - 1));
  if (failures == failures_before)
    std::printf("N = %d: ok\n", n);
}
}  // namespace

int main()
{
  for (int n : { 1, 2, 3, 5 })
    check_group(n);
  if (failures)
  {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
