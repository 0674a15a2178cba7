// host_group_sync.h — the thread synchronisation of a device group (host_group.h), free of HIP: nothing but the C++ standard
// library, so that tests/cpp/group_sync_check.cpp runs it on a CPU (plain, ThreadSanitizer, AddressSanitizer + UBSan).
//
//   WorkerPool    one thread per rank; run_all() hands every rank the same closure and waits for all
//   VoteBarrier   every rank casts one vote and gets the conjunction back
//   run_round     one vote-and-collective round over the pool: the rules by which the ranks enter a collective together
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace
{
inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  __asm__ __volatile__("yield");
#endif
}

// One worker thread per device; run_all() hands every worker the same closure (argument = rank) and waits for all.
// Hand-over and completion are SPUN on for a short while before anybody sleeps on a condition variable: updates follow
// each other within a fraction of a millisecond while a filter runs, and a futex wake-up costs 20 - 50 us per hop — two hops
// per update, a tenth of a C2 update. A worker that has seen no task for SPIN_US goes to sleep (an idle filter burns nothing);
// the caller spins while the ranks work (that is its only job) and sleeps only behind a long update.
class WorkerPool
{
public:
  void start(int n)
  {
    rc_.assign(n, 0);
    for (int r = 0; r < n; ++r)
      threads_.emplace_back([this, r] { loop(r); });
  }
  void stop()
  {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_.store(true, std::memory_order_release);
    }
    cv_task_.notify_all();
    for (std::thread& t : threads_)
      t.join();
    threads_.clear();
  }
  // returns the first non-zero return code (by rank), 0 if every rank succeeded
  int run_all(const std::function<int(int)>& f, int* failed_rank)
  {
    if (threads_.empty())
    {
      const int rc = f(0);
      if (rc != 0 && failed_rank)
        *failed_rank = 0;
      return rc;
    }
    task_ = &f;
    pending_.store(static_cast<int>(threads_.size()), std::memory_order_relaxed);
    gen_.fetch_add(1);  // publishes task_ and pending_ (sequentially consistent: paired with the sleeper's count-then-look)
    if (sleepers_.load() > 0)
    {
      std::lock_guard<std::mutex> lk(m_);  // (a worker between its last look at gen_ and its wait holds m_)
      cv_task_.notify_all();
    }
    // completion: spin, then sleep
    const auto t0 = std::chrono::steady_clock::now();
    bool done = false;
    for (long spin = 0; !(done = pending_.load(std::memory_order_acquire) == 0); ++spin)
    {
      cpu_relax();
      if ((spin & 1023) == 1023 &&
          std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > 2000.0)
        break;
    }
    if (!done)
    {
      std::unique_lock<std::mutex> lk(m_);
      waiter_.store(true);  // (sequentially consistent, like the worker's decrement-then-look: one of the two sees the other)
      cv_done_.wait(lk, [this] { return pending_.load() == 0; });
      waiter_.store(false);
    }
    task_ = nullptr;
    for (size_t r = 0; r < rc_.size(); ++r)
      if (rc_[r] != 0)
      {
        if (failed_rank)
          *failed_rank = static_cast<int>(r);
        return rc_[r];
      }
    return 0;
  }

private:
  static constexpr double SPIN_US = 300.0;
  void loop(int r)
  {
    uint64_t seen = 0;
    for (;;)
    {
      // the next task: spin for a while, then sleep
      const auto t0 = std::chrono::steady_clock::now();
      bool have = false;
      for (long spin = 0; !stop_.load(std::memory_order_acquire); ++spin)
      {
        if (gen_.load(std::memory_order_acquire) != seen)
        {
          have = true;
          break;
        }
        cpu_relax();
        if ((spin & 255) == 255 &&
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > SPIN_US)
          break;
      }
      if (!have)
      {
        std::unique_lock<std::mutex> lk(m_);
        sleepers_.fetch_add(1);
        cv_task_.wait(lk, [&] { return stop_.load() || gen_.load() != seen; });
        sleepers_.fetch_sub(1);
      }
      if (stop_.load(std::memory_order_acquire))
        return;
      seen = gen_.load(std::memory_order_acquire);
      const std::function<int(int)>* f = task_;
      rc_[r] = (*f)(r);
      if (pending_.fetch_sub(1) == 1 && waiter_.load())
      {
        std::lock_guard<std::mutex> lk(m_);
        cv_done_.notify_one();
      }
    }
  }
  std::vector<std::thread> threads_;
  std::mutex m_;
  std::condition_variable cv_task_, cv_done_;
  const std::function<int(int)>* task_ = nullptr;
  std::atomic<uint64_t> gen_{ 0 };
  std::atomic<int> pending_{ 0 }, sleepers_{ 0 };
  std::atomic<bool> stop_{ false }, waiter_{ false };
  std::vector<int> rc_;
};

// Every worker of one run_all() casts one vote and gets the conjunction of all votes back. The update's collective is
// enqueued only when every rank reached it: a rank whose upload / launch failed must not leave the others blocked inside
// an all-reduce that can never complete (api_group.inl, the RCCL path).
class VoteBarrier
{
public:
  void resize(int n)
  {
    n_ = n;
  }
  bool vote(bool ok)
  {
    if (n_ <= 1)
      return ok;
    std::unique_lock<std::mutex> lk(m_);
    const uint64_t gen = gen_;
    if (count_ == 0)
      all_ok_ = true;
    all_ok_ = all_ok_ && ok;
    if (++count_ == n_)
    {
      result_[gen & 1] = all_ok_;
      count_ = 0;
      ++gen_;
      cv_.notify_all();
      return result_[gen & 1];
    }
    cv_.wait(lk, [&] { return gen_ != gen; });
    return result_[gen & 1];
  }

private:
  std::mutex m_;
  std::condition_variable cv_;
  int n_ = 1, count_ = 0;
  uint64_t gen_ = 0;
  bool all_ok_ = true, result_[2] = { true, true };
};

// ---- one round: every rank enters a collective, or none does -----------------------------------------------------------
// The code of a rank that did nothing wrong and stood down because another rank may not proceed.
constexpr int RC_ABANDONED = -8;
constexpr int ROUND_MAX_RANKS = 64;

// What the round hands a rank's body. Both calls are votes: every rank of the round makes the same calls in the same order
// (enter() once, enqueued() once behind each collective it enqueues), whatever its own result is — a rank that does not vote
// leaves the others waiting. Each returns 0 when all ranks voted ok, the rank's own code when it failed, RC_ABANDONED when
// another rank did; a rank that gets non-zero back returns at once and votes no more (no rank got 0, so none goes on).
class RoundRank
{
public:
  RoundRank(VoteBarrier* vote, bool* entered) : vote_(vote), entered_(entered)
  {
  }
  // the first vote, with the result of everything the rank did ahead of the collective
  int enter(int own_rc)
  {
    const int rc = cast(own_rc);
    *entered_ = rc == 0;
    return rc;
  }
  // the second vote, with the result of enqueueing a collective: one that a rank could not enqueue never completes on the
  // ranks that did, so nobody may wait for it
  int enqueued(int own_rc)
  {
    return cast(own_rc);
  }

private:
  int cast(int own_rc)
  {
    const bool all_ok = vote_->vote(own_rc == 0);
    return own_rc != 0 ? own_rc : (all_ok ? 0 : RC_ABANDONED);
  }
  VoteBarrier* vote_;
  bool* entered_;
};

struct RoundVerdict
{
  int rc = 0;    // 0, or the code of the lowest rank that FAILED (not one that stood down); run_all's where there is none
  int rank = 0;  // ... and that rank
  // a rank failed or stood down behind the first vote: a collective may be enqueued on some ranks and not on others
  bool behind_first_vote = false;
};

// body(rank, RoundRank&) -> the rank's final code, on every rank of the pool (n ranks, n <= ROUND_MAX_RANKS)
template <typename Body>
RoundVerdict run_round(WorkerPool& pool, VoteBarrier& vote, int n, const Body& body)
{
  int code[ROUND_MAX_RANKS] = {};
  bool entered[ROUND_MAX_RANKS] = {};
  RoundVerdict v;
  v.rc = pool.run_all(
      [&](int r) -> int
      {
        RoundRank rank(&vote, &entered[r]);
        return code[r] = body(r, rank);
      },
      &v.rank);
  for (int r = n - 1; r >= 0; --r)
  {
    if (code[r] != 0 && code[r] != RC_ABANDONED)
    {
      v.rc = code[r];
      v.rank = r;
    }
    v.behind_first_vote = v.behind_first_vote || (entered[r] && code[r] != 0);
  }
  return v;
}
}  // namespace
