// host_group.h — part of the single translation unit mcl3dl_hip.hip: a device group = N contexts (one per GPU) owned by ONE
// host process, the in-process form of SURVEY.md §8e behind the C ABI (the reference node is one C++ process,
// src/mcl_3dl.cpp:1466).  Contiguous particle shards, map + scan replicated, one worker thread per device so that the
// launches of the N GPUs are enqueued concurrently, and ONE collective per update: ncclAllReduce(sum) of 2 + 2N doubles
// over RCCL (librccl is dlopen'ed the first time a group with more than one device needs it — a single-GPU user never
// loads it), or a host-side combine of the same record (collective = "host": used when device ids repeat — several
// contexts on one GPU, which RCCL refuses — and as a fallback when librccl is not installed).
// The threads and the rules by which the ranks enter a collective are host_group_sync.h's (no HIP: tested on a CPU); below
// them here: the shard view of a rank, the voted collective call and the all-reduce of the record.
#pragma once

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enum values only: every RCCL call goes through the dlopen'ed pointers below

#include "host_group_sync.h"  // WorkerPool, VoteBarrier, run_round
#include "shard_layout.h"     // shard_bounds, shard_capacity, the inverse map

namespace
{
struct RcclApi
{
  void* lib = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommAbort) CommAbort = nullptr;   // optional: tears a communicator down with a collective still pending
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;

  // "" on success, otherwise why RCCL is not usable
  std::string load()
  {
    if (lib)
      return "";
    const char* env = getenv("MCL3DL_HIP_RCCL_LIB");
    const char* names[] = { env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
    // a copy that is already in the process (e.g. the one torch brought) is preferred over loading a second one
    for (const char* n : names)
      if (n && !lib)
        lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
    for (const char* n : names)
      if (n && !lib)
        lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!lib)
      return std::string("librccl not found (") + dlerror() + ")";
    CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(lib, "ncclAllReduce"));
    AllGather = reinterpret_cast<decltype(AllGather)>(dlsym(lib, "ncclAllGather"));
    CommAbort = reinterpret_cast<decltype(CommAbort)>(dlsym(lib, "ncclCommAbort"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
    if (!CommInitAll || !CommDestroy || !AllReduce || !AllGather || !GetErrorString)
    {
      lib = nullptr;
      return "librccl lacks ncclCommInitAll / ncclAllReduce / ncclAllGather";
    }
    return "";
  }
};

}  // namespace

// how a sharded call combines its ranks: not at all (a group of one device that may call its context directly: it never loads
// RCCL), through the host ("collective" 1), or over RCCL
enum GroupRoute { ROUTE_DIRECT, ROUTE_HOST, ROUTE_RCCL };

struct mcl3dl_hip_group
{
  std::vector<mcl3dl_hip_ctx*> ctx;
  std::vector<int> devices;
  std::string err;
  int collective = 0;  // 0 = RCCL all-reduce, 1 = host combine
  int direct_single = 1;  // 1 = a group of one device calls its context directly; 0 = it takes the sharded path too
  bool devices_distinct = true;
  WorkerPool pool;
  VoteBarrier vote;
  int inject_failure_rank = -1;  // test hook (option "inject_failure_rank"): that rank fails ahead of the collective, once
  OrderedScan scan;  // ordered once per update, pushed to every device
  // RCCL (created on first use by a group of more than one device)
  RcclApi rccl;
  std::vector<ncclComm_t> comms;
  uint64_t collectives_rccl = 0, collectives_host = 0;
  // per-rank scratch of the host combine
  std::vector<std::vector<double>> host_packed;
  // poses kept on the devices by group_upload_poses
  size_t n_pose_uploaded = 0;
  // the batch mcl3dl_hip_group_measure_batch_begin started
  size_t prog_n_p = 0;
  bool prog_direct = false;
  bool prog_sharded = false;          // every rank holds a progressive batch of its own over its shard (api_group.inl)
  std::vector<bool> prog_done;        // ... ranks whose whole shard has been handed to the caller's arrays
  // particles resident on the devices (api_group_state.inl): 13-float states + weights, sharded by shard_bounds
  size_t n_resident = 0;
  std::vector<float> h_weight, h_state;  // host gather buffers of the resampling steps
  std::vector<double> h_parts;           // per-rank records of the reductions
  size_t rs_n_out = 0;                   // set by group_resample_begin
  bool rs_begun = false, rs_planned = false;
  size_t rs_n_dup = 0;
  // api_group_motion.inl: State6DOF's odometry noise is on the devices (gs_noise) once set_odom_noise installed it; until then, and
  // again after an upload or add_noise, it is zero everywhere and nothing holds or moves it
  bool noise_on = false;
  float odom_sigma = 0.f;        // > 0: update_resident without `extra` forms the odometry factor on the devices
  std::vector<float> h_noise;    // host gather buffer of the resampling step

  // a communicator that saw a failed or abandoned collective: aborted where RCCL can (a pending collective would block a
  // plain destroy), rebuilt by group_comms on next use
  void drop_comms()
  {
    for (ncclComm_t& c : comms)
      if (c)
      {
        if (rccl.CommAbort)
          (void)rccl.CommAbort(c);
        else
          (void)rccl.CommDestroy(c);
        c = nullptr;
      }
    comms.clear();
  }
  void count_collective(bool over_rccl)
  {
    ++(over_rccl ? collectives_rccl : collectives_host);
  }

  int n() const
  {
    return static_cast<int>(ctx.size());
  }
  GroupRoute route() const
  {
    return n() == 1 && direct_single ? ROUTE_DIRECT : collective == 1 ? ROUTE_HOST : ROUTE_RCCL;
  }
  int fail(int code, const char* fmt, ...)
  {
    char buf[640];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
  int fail_rank(int rc, int r)
  {
    return fail(rc, "device %d (rank %d): %s", devices[r], r, ctx[r]->err.c_str());
  }
};

namespace
{
// rank r's view of n_p sharded particles: its context and its shard [lo, lo + n)
struct Shard
{
  mcl3dl_hip_ctx* ctx;
  int r;
  size_t lo, n;
};

inline Shard shard_of(const mcl3dl_hip_group* g, size_t n_p, int r)
{
  size_t lo, hi;
  shard_bounds(n_p, g->n(), r, &lo, &hi);
  return Shard{ g->ctx[r], r, lo, hi - lo };
}

// f(rank) on every rank's worker, the failing rank's error reported; no collective, nothing waits for another rank
template <typename F>
int group_run(mcl3dl_hip_group* g, const F& f)
{
  int bad = 0;
  const int rc = g->pool.run_all(f, &bad);
  return rc ? g->fail_rank(rc, bad) : 0;
}

// ... f(shard), over the shards of n_p particles
template <typename F>
int group_run_shards(mcl3dl_hip_group* g, size_t n_p, const F& f)
{
  return group_run(g, [&](int r) -> int { return f(shard_of(g, n_p, r)); });
}

// f(ctx, rank) on every rank in turn ON THE CALLING THREAD (the setters, and a group of one device that calls its context
// directly), the first failing rank's error reported
template <typename F>
int group_forward(mcl3dl_hip_group* g, const F& f)
{
  for (int r = 0; r < g->n(); ++r)
  {
    const int rc = f(g->ctx[r], r);
    if (rc)
      return g->fail_rank(rc, r);
  }
  return 0;
}

// the guard of every call on the resident particles
inline int group_resident(mcl3dl_hip_group* g)
{
  return g->n_resident ? 0 : g->fail(-5, "no resident particles (mcl3dl_hip_group_upload_state first)");
}

// ... and of a rank: it holds the n particles of its shard
inline int rank_holds(mcl3dl_hip_ctx* ctx, size_t n)
{
  return ctx->gs_n == n ? 0 : ctx->fail(-5, "this device holds %zu resident particles, its shard has %zu", ctx->gs_n, n);
}

// the shard-local calls on the resident particles: f(ctx, rank, lo, n) on every rank whose shard holds particles
template <typename F>
int group_each_shard(mcl3dl_hip_group* g, const F& f)
{
  TRY(group_resident(g));
  return group_run_shards(g, g->n_resident,
                          [&](const Shard& s) -> int
                          {
                            mcl3dl_hip_ctx* ctx = s.ctx;
                            if (s.n == 0)
                              return 0;
                            HIP_TRY(hipSetDevice(ctx->device));
                            TRY(rank_holds(ctx, s.n));
                            return f(ctx, s.r, s.lo, s.n);
                          });
}

// Every rank computed the same `width` words (words[width * r + k]) for itself — deterministic replicas, no collective: rank r is
// held against rank 0 unless either sat the call out (took_part, null: all did). -4 names what differs, the values and the rank.
template <typename W>
int group_agree(mcl3dl_hip_group* g, const char* what, const W* words, size_t width, const char* took_part = nullptr)
{
  for (int r = 1; r < g->n(); ++r)
    for (size_t k = 0; k < width && (!took_part || (took_part[0] && took_part[r])); ++k)
      if (words[width * r + k] != words[k])
        return g->fail(-4, "the ranks disagree on %s (%llu on rank 0, %llu on rank %d)", what,
                       static_cast<unsigned long long>(words[k]), static_cast<unsigned long long>(words[width * r + k]), r);
  return 0;
}

int group_comms(mcl3dl_hip_group* g)
{
  if (g->collective == 1 || !g->comms.empty())
    return 0;
  if (!g->devices_distinct)
    return g->fail(-3, "a device id is listed more than once: RCCL needs one GPU per rank — set option \"collective\" to 1 "
                       "(host combine) for several contexts on one GPU");
  const std::string why = g->rccl.load();
  if (!why.empty())
    return g->fail(-7, "%s; set option \"collective\" to 1 (host combine) or MCL3DL_HIP_RCCL_LIB", why.c_str());
  g->comms.assign(g->n(), nullptr);
  const ncclResult_t rc = g->rccl.CommInitAll(g->comms.data(), g->n(), g->devices.data());
  if (rc != ncclSuccess)
  {
    g->comms.clear();
    return g->fail(-7, "ncclCommInitAll over %d devices failed: %s", g->n(), g->rccl.GetErrorString(rc));
  }
  return 0;
}

// ---- the voted collective call ("One round for every collective") --------------------------------------------
// `what` names the call and `collective` what it enters ("all-reduce", "all-gather") in the error texts.
struct VotedCall
{
  mcl3dl_hip_group* g;
  const char* what;
  const char* collective;
};

// What the part of a rank behind the first vote is handed: enqueued() behind each RCCL collective it enqueued (the second
// vote). 0: go on; else the rank's code — its error text is set — to return at once.
struct VotedRank
{
  const VotedCall& call;
  const Shard& s;
  RoundRank& round;
  int enqueued(ncclResult_t nrc, const char* nccl_call) const
  {
    const int own = nrc == ncclSuccess ? 0 : s.ctx->fail(-7, "%s failed: %s", nccl_call, call.g->rccl.GetErrorString(nrc));
    const int rc = round.enqueued(own);
    // (its stream is NOT drained: the collective in it never completes; the communicators are aborted behind the round)
    return rc != RC_ABANDONED ? rc : s.ctx->fail(RC_ABANDONED, "%s abandoned: another rank could not enqueue the %s", call.what,
                                                 call.collective);
  }
};

// One round (host_group_sync.h:run_round) over the shards of n_p particles: ahead(shard) is everything a rank does in front of
// the collective and waits for no other rank; behind(shard, VotedRank) runs only when EVERY rank's `ahead` succeeded — the
// collective(s), each followed by VotedRank::enqueued, and what follows them. A rank that may not proceed drains its stream,
// drops what it staged and stands down. over_rccl: the communicators are dropped when a rank failed or stood down behind the
// first vote. count: a successful call is one collective of that kind.
template <typename Ahead, typename Behind>
int group_voted_call(const VotedCall& call, size_t n_p, bool over_rccl, bool count, const Ahead& ahead, const Behind& behind)
{
  mcl3dl_hip_group* g = call.g;
  const int inject = g->inject_failure_rank;  // (the test hook: that rank fails behind its `ahead`, once)
  g->inject_failure_rank = -1;
  const RoundVerdict v = run_round(
      g->pool, g->vote, g->n(),
      [&](int r, RoundRank& round) -> int
      {
        const Shard s = shard_of(g, n_p, r);
        int rc = ahead(s);
        if (rc == 0 && r == inject)
          rc = s.ctx->fail(-9, "injected failure ahead of the collective (test hook)");
        rc = round.enter(rc);
        if (rc == 0)
          return behind(s, VotedRank{ call, s, round });
        if (rc == RC_ABANDONED)
          s.ctx->fail(RC_ABANDONED, "%s abandoned: another rank failed ahead of the %s", call.what, call.collective);
        (void)hipStreamSynchronize(s.ctx->stream);  // drain what this rank enqueued; its results are discarded
        s.ctx->stage_reset();
        return rc;
      });
  if (v.rc)
  {
    // communicators that saw a failed or abandoned collective are rebuilt on next use
    if (over_rccl && v.behind_first_vote)
      g->drop_comms();
    return g->fail_rank(v.rc, v.rank);
  }
  if (count)
    g->count_collective(over_rccl);
  return 0;
}

// pf::measure's collective: the record of 2 + 2N doubles in ctx->packed, summed over the ranks. phase_a(shard) enqueues what
// fills the rank's record (the rank's device is current, ctx->packed holds room), phase_b(shard) what reads the total and
// brings the rank's results home. RCCL: ncclAllReduce on the rank's stream and phase B behind it on the same worker; host
// combine (collective = 1): the records come home, are summed in rank order (deterministic) and go back up in a second pass
// over the workers, which runs phase B; a group of one device that may call its context directly needs no collective (and
// never loads RCCL): phase B follows phase A.
template <typename PhaseA, typename PhaseB>
int group_allreduce_record(mcl3dl_hip_group* g, const char* what, size_t n_p, const PhaseA& phase_a, const PhaseB& phase_b)
{
  const int N = g->n();
  const bool host_combine = g->route() == ROUTE_HOST, over_rccl = g->route() == ROUTE_RCCL;
  if (over_rccl)
    TRY(group_comms(g));
  const size_t n_pack = 2 + 2 * static_cast<size_t>(N);
  TRY(group_voted_call(
      VotedCall{ g, what, "all-reduce" }, n_p, over_rccl, over_rccl,
      [&](const Shard& s) -> int
      {
        mcl3dl_hip_ctx* ctx = s.ctx;
        HIP_TRY(hipSetDevice(ctx->device));
        TRY(ensure(ctx, ctx->packed, sizeof(double) * n_pack));
        return phase_a(s);
      },
      [&](const Shard& s, const VotedRank& voted) -> int
      {
        mcl3dl_hip_ctx* ctx = s.ctx;
        if (host_combine)
        {
          g->host_packed[s.r].resize(n_pack);
          TRY(d2h(ctx, g->host_packed[s.r].data(), ctx->packed.p, sizeof(double) * n_pack));
          return sync_stream(ctx);
        }
        if (over_rccl)
          // the call's single collective: 16 + 16 N bytes over xGMI, on this device's stream
          TRY(voted.enqueued(g->rccl.AllReduce(ctx->packed.p, ctx->packed.p, n_pack, ncclDouble, ncclSum, g->comms[s.r], ctx->stream),
                             "ncclAllReduce"));
        return phase_b(s);
      }));
  if (!host_combine)
    return 0;
  double total[2 + 2 * ROUND_MAX_RANKS] = {};
  for (int r = 0; r < N; ++r)
    for (size_t i = 0; i < n_pack; ++i)
      total[i] += g->host_packed[r][i];
  TRY(group_run_shards(g, n_p,
                       [&](const Shard& s) -> int
                       {
                         mcl3dl_hip_ctx* ctx = s.ctx;
                         HIP_TRY(hipSetDevice(ctx->device));
                         TRY(h2d(ctx, ctx->packed.p, total, sizeof(double) * n_pack));
                         return phase_b(s);
                       }));
  g->count_collective(false);
  return 0;
}
}  // namespace
