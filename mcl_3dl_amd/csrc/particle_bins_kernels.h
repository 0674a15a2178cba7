// particle_bins_kernels.h — which cells of a pose grid the particles occupy, by how many particles and by how much weight
// (particle_bins.h holds the definitions). wave64, no scratch, built with -ffp-contract=off.
//
//   pb_minmax_kernel     min / max over the finite positions of strided state rows (cloud_kernels.h's partial-and-ticket finish)
//   pb_key_kernel        (key, particle index) per row; the pairs then go through the stable radix sort (sort_kernels.h)
//   pb_block_kernel      launch 1 over the sorted pairs: per work-group of PB_BLOCK entries the number of runs that BEGIN in it
//                        and the aggregate of its last run's part inside it
//   pb_bins_kernel       launch 2: the same segmented scan again; the entry that ENDS a run writes the run's record, at the
//                        rank of the run's head (blocks_ahead over launch 1's counts). A run that began in an earlier work-group
//                        is completed from launch 1's partials by the whole work-group, 256 partials a step: nobody waits for
//                        anybody, no float atomics, and no thread looks at more than PB_BLOCK entries or n / PB_BLOCK / 256 partials
//                        whatever the distribution — a converged filter puts every particle into a handful of runs
//   pb_select_kernel     one work-group: bins with mass > 0, and top_k rounds of an arg-max by (mass descending, key ascending)
//
// An aggregate is {count, fp64 mass, largest weight, its particle index}; combine(earlier, later) keeps the EARLIER particle on
// a tie (pf::max()'s strict `<`: the sort is stable, so positions inside a run ascend with the particle index) and lets a NaN
// weight lead only where every weight is one. The order of the additions follows from the sorted pairs alone: the same data
// gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloud_kernels.h"
#include "particle_bins.h"
#pragma clang fp contract(off)

namespace mcl3dl
{
constexpr int PB_THREADS = 256;
constexpr int PB_PER_THREAD = 4;
constexpr int PB_BLOCK = PB_THREADS * PB_PER_THREAD;
constexpr int PB_SELECT_THREADS = 1024;

struct PbAgg
{
  double mass;
  float wmax;
  uint32_t idx;
  uint32_t count;  // 0: nothing (the identity of pb_combine)
};

__device__ inline PbAgg pb_none()
{
  return PbAgg{ 0.0, 0.f, 0u, 0u };
}

__device__ inline PbAgg pb_one(float w, uint32_t idx)
{
  return PbAgg{ static_cast<double>(w), w, idx, 1u };
}

// a before b in sorted order
// (by value and field by field: selects between registers, never between two objects' addresses)
__device__ inline PbAgg pb_combine(const PbAgg a, const PbAgg b)
{
  const bool no_a = a.count == 0u, no_b = b.count == 0u;
  const bool later = no_a || (!no_b && (b.wmax > a.wmax || (a.wmax != a.wmax && b.wmax == b.wmax)));
  const double sum = a.mass + b.mass;
  PbAgg r;
  r.mass = no_a ? b.mass : (no_b ? a.mass : sum);
  r.count = a.count + b.count;
  r.wmax = later ? b.wmax : a.wmax;
  r.idx = later ? b.idx : a.idx;
  return r;
}

__device__ inline PbAgg pb_shfl_up(const PbAgg a, int off)
{
  PbAgg r;
  r.mass = __shfl_up(a.mass, off, 64);
  r.wmax = __shfl_up(a.wmax, off, 64);
  r.idx = __shfl_up(a.idx, off, 64);
  r.count = __shfl_up(a.count, off, 64);
  return r;
}

__device__ inline PbAgg pb_shfl_down(const PbAgg a, int off)
{
  PbAgg r;
  r.mass = __shfl_down(a.mass, off, 64);
  r.wmax = __shfl_down(a.wmax, off, 64);
  r.idx = __shfl_down(a.idx, off, 64);
  r.count = __shfl_down(a.count, off, 64);
  return r;
}

// what launch 1 leaves per work-group
struct PbBlockOut
{
  uint32_t* heads;  // runs that begin in the work-group
  double* mass;     // the aggregate from the work-group's last head (its first entry when it has none) to its last entry
  float* wmax;
  uint32_t* idx;
  uint32_t* count;
};

// ---- min / max of the finite positions ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pb_minmax_kernel(const float* __restrict__ rows, long long stride, long long n, MinMaxOut mm)
{
  float mn[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, mx[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
  unsigned cnt = 0;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * 256)
  {
    const float* r = rows + i * stride;
    minmax_accumulate(make_float4(r[0], r[1], r[2], 0.f), mn, mx, cnt);
  }
  block_minmax_finish(mn, mx, cnt, mm);
}

// ---- keys -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pb_key_kernel(const float* __restrict__ rows, long long stride, long long n,
                                                     ParticleBinGrid g, const double* __restrict__ cs,
                                                     uint32_t* __restrict__ key, uint32_t* __restrict__ val)
{
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n)
    return;
  const float* r = rows + i * stride;
  const float pos[3] = { r[0], r[1], r[2] };
  const float rot[4] = { r[3], r[4], r[5], r[6] };
  key[i] = pb_finite3(pos[0], pos[1], pos[2]) ? pb_key(pos, rot, g, cs) : g.nonfinite_key;
  val[i] = static_cast<uint32_t>(i);
}

// ---- the segmented scan of one work-group ---------------------------------------------------------------------------------
// Thread t owns the sorted entries base + 4 t ... + 3 (entries at or behind n_f take no part). Afterwards, for each of them:
//   head[k]   the entry begins a run
//   tail[k]   the entry ends a run
//   incl[k]   the aggregate from the run's head — or from the work-group's first entry, if the run began before it — to the entry
//   open[k]   that run began before the work-group's first entry
struct PbScan
{
  bool head[PB_PER_THREAD], tail[PB_PER_THREAD], open[PB_PER_THREAD];
  PbAgg incl[PB_PER_THREAD];
  uint32_t n_heads;  // of this thread
};

__device__ inline void pb_block_scan(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                     const float* __restrict__ weight, long long n_f, PbScan& s)
{
  __shared__ PbAgg s_wave[PB_THREADS / 64];
  __shared__ int s_wave_flag[PB_THREADS / 64];
  const long long block_base = static_cast<long long>(blockIdx.x) * PB_BLOCK;
  const long long base = block_base + threadIdx.x * PB_PER_THREAD;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // the thread's four entries and the keys either side of them
  uint32_t k[PB_PER_THREAD + 2];
#pragma unroll
  for (int j = 0; j < PB_PER_THREAD + 2; ++j)
  {
    const long long i = base - 1 + j;
    k[j] = (i >= 0 && i < n_f) ? key[i] : 0u;
  }
  PbAgg run = pb_none();  // from the thread's last head, or its first entry, on
  bool flag = false;      // the thread holds a head
  s.n_heads = 0;
#pragma unroll
  for (int j = 0; j < PB_PER_THREAD; ++j)
  {
    const long long i = base + j;
    const bool live = i < n_f;
    s.head[j] = live && (i == 0 || k[j] != k[j + 1]);
    s.tail[j] = live && (i + 1 == n_f || k[j + 2] != k[j + 1]);
    PbAgg e = pb_none();
    if (live)
    {
      const uint32_t p = val[i];
      e = pb_one(weight[p], p);
    }
    run = s.head[j] ? e : pb_combine(run, e);
    flag = flag || s.head[j];
    s.incl[j] = run;
    s.open[j] = !flag;  // (so far: open inside the thread)
    s.n_heads += s.head[j] ? 1u : 0u;
  }
  // inclusive segmented scan of (flag, run) over the wavefront
  PbAgg inc = run;
  bool inc_flag = flag;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1)
  {
    const PbAgg o = pb_shfl_up(inc, off);
    const int of = __shfl_up(inc_flag ? 1 : 0, off, 64);
    if (lane >= off)
    {
      if (!inc_flag)
        inc = pb_combine(o, inc);
      inc_flag = inc_flag || of != 0;
    }
  }
  // what reaches this thread from the lanes in front of it
  PbAgg carry = pb_shfl_up(inc, 1);
  int carry_flag = __shfl_up(inc_flag ? 1 : 0, 1, 64);
  if (lane == 0)
  {
    carry = pb_none();
    carry_flag = 0;
  }
  __syncthreads();  // (s_wave may still be read by a previous call)
  if (lane == 63)
  {
    s_wave[w] = inc;
    s_wave_flag[w] = inc_flag ? 1 : 0;
  }
  __syncthreads();
  // ... and from the wavefronts in front of this one
  PbAgg before = pb_none();
  bool before_flag = false;
  for (int v = 0; v < w; ++v)
  {
    const PbAgg a = s_wave[v];
    const bool f = s_wave_flag[v] != 0;
    before = f ? a : pb_combine(before, a);
    before_flag = before_flag || f;
  }
  if (!carry_flag)
    carry = pb_combine(before, carry);
  const bool carry_open = !carry_flag && !before_flag;
#pragma unroll
  for (int j = 0; j < PB_PER_THREAD; ++j)
    if (s.open[j])  // no head in the thread up to this entry: the run comes in from the front
    {
      s.incl[j] = pb_combine(carry, s.incl[j]);
      s.open[j] = carry_open;
    }
}

// launch 1
__global__ __launch_bounds__(PB_THREADS) void pb_block_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                              const float* __restrict__ weight, long long n_f, PbBlockOut out)
{
  PbScan s;
  pb_block_scan(key, val, weight, n_f, s);
  uint32_t total;
  block_scan_excl(s.n_heads, total);
  if (threadIdx.x == PB_THREADS - 1)
  {
    // the last entry's inclusive aggregate; entries behind n_f are the identity, so it is the last live entry's
    const PbAgg a = s.incl[PB_PER_THREAD - 1];
    out.heads[blockIdx.x] = total;
    out.mass[blockIdx.x] = a.mass;
    out.wmax[blockIdx.x] = a.wmax;
    out.idx[blockIdx.x] = a.idx;
    out.count[blockIdx.x] = a.count;
  }
}

// one record per occupied bin, in ascending key order
struct PbBins
{
  uint32_t* key;
  uint32_t* count;
  uint32_t* leader;
  double* mass;
  unsigned long long* n_bins;  // written by the last work-group
};

// The part of this work-group's first run that lies in the work-groups in front of it: their partials from the nearest one
// that holds a head on, in sorted order. Called by every thread; the result is valid in thread 0.
__device__ inline PbAgg pb_run_before(const PbBlockOut& part)
{
  __shared__ PbAgg s_part[PB_THREADS / 64];
  __shared__ int s_found;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  PbAgg total = pb_none();
  for (long long hi = static_cast<long long>(blockIdx.x) - 1; hi >= 0; hi -= PB_THREADS)
  {
    // thread t looks at work-group hi - t: a higher thread holds an EARLIER partial
    const long long c = hi - threadIdx.x;
    const bool has_head = c >= 0 && part.heads[c] != 0u;
    if (threadIdx.x == 0)
      s_found = 0x7fffffff;
    __syncthreads();
    if (has_head)
      atomicMin(&s_found, static_cast<int>(threadIdx.x));
    __syncthreads();
    const int first = s_found;  // the nearest work-group with a head is hi - first
    PbAgg a = pb_none();
    if (c >= 0 && static_cast<int>(threadIdx.x) <= first)
      a = PbAgg{ part.mass[c], part.wmax[c], part.idx[c], part.count[c] };
    // ordered reduction: lane l ends up with lanes l ... 63, the higher (earlier) ones in front
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
    {
      const PbAgg o = pb_shfl_down(a, off);
      if (lane + off < 64)
        a = pb_combine(o, a);
    }
    if (lane == 0)
      s_part[w] = a;
    __syncthreads();
    if (threadIdx.x == 0)
    {
      PbAgg chunk = pb_none();
      for (int v = PB_THREADS / 64 - 1; v >= 0; --v)
        chunk = pb_combine(chunk, s_part[v]);
      total = pb_combine(chunk, total);
    }
    __syncthreads();  // (s_found, s_part are rewritten by the next step)
    if (first != 0x7fffffff)
      break;
  }
  return total;
}

// launch 2
__global__ __launch_bounds__(PB_THREADS) void pb_bins_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                             const float* __restrict__ weight, long long n_f, PbBlockOut part,
                                                             PbBins bins)
{
  __shared__ PbAgg s_before;
  PbScan s;
  pb_block_scan(key, val, weight, n_f, s);
  const uint32_t ahead = blocks_ahead(part.heads);
  uint32_t total;
  const uint32_t heads_before = ahead + block_scan_excl(s.n_heads, total);
  // does a run that began in an earlier work-group end here? (uniform over the work-group: every thread must take the same way)
  bool wants = false;
#pragma unroll
  for (int j = 0; j < PB_PER_THREAD; ++j)
    wants = wants || (s.tail[j] && s.open[j]);
  const bool any = __syncthreads_or(wants ? 1 : 0) != 0;
  if (any && blockIdx.x > 0)
  {
    const PbAgg before = pb_run_before(part);
    if (threadIdx.x == 0)
      s_before = before;
    __syncthreads();
  }
  const long long base = static_cast<long long>(blockIdx.x) * PB_BLOCK + threadIdx.x * PB_PER_THREAD;
  uint32_t heads = heads_before;
#pragma unroll
  for (int j = 0; j < PB_PER_THREAD; ++j)
  {
    heads += s.head[j] ? 1u : 0u;
    if (!s.tail[j])
      continue;
    PbAgg a = s.incl[j];
    if (s.open[j] && blockIdx.x > 0)
      a = pb_combine(s_before, a);
    // the run's rank: the heads up to and including its own, less one (its head lies at or before this entry)
    const uint32_t r = heads - 1u;
    bins.key[r] = key[base + j];
    bins.count[r] = a.count;
    bins.leader[r] = a.idx;
    bins.mass[r] = a.mass;
  }
  if (blockIdx.x + 1 == gridDim.x && threadIdx.x == 0)
    *bins.n_bins = static_cast<unsigned long long>(ahead) + total;
}

// ---- totals and the top K -------------------------------------------------------------------------------------------------
struct PbTop
{
  double mass;
  uint32_t key, count, leader, pad;
};

struct PbResult
{
  unsigned long long occupied, occupied_alive;
  uint32_t top_n, pad;
  PbTop top[PB_MAX_TOP_K];
};

// a ranks before b: more mass, the lower key on a tie (keys are distinct)
__device__ inline bool pb_ranks_before(double mass_a, uint32_t key_a, double mass_b, uint32_t key_b)
{
  return mass_a > mass_b || (mass_a == mass_b && key_a < key_b);
}

__global__ __launch_bounds__(PB_SELECT_THREADS) void pb_select_kernel(PbBins bins, int top_k, PbResult* __restrict__ out)
{
  __shared__ double s_mass[PB_SELECT_THREADS / 64];
  __shared__ uint32_t s_key[PB_SELECT_THREADS / 64];
  __shared__ long long s_at[PB_SELECT_THREADS / 64];
  __shared__ unsigned long long s_alive[PB_SELECT_THREADS / 64];
  __shared__ double s_last_mass;
  __shared__ uint32_t s_last_key;
  __shared__ int s_have_last;
  const long long n_bins = static_cast<long long>(*bins.n_bins);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long alive = 0;
  for (long long i = threadIdx.x; i < n_bins; i += PB_SELECT_THREADS)
    alive += bins.mass[i] > 0.0 ? 1ull : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    alive += __shfl_xor(alive, off, 64);
  if (lane == 0)
    s_alive[w] = alive;
  if (threadIdx.x == 0)
    s_have_last = 0;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    unsigned long long a = 0;
    for (int v = 0; v < PB_SELECT_THREADS / 64; ++v)
      a += s_alive[v];
    out->occupied = static_cast<unsigned long long>(n_bins);
    out->occupied_alive = a;
    out->pad = 0u;
  }
  uint32_t found = 0;
  for (int round = 0; round < top_k; ++round)
  {
    // the best record behind the one the previous round took
    const bool have_last = s_have_last != 0;
    const double last_mass = s_last_mass;
    const uint32_t last_key = s_last_key;
    double best_mass = 0.0;
    uint32_t best_key = 0u;
    long long best_at = -1;
    for (long long i = threadIdx.x; i < n_bins; i += PB_SELECT_THREADS)
    {
      const double m = bins.mass[i];
      const uint32_t k = bins.key[i];
      if (have_last && !pb_ranks_before(last_mass, last_key, m, k))
        continue;
      if (!have_last && m != m)
        continue;  // (a NaN mass ranks nowhere)
      if (best_at < 0 || pb_ranks_before(m, k, best_mass, best_key))
      {
        best_mass = m;
        best_key = k;
        best_at = i;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
      const double om = __shfl_xor(best_mass, off, 64);
      const uint32_t ok = __shfl_xor(best_key, off, 64);
      const long long oa = __shfl_xor(best_at, off, 64);
      if (oa >= 0 && (best_at < 0 || pb_ranks_before(om, ok, best_mass, best_key)))
      {
        best_mass = om;
        best_key = ok;
        best_at = oa;
      }
    }
    __syncthreads();  // (the previous round's s_last_* and s_mass have been read)
    if (lane == 0)
    {
      s_mass[w] = best_mass;
      s_key[w] = best_key;
      s_at[w] = best_at;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
      for (int v = 1; v < PB_SELECT_THREADS / 64; ++v)
        if (s_at[v] >= 0 && (best_at < 0 || pb_ranks_before(s_mass[v], s_key[v], best_mass, best_key)))
        {
          best_mass = s_mass[v];
          best_key = s_key[v];
          best_at = s_at[v];
        }
      if (best_at >= 0)
      {
        PbTop t;
        t.mass = best_mass;
        t.key = best_key;
        t.count = bins.count[best_at];
        t.leader = bins.leader[best_at];
        t.pad = 0u;
        out->top[round] = t;
        s_last_mass = best_mass;
        s_last_key = best_key;
        s_have_last = 1;
        ++found;
      }
      else
        s_have_last = 2;  // nothing is left: the remaining rounds find nothing either
    }
    __syncthreads();
    if (s_have_last == 2)
      break;
  }
  if (threadIdx.x == 0)
    out->top_n = found;
}
}  // namespace mcl3dl
