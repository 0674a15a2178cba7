// pf_kernels.h — pf::ParticleFilter::measure (R1/R2) and the "next" rows: expectation / max / covariance, resampling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "beam_kernels.h"
#include "device_math.h"
#include "float_chain.h"
#include "motion_kernels.h"
#include "pf_sums.h"

#pragma clang fp contract(off)

namespace mcl3dl
{
// ---------------------------------------------------------------------------------------------------------
// pf::ParticleFilter::measure, include/mcl_3dl/pf.h:252-279  (+ the lambda's product, src/mcl_3dl.cpp:407-424)
// ---------------------------------------------------------------------------------------------------------
constexpr int PF_BLOCK = 256;

// The results of an update written a second time, into page-locked (device-mapped) host memory, by the kernel that produces
// the final weights — a host-buffer update then ends without a D2H copy (SURVEY.md 8d's region: "D2H of weights"). Any
// pointer may be null.
struct PfEmit
{
  float* stats4;
  float* w;
  float* lik;
  float* ratio;
  float* beam;
};

// The beam model's last step (beam_kernels.h: beam_score, as beam_finalize_kernel calls it) for the kernel that needs the score
// next, instead of a launch of its own in front of it (round 6): penalty != null — the score is formed from the count, written
// to beam_out, and the counter is ZEROED behind the read (the next update's beam kernel counts from 0 without a launch that
// clears: mcl3dl_hip_ctx::penalty_clean_n).
struct BeamCounts
{
  unsigned* penalty;     // [n] penalised rays per particle
  const float* pow_table;
  float beam_likelihood_min;
  float* beam_out;       // [n]
};
__device__ inline float beam_score_from_count(const BeamCounts& bc, int i)
{
  const float sb = beam_score(bc.pow_table, bc.penalty[i], bc.beam_likelihood_min);
  bc.penalty[i] = 0u;
  bc.beam_out[i] = sb;
  return sb;
}

// w_new = pf_weight(...); per-block partials (PfSums, pf_sums.h).
__global__ __launch_bounds__(PF_BLOCK) void pf_partial_kernel(const float* __restrict__ w, const float* __restrict__ lik,
                                                              const float* __restrict__ beam,
                                                              const float* __restrict__ extra,
                                                              const float* __restrict__ ratio, int n,
                                                              float* __restrict__ w_new,
                                                              double* __restrict__ block_partials, BeamCounts bc = BeamCounts{},
                                                              ImuGravity imu = ImuGravity{})
{
  PfSums a = pf_no_sums();
  for (int i = blockIdx.x * PF_BLOCK + threadIdx.x; i < n; i += gridDim.x * PF_BLOCK)
  {
    const float b = bc.penalty ? beam_score_from_count(bc, i) : beam ? beam[i] : 1.0f;
    const float lk = imu.state13 ? imu_gravity_likelihood(imu, i) : lik[i];  // (the IMU update: the likelihood formed here, lik == null)
    const float wn = pf_weight(w[i], b, lk, extra ? extra[i] : 1.0f);
    w_new[i] = wn;
    pf_add_weight(a, wn);
    if (ratio)
      pf_add_ratio(a, ratio[i]);
  }
  __shared__ PfSums sh[PF_BLOCK / 64];
  a = pf_wave_reduce(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
    sh[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    pf_store(block_partials + 4 * blockIdx.x, pf_block_combine(sh));
}

// lik_finalize_kernel + pf_partial_kernel as ONE launch (round 6; one GPU, the tiled likelihood kernel in front, at most
// 1024 x 256 particles — one per thread of pf_partial_kernel's grid). A work-group owns 64 consecutive particles (one wavefront
// of pf_partial_kernel's 256-thread blocks) with lik_finalize_kernel's own parallelism: its four wavefronts add up the eight
// tile slices of the per-tile partials (wavefront v: slices v and v + 4, every eighth tile in increasing order), the first one
// combines them in order — lik_finalize_kernel's association — and goes on with pf_sums.h's product, terms and wavefront
// reduction. What leaves is the WAVEFRONT partial of the 64 particles; pf_reduce_lanes (n_waves > 0) forms pf_partial_kernel's block
// partials from four of them with the same pf_block_combine. Same arithmetic in the same association as the two launches: the
// same bits (tests/test_gpu_pf_fused.py).
struct LikTiles
{
  const double* psum;    // [n_tiles][n]
  const unsigned* pcnt;  // [n_tiles][n]
  int n_tiles, n_s;
  float* lik_out;        // [n]
  float* ratio_out;      // [n]
  float* beam_fill;      // [n] set to 1 (an update without beam points), or null
  BeamCounts bc;         // the beam model's last step as well (penalty != null)
};
constexpr int LIK_TAIL_UNROLL = 16;  // tiles per wavefront of the unrolled form: up to 64 tiles (16 384 scan points)
__global__ __launch_bounds__(256) void lik_pf_partial_kernel(LikTiles lt, const float* __restrict__ w,
                                                             const float* __restrict__ beam, const float* __restrict__ extra,
                                                             int n, float* __restrict__ w_new,
                                                             double* __restrict__ wave_partials)
{
  __shared__ double s_a[8][64];
  __shared__ unsigned s_n[8][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * 64 + lane;
  // Every load a lane needs is issued before the first add that depends on one: the partials were written by other XCDs a moment
  // ago, so each wait is a round trip to memory, and a dozen of them one behind the other were most of this launch.
  const bool read_beam = !lt.bc.penalty && beam && !lt.beam_fill;
  float w_p = 0.0f, beam_p = 1.0f, extra_p = 1.0f;
  if (wave == 0 && p < n)
  {
    w_p = w[p];
    if (read_beam)
      beam_p = beam[p];
    if (extra)
      extra_p = extra[p];
  }
  double a0 = 0.0, a1 = 0.0;
  unsigned n0 = 0, n1 = 0;
  if (p < n)
  {
    const double* ps = lt.psum + p;
    const unsigned* pc = lt.pcnt + p;
    if (lt.n_tiles > 0 && lt.n_tiles <= 4 * LIK_TAIL_UNROLL)
    {
      // unrolled: tile wave + 4 j for every j, a tile past the end read as the last one (a line this lane has anyway) and not added
      double x[LIK_TAIL_UNROLL];
      unsigned c[LIK_TAIL_UNROLL];
#pragma unroll
      for (int j = 0; j < LIK_TAIL_UNROLL; ++j)
      {
        const int tl = min(wave + 4 * j, lt.n_tiles - 1);
        x[j] = ps[static_cast<size_t>(tl) * n];
        c[j] = pc[static_cast<size_t>(tl) * n];
      }
      // the loop's order: slice `wave` (even j) into a0 and slice `wave + 4` (odd j) into a1, tiles ascending
#pragma unroll
      for (int j = 0; j < LIK_TAIL_UNROLL; j += 2)
      {
        const bool h0 = wave + 4 * j < lt.n_tiles, h1 = wave + 4 * j + 4 < lt.n_tiles;
        a0 = h0 ? a0 + x[j] : a0;
        n0 = h0 ? n0 + c[j] : n0;
        a1 = h1 ? a1 + x[j + 1] : a1;
        n1 = h1 ? n1 + c[j + 1] : n1;
      }
    }
    else
    {
      int tl = wave;
      for (; tl + 4 < lt.n_tiles; tl += 8)  // slice `wave` and slice `wave + 4` side by side: two independent chains of loads
      {
        const double x0 = ps[static_cast<size_t>(tl) * n], x1 = ps[static_cast<size_t>(tl + 4) * n];
        const unsigned c0 = pc[static_cast<size_t>(tl) * n], c1 = pc[static_cast<size_t>(tl + 4) * n];
        a0 += x0;
        a1 += x1;
        n0 += c0;
        n1 += c1;
      }
      if (tl < lt.n_tiles)
      {
        a0 += ps[static_cast<size_t>(tl) * n];
        n0 += pc[static_cast<size_t>(tl) * n];
      }
    }
  }
  s_a[wave][lane] = a0;
  s_a[wave + 4][lane] = a1;
  s_n[wave][lane] = n0;
  s_n[wave + 4][lane] = n1;
  __syncthreads();
  if (wave != 0)
    return;
  PfSums sums = pf_no_sums();
  if (p < n)
  {
    double a = a0;
    unsigned cnt = n0;
#pragma unroll
    for (int k = 1; k < 8; ++k)
    {
      a += s_a[k][lane];
      cnt += s_n[k][lane];
    }
    const float lk = static_cast<float>(a);
    const float r32 = static_cast<float>(cnt) / static_cast<float>(lt.n_s);
    lt.lik_out[p] = lk;
    lt.ratio_out[p] = r32;
    if (lt.beam_fill)
      lt.beam_fill[p] = 1.0f;
    // (beam_p is 1 for an update without beam points: what pf_partial_kernel reads back from the array filled with ones)
    const float wn = pf_weight(w_p, lt.bc.penalty ? beam_score_from_count(lt.bc, p) : beam_p, lk, extra_p);
    w_new[p] = wn;
    pf_add_weight(sums, wn);
    pf_add_ratio(sums, r32);
  }
  sums = pf_wave_reduce(sums);
  if (lane == 0)
    pf_store(wave_partials + 4 * blockIdx.x, sums);
}

// Fixed-order reduction of the block partials (deterministic run to run). The result is written in the layout the
// update's single all-reduce(SUM) needs (mcl_3dl_amd/distributed.py): [0] sum w, [1] sum w ln w, then per rank r the pair
// [2+2r] max ratio, [3+2r] -min ratio — this rank fills its own pair and zeroes the others, so that after the SUM every
// rank holds every rank's pair. world == 1 degenerates to the plain 4 doubles.
// n_waves > 0: `block_partials` holds lik_pf_partial_kernel's n_waves WAVEFRONT partials instead (block k = wavefronts 4 k .. 4 k + 3,
// every one of them loaded before pf_block_combine's first add).
__device__ inline PfSums pf_reduce_lanes(const double* __restrict__ block_partials, int n_blocks, int n_waves, int lane)
{
  return pf_reduce_blocks(n_blocks, lane, [&](int k) {
    if (n_waves <= 0)
      return pf_load(block_partials + 4 * k);
    const double* wp = block_partials + 16 * static_cast<size_t>(k);
    PfSums wv[4] = { pf_load(wp), pf_no_sums(), pf_no_sums(), pf_no_sums() };
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (4 * k + j < n_waves)
        wv[j] = pf_load(wp + 4 * j);
    return pf_block_combine(wv);
  });
}

__global__ __launch_bounds__(64) void pf_reduce_kernel(const double* __restrict__ block_partials, int n_blocks, int rank,
                                                       int world, double* __restrict__ packed, int n_waves = 0)
{
  const PfSums a = pf_reduce_lanes(block_partials, n_blocks, n_waves, threadIdx.x);
  if (threadIdx.x == 0)
  {
    packed[0] = a.s;
    packed[1] = a.t;
    for (int r = 0; r < world; ++r)
    {
      packed[2 + 2 * r] = (r == rank) ? a.rmax : 0.0;
      packed[3 + 2 * r] = (r == rank) ? a.rneg : 0.0;
    }
  }
}

// pf::measure's `sum += p.probability_` (pf.h:255-260) as the reference runs it — a float recurrence in particle order — behind
// pf_partial / pf_reduce: the result replaces the fp64 tree sum in packed[0] so that pf_apply_kernel divides by exactly the
// reference's float. One work-group: 256 lanes stage 4096 weights at a time in LDS (coalesced), the first wavefront runs
// the recurrence over them (float_chain.h: 256 terms a pass instead of one), carrying the sum from chunk to chunk.
__global__ __launch_bounds__(256) void pf_strict_sum_kernel(const float* __restrict__ w_new, int n,
                                                            double* __restrict__ packed)
{
  __shared__ __attribute__((aligned(16))) float buf[4096 + 4];
  if (blockIdx.x != 0)
    return;
  float sum = 0.0f;
  for (int base = 0; base < n; base += 4096)
  {
    const int m = min(4096, n - base), m4 = chain_row_floats(m);
    for (int j = threadIdx.x; j < m4; j += 256)
      buf[j] = j < m ? w_new[base + j] : 0.0f;
    __syncthreads();
    if (threadIdx.x < 64)
      sum = seq_sum_wave(buf, m, static_cast<int>(threadIdx.x), sum);
    __syncthreads();
  }
  if (threadIdx.x == 0)
    packed[0] = static_cast<double>(sum);
}

// Normalise (pf.h:262-272) or restore (pf.h:274-278); the statistics: pf_write_stats.
// `packed` is the (all-reduced) vector described above.
// emit (+ the device arrays its lik / ratio / beam copies come from): see PfEmit.
// partials != null (one GPU, world == 1): EVERY work-group runs pf_reduce_lanes itself (first wavefront) instead of reading
// `packed` behind a launch of its own; work-group 0 also leaves the four sums in packed_w.
__global__ __launch_bounds__(PF_BLOCK) void pf_apply_kernel(float* __restrict__ w, const float* __restrict__ w_new,
                                                            int n, int world, const double* __restrict__ packed_in,
                                                            float* __restrict__ stats4, PfEmit emit = PfEmit{},
                                                            const float* __restrict__ lik = nullptr,
                                                            const float* __restrict__ ratio = nullptr,
                                                            const float* __restrict__ beam = nullptr,
                                                            const double* __restrict__ partials = nullptr, int n_blocks = 0,
                                                            int n_waves = 0, double* __restrict__ packed_w = nullptr)
{
  __shared__ double s_tot[4];
  const double* packed = packed_in;
  // a thread's first element (its only one when the grid covers n): read before the reduction and its barrier, not behind them
  const int i0 = blockIdx.x * PF_BLOCK + threadIdx.x;
  const bool emits = emit.lik || emit.ratio || emit.beam;
  float wn0 = 0.0f, lik0 = 0.0f, ratio0 = 0.0f, beam0 = 0.0f;
  if (i0 < n)
  {
    wn0 = w_new[i0];
    if (emit.lik)
      lik0 = lik[i0];
    if (emit.ratio)
      ratio0 = ratio[i0];
    if (emit.beam)
      beam0 = beam[i0];
  }
  if (partials)
  {
    if (threadIdx.x < 64)
    {
      const PfSums a = pf_reduce_lanes(partials, n_blocks, n_waves, threadIdx.x);
      if (threadIdx.x == 0)
      {
        pf_store(s_tot, a);
        if (blockIdx.x == 0 && packed_w)
          pf_store(packed_w, a);
      }
    }
    __syncthreads();
    packed = s_tot;
  }
  const double S = packed[0];
  const float sum_f = static_cast<float>(S);
  const bool alive = sum_f > 0.0f;
  if (alive)
  {
    for (int i = i0; i < n; i += gridDim.x * PF_BLOCK)
    {
      const float wv = (i == i0 ? wn0 : w_new[i]) / sum_f;
      w[i] = wv;
      if (emit.w)
        emit.w[i] = wv;
    }
  }
  else if (emit.w)
  {
    for (int i = blockIdx.x * PF_BLOCK + threadIdx.x; i < n; i += gridDim.x * PF_BLOCK)
      emit.w[i] = w[i];
  }
  if (emits)
    for (int i = i0; i < n; i += gridDim.x * PF_BLOCK)
    {
      if (emit.lik)
        emit.lik[i] = i == i0 ? lik0 : lik[i];
      if (emit.ratio)
        emit.ratio[i] = i == i0 ? ratio0 : ratio[i];
      if (emit.beam)
        emit.beam[i] = i == i0 ? beam0 : beam[i];
    }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (stats4 || emit.stats4))
  {
    // every rank's slot holds a value in [0,1] resp. [-1,0] (0 in both for a rank whose shard saw no ratios is impossible:
    // an empty shard reports max 0 / -min -1); the maxima over the slots are the global max ratio and -min ratio
    double rmax = packed[2], rneg = packed[3];
    for (int r = 1; r < world; ++r)
    {
      rmax = packed[2 + 2 * r] > rmax ? packed[2 + 2 * r] : rmax;
      rneg = packed[3 + 2 * r] > rneg ? packed[3 + 2 * r] : rneg;
    }
    pf_write_stats(PfSums{ S, packed[1], rmax, rneg }, alive, stats4, emit.stats4);
  }
}

// pf_partial_kernel -> pf_reduce_kernel -> pf_apply_kernel for ONE GPU and at most PF_FUSED_MAX particles, as a single
// work-group: the reference's real operating range (64 .. a few thousand particles) is launch-bound — three launches of
// a few microseconds each around ~1 us of work. The arithmetic is pf_sums.h's, called in the three kernels' association (the
// 256-thread "blocks" of pf_partial_kernel become quarters of this 1024-thread group that walk the same elements,
// pf_reduce_blocks runs in the first wavefront), so weights, entropy and ratio bounds are bit-identical to the split form.
// Measured and NOT kept (round 3, commit 5b571a1): pf_partial_kernel's grid with the reduce and the apply run by the last
// work-group behind an arrival-ticket tree, for 1024 < n <= 16 384 — bit-identical, and the group cost 24 us instead of
// 12.5 us at 4096 particles (49 at 16 384): three launches enqueued back to back cost 4.2 us each, less than two ticket
// levels plus one work-group's sc1 loads of every weight (profiles/r03z_pf_one_launch_ab.txt).
constexpr int PF_FUSED_MAX = 4096;

__global__ __launch_bounds__(1024) void pf_fused_kernel(float* __restrict__ w, const float* __restrict__ lik,
                                                        const float* __restrict__ beam, const float* __restrict__ extra,
                                                        const float* __restrict__ ratio, int n, float* __restrict__ w_new,
                                                        double* __restrict__ packed, float* __restrict__ stats4,
                                                        PfEmit emit = PfEmit{}, int float_order = 0, BeamCounts bc = BeamCounts{},
                                                        ImuGravity imu = ImuGravity{})
{
  // float_order: pf::measure's `sum += p.probability_` (pf.h:255-260) as the reference runs it — float, sequentially, in
  // particle order (float_chain.h) — instead of the fp64 tree: the weights are divided by exactly the reference's float
  __shared__ __attribute__((aligned(16))) float s_w[PF_FUSED_MAX + 4];
  __shared__ PfSums sh[16];             // per wavefront of the group
  __shared__ PfSums part[16];           // per virtual block (n <= 4096 -> at most 16 of them)
  __shared__ PfSums tot;
  const int nb = (n + PF_BLOCK - 1) / PF_BLOCK;  // pf_blocks(n) for n <= 4096
  const int q = threadIdx.x >> 8, tid = threadIdx.x & 255, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int vb0 = 0; vb0 < nb; vb0 += 4)
  {
    const int vb = vb0 + q;  // this quarter's virtual block
    PfSums a = pf_no_sums();
    const int i = vb * PF_BLOCK + tid;  // stride nb * PF_BLOCK >= n: one element per thread, like pf_partial_kernel
    if (vb < nb && i < n)
    {
      // (beam == bc.beam_out: the apply loop below re-reads what THIS thread writes here; the IMU update: no emit.lik)
      const float b = bc.penalty ? beam_score_from_count(bc, i) : beam ? beam[i] : 1.0f;
      const float lk = imu.state13 ? imu_gravity_likelihood(imu, i) : lik[i];
      const float wn = pf_weight(w[i], b, lk, extra ? extra[i] : 1.0f);
      w_new[i] = wn;
      if (float_order)
        s_w[i] = wn;
      pf_add_weight(a, wn);
      if (ratio)
        pf_add_ratio(a, ratio[i]);
    }
    a = pf_wave_reduce(a);
    if (lane == 0)
      sh[wave] = a;
    __syncthreads();
    if (tid == 0 && vb < nb)
      part[vb] = pf_block_combine(sh + 4 * q);
    __syncthreads();
  }
  if (wave == 0)
  {
    PfSums a = pf_reduce_blocks(nb, lane, [&](int k) { return part[k]; });
    if (float_order)
    {
      // (s_w[0 .. n) was written before the loop's last barrier; the padding of the last float4 here, by this wavefront)
      if (lane < chain_row_floats(n) - n)
        s_w[n + lane] = 0.0f;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      a.s = static_cast<double>(seq_sum_wave(s_w, n, lane));
    }
    if (lane == 0)
    {
      tot = a;
      pf_store(packed, a);
    }
  }
  __syncthreads();
  // pf_apply_kernel
  const double S = tot.s;
  const float sum_f = static_cast<float>(S);
  const bool alive = sum_f > 0.0f;
  for (int i = threadIdx.x; i < n; i += 1024)
  {
    float wv;
    if (alive)
    {
      wv = w_new[i] / sum_f;
      w[i] = wv;
    }
    else
      wv = w[i];
    if (emit.w)
      emit.w[i] = wv;
    if (emit.lik)
      emit.lik[i] = lik[i];
    if (emit.ratio)
      emit.ratio[i] = ratio ? ratio[i] : 0.f;
    if (emit.beam)
      emit.beam[i] = beam ? beam[i] : 1.f;
  }
  if (threadIdx.x == 0)
    pf_write_stats(tot, alive, stats4, emit.stats4);
}

// per-particle results of the two models -> page-locked host memory (mcl3dl_hip_measure_batch without a D2H copy)
__global__ __launch_bounds__(PF_BLOCK) void emit3_kernel(PfEmit emit, const float* __restrict__ lik, const float* __restrict__ ratio,
                                                         const float* __restrict__ beam, int n)
{
  for (int i = blockIdx.x * PF_BLOCK + threadIdx.x; i < n; i += gridDim.x * PF_BLOCK)
  {
    if (emit.lik)
      emit.lik[i] = lik[i];
    if (emit.ratio)
      emit.ratio[i] = ratio[i];
    if (emit.beam)
      emit.beam[i] = beam[i];
  }
}

// ---------------------------------------------------------------------------------------------------------
// "Next" row: the reductions that follow pf::measure in the node (src/mcl_3dl.cpp:451-452,706-709):
// pf::expectationBiased / max / maxBiased (include/mcl_3dl/pf.h:294-303,361-390) with ParticleWeightedMeanQuat
// (include/mcl_3dl/state_6dof.h:316-355), and pf::covariance (pf.h:304-360) with State6DOF::covElement (:162-184).
// Per-particle products are the reference's float expressions; the sums are fp64 trees (reference: float sequential).
// ---------------------------------------------------------------------------------------------------------
constexpr int MOM_N = 10;  // p_sum, pos[3], front[3], up[3]

struct ArgMax
{
  float v;
  int i;
};
__device__ inline ArgMax argmax_better(ArgMax a, ArgMax b)
{
  // pf.h:365-372: `if (max_probability < p.probability_)` -> the FIRST maximum wins
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

// probability_bias_ as pf::bias left it (pf.h:238-244): the caller's array, or 1 for every particle
struct BiasArray
{
  const float* bias;  // [n] or null
  __device__ float operator()(const float*, int i) const { return bias ? bias[i] : 1.0f; }
};

// The moments pass over one shard; Bias(pose of particle i, i) = probability_bias_ of that particle (BiasArray, or formed from
// the pose on the spot: landmark_kernels.h).
template <class Bias>
__device__ __forceinline__ void pf_moments_body(const float* __restrict__ pose7, const float* __restrict__ w, const Bias& bias,
                                                int n, double* __restrict__ block_mom /*[grid][MOM_N]*/,
                                                ArgMax* __restrict__ block_arg /*[grid][2]*/)
{
  double m[MOM_N];
#pragma unroll
  for (int k = 0; k < MOM_N; ++k)
    m[k] = 0.0;
  ArgMax am = { -1.0f, 0x7fffffff }, ab = { -1.0f, 0x7fffffff };
  bool first = true;
  for (int i = blockIdx.x * PF_BLOCK + threadIdx.x; i < n; i += gridDim.x * PF_BLOCK)
  {
    const float* ps = pose7 + 7 * static_cast<size_t>(i);
    const float prob = w[i] * bias(ps, i);  // pf.h:300
    const Quat rot = { ps[3], ps[4], ps[5], ps[6] };
    const Vec3f front = vscale(qrot(rot, Vec3f{ 1.0f, 0.0f, 0.0f }), prob);  // state_6dof.h:337-338
    const Vec3f up = vscale(qrot(rot, Vec3f{ 0.0f, 0.0f, 1.0f }), prob);
    m[0] += static_cast<double>(prob);
    m[1] += static_cast<double>(ps[0] * prob);  // e_.pos_ += e1.pos_ * prob, :335
    m[2] += static_cast<double>(ps[1] * prob);
    m[3] += static_cast<double>(ps[2] * prob);
    m[4] += static_cast<double>(front.x);
    m[5] += static_cast<double>(front.y);
    m[6] += static_cast<double>(front.z);
    m[7] += static_cast<double>(up.x);
    m[8] += static_cast<double>(up.y);
    m[9] += static_cast<double>(up.z);
    const ArgMax cm = { w[i], i }, cb = { prob, i };
    am = first ? cm : argmax_better(am, cm);
    ab = first ? cb : argmax_better(ab, cb);
    first = false;
  }
  __shared__ double sh[MOM_N][PF_BLOCK / 64];
  __shared__ ArgMax sa[2][PF_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < MOM_N; ++k)
  {
    const double s = wave_sum(m[k]);
    if (lane == 0)
      sh[k][wave] = s;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
  {
    ArgMax o1 = { __shfl_down(am.v, off, 64), __shfl_down(am.i, off, 64) };
    ArgMax o2 = { __shfl_down(ab.v, off, 64), __shfl_down(ab.i, off, 64) };
    am = argmax_better(am, o1);
    ab = argmax_better(ab, o2);
  }
  if (lane == 0)
  {
    sa[0][wave] = am;
    sa[1][wave] = ab;
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    for (int k = 0; k < MOM_N; ++k)
    {
      double s = 0;
      for (int q = 0; q < PF_BLOCK / 64; ++q)
        s += sh[k][q];
      block_mom[MOM_N * blockIdx.x + k] = s;
    }
    ArgMax a = sa[0][0], b = sa[1][0];
    for (int q = 1; q < PF_BLOCK / 64; ++q)
    {
      a = argmax_better(a, sa[0][q]);
      b = argmax_better(b, sa[1][q]);
    }
    block_arg[2 * blockIdx.x + 0] = a;
    block_arg[2 * blockIdx.x + 1] = b;
  }
}

__global__ __launch_bounds__(PF_BLOCK) void pf_moments_kernel(const float* __restrict__ pose7,
                                                              const float* __restrict__ w,
                                                              const float* __restrict__ bias, int n,
                                                              double* __restrict__ block_mom /*[grid][MOM_N]*/,
                                                              ArgMax* __restrict__ block_arg /*[grid][2]*/)
{
  pf_moments_body(pose7, w, BiasArray{ bias }, n, block_mom, block_arg);
}

__global__ __launch_bounds__(64) void pf_moments_reduce_kernel(const double* __restrict__ block_mom,
                                                               const ArgMax* __restrict__ block_arg, int n_blocks,
                                                               double* __restrict__ out_mom /*[MOM_N]*/,
                                                               int* __restrict__ out_arg /*[2]*/,
                                                               double* __restrict__ out16 /*or null: shard record*/)
{
  if (threadIdx.x < MOM_N)
  {
    double s = 0;
    for (int b = 0; b < n_blocks; ++b)  // fixed order
      s += block_mom[MOM_N * b + threadIdx.x];
    out_mom[threadIdx.x] = s;
    if (out16)
      out16[threadIdx.x] = s;
  }
  if (threadIdx.x == 32 || threadIdx.x == 33)
  {
    const int which = threadIdx.x - 32;
    ArgMax a = block_arg[which];
    for (int b = 1; b < n_blocks; ++b)
      a = argmax_better(a, block_arg[2 * b + which]);
    out_arg[which] = a.i;
    if (out16)
    {
      // {10: max weight, 11: its index in this shard, 12: max biased weight, 13: its index, 14-15: 0}
      out16[MOM_N + 2 * which] = static_cast<double>(a.v);
      out16[MOM_N + 2 * which + 1] = static_cast<double>(a.i);
      out16[14 + which] = 0.0;
    }
  }
}

// Quat::getRPY, include/mcl_3dl/quat.h:188-203 (float storage, double intermediates; device atan2f / asinf)
struct RpyTerms
{
  float t0, t1, t2, t3, t4;
};
__host__ __device__ inline RpyTerms quat_rpy_terms(Quat q)
{
  const float ysq = q.y * q.y;
  RpyTerms t;
  t.t0 = static_cast<float>(-2.0 * (ysq + q.z * q.z) + 1.0);
  t.t1 = static_cast<float>(+2.0 * (q.x * q.y + q.w * q.z));
  const double t2d = -2.0 * (q.x * q.z - q.w * q.y);
  t.t2 = static_cast<float>(t2d > 1.0 ? 1.0 : (t2d < -1.0 ? -1.0 : t2d));
  t.t3 = static_cast<float>(+2.0 * (q.y * q.z + q.w * q.x));
  t.t4 = static_cast<float>(-2.0 * (q.x * q.x + ysq) + 1.0);
  return t;
}
__host__ __device__ inline Vec3f quat_get_rpy(Quat q)
{
  const RpyTerms t = quat_rpy_terms(q);
  return { atan2f(t.t3, t.t4), asinf(t.t2), atan2f(t.t1, t.t0) };
}

constexpr int COV_N = 22;  // 21 upper-triangular sums + p_sum

// subset == nullptr: particles 0..n-1; else the n indices the caller drew (pf.h:322-336 shuffles them with its own RNG).
// WINDOW: pose7 / w hold the particles [window_lo, window_lo + window_n) of a sharded set and the list names particles of the
// whole set: an entry outside the window contributes nothing and keeps its place in the list, so every entry is summed by the
// lane and in the turn that the unwindowed kernel gives it.
template <bool WINDOW>
__device__ __forceinline__ void pf_covariance_body(const float* __restrict__ pose7, const float* __restrict__ w,
                                                   const uint32_t* __restrict__ subset, int n, uint32_t window_lo,
                                                   uint32_t window_n, float e0, float e1, float e2, Vec3f exp_rpy,
                                                   double* __restrict__ block_cov /*[grid][COV_N]*/)
{
  double acc[COV_N];
#pragma unroll
  for (int k = 0; k < COV_N; ++k)
    acc[k] = 0.0;
  for (int t = blockIdx.x * PF_BLOCK + threadIdx.x; t < n; t += gridDim.x * PF_BLOCK)
  {
    size_t i = subset ? subset[t] : static_cast<size_t>(t);
    if (WINDOW)
    {
      if (i < window_lo || i - window_lo >= window_n)
        continue;
      i -= window_lo;
    }
    const float* ps = pose7 + 7 * i;
    const float prob = w[i];
    const Vec3f rpy = quat_get_rpy(Quat{ ps[3], ps[4], ps[5], ps[6] });
    float d[6] = { ps[0] - e0, ps[1] - e1, ps[2] - e2, rpy.x - exp_rpy.x, rpy.y - exp_rpy.y, rpy.z - exp_rpy.z };
#pragma unroll
    for (int a = 3; a < 6; ++a)  // covElement, state_6dof.h:175-179
    {
      while (d[a] > M_PI)
        d[a] = static_cast<float>(d[a] - 2 * M_PI);
      while (d[a] < -M_PI)
        d[a] = static_cast<float>(d[a] + 2 * M_PI);
    }
    int idx = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int k = j; k < 6; ++k)
      {
        float val = 1.0f;
        val *= d[j];
        val *= d[k];
        acc[idx++] += static_cast<double>(val * prob);  // pf.h:347
      }
    acc[21] += static_cast<double>(prob);
  }
  __shared__ double sh[COV_N][PF_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < COV_N; ++k)
  {
    const double s = wave_sum(acc[k]);
    if (lane == 0)
      sh[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x < COV_N)
  {
    double s = 0;
    for (int q = 0; q < PF_BLOCK / 64; ++q)
      s += sh[threadIdx.x][q];
    block_cov[COV_N * blockIdx.x + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(PF_BLOCK) void pf_covariance_kernel(const float* __restrict__ pose7,
                                                                 const float* __restrict__ w,
                                                                 const uint32_t* __restrict__ subset, int n,
                                                                 float e0, float e1, float e2, Vec3f exp_rpy,
                                                                 double* __restrict__ block_cov /*[grid][COV_N]*/)
{
  pf_covariance_body<false>(pose7, w, subset, n, 0u, 0u, e0, e1, e2, exp_rpy, block_cov);
}

// the sampled covariance of a device group (api_shuffle.inl): one shard's share of a list over the whole particle set
__global__ __launch_bounds__(PF_BLOCK) void pf_covariance_window_kernel(const float* __restrict__ pose7,
                                                                        const float* __restrict__ w,
                                                                        const uint32_t* __restrict__ subset, int n,
                                                                        uint32_t window_lo, uint32_t window_n, float e0,
                                                                        float e1, float e2, Vec3f exp_rpy,
                                                                        double* __restrict__ block_cov /*[grid][COV_N]*/)
{
  pf_covariance_body<true>(pose7, w, subset, n, window_lo, window_n, e0, e1, e2, exp_rpy, block_cov);
}

__global__ __launch_bounds__(64) void pf_covariance_reduce_kernel(const double* __restrict__ block_cov, int n_blocks,
                                                                  double* __restrict__ out_cov /*[COV_N]*/)
{
  if (threadIdx.x < COV_N)
  {
    double s = 0;
    for (int b = 0; b < n_blocks; ++b)
      s += block_cov[COV_N * b + threadIdx.x];
    out_cov[threadIdx.x] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------
// "Next" row: pf::ParticleFilter::resample / resizeParticle (include/mcl_3dl/pf.h:187-225, 399-436).
// libstdc++'s std::sort of the tie groups stays on the host (api_resample.inl), and so do the float prefix sums of the
// three-call form (resample_prefix_kernels.h runs them on a wavefront); the device does the n_out independent
// std::lower_bound searches, the it/it_prev walk as a neighbour comparison + scan, and the gather of the 13-dof states with
// State6DOF::operator+ / normalize() for the duplicated ones.
// ---------------------------------------------------------------------------------------------------------
__global__ void resample_lower_bound_kernel(const float* __restrict__ keys, int n, const float* __restrict__ pscan,
                                            float pstep, float initial_p, int n_out, uint32_t* __restrict__ it_out,
                                            uint32_t* __restrict__ last_valid)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out)
    return;
  // resample: pscan = pstep * i + initial_p with i a size_t converted to float (pf.h:209); resizeParticle: the host's
  // running sum
  const float p = pscan ? pscan[i] : pstep * static_cast<float>(static_cast<unsigned long long>(i)) + initial_p;
  int lo = 0, len = n;  // std::lower_bound with Particle::operator< (pf.h:104-107): first key with !(key < p)
  while (len > 0)
  {
    const int half = len >> 1;
    if (keys[lo + half] < p)
    {
      lo += half + 1;
      len -= half + 1;
    }
    else
      len = half;
  }
  it_out[i] = static_cast<uint32_t>(lo);
  if (lo < n)
    atomicMax(last_valid, static_cast<uint32_t>(lo));  // = it_prev once the scan position runs past the last key
}

// The it / it_prev walk of pf.h:204-223 (resample) and :414-434 (resizeParticle) for non-decreasing search results:
// slot i copies particles_dup_[it[i]]; it is a duplicate (gets noise) when it[i] equals the previous slot's result
// (it_prev starts at begin(), so slot 0 is a duplicate when it lands on element 0); once it[i] == n every remaining slot
// copies the last element found before the end and nothing else changes (`continue`, :212-216).
__global__ void resample_walk_kernel(const uint32_t* __restrict__ it, int n, const uint32_t* __restrict__ order /*or null*/,
                                     int mode, int n_out, uint32_t* __restrict__ source, uint32_t* __restrict__ dup_flag)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out)
    return;
  const uint32_t cur = it[i];
  uint32_t pick, dup = 0u;
  if (cur >= static_cast<uint32_t>(n))
    pick = it[n_out];  // last search result below n (0 = begin() if there was none)
  else
  {
    pick = cur;
    const uint32_t prev = i ? it[i - 1] : 0u;
    dup = (mode == 0 && cur == prev) ? 1u : 0u;
  }
  source[i] = order ? order[pick] : pick;
  dup_flag[i] = dup;
}

// noise slot of every duplicated output slot = its rank among the duplicates (exclusive scan of the flags)
__global__ void resample_slot_kernel(const uint32_t* __restrict__ scanned, int n_out, uint32_t* __restrict__ slot_inout,
                                     uint8_t* __restrict__ dup8)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out)
    return;
  const uint32_t flag = slot_inout[i];  // the un-scanned flag was parked here
  slot_inout[i] = flag ? scanned[i] : 0xffffffffu;
  if (dup8)
    dup8[i] = static_cast<uint8_t>(flag);
}

// slot i receives the state of particle source[i]; duplicated picks get `state + noise` (State6DOF::operator+,
// state_6dof.h:248-260: components 0-2 and 7-12 add, rot = noise.rot * state.rot) followed by normalize() (:150-153).
__global__ void resample_apply_kernel(const float* __restrict__ state_in, const uint32_t* __restrict__ source,
                                      const uint32_t* __restrict__ noise_slot /* 0xffffffff = not duplicated */,
                                      const float* __restrict__ noise13, int n_out, float* __restrict__ state_out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out)
    return;
  const float* s = state_in + 13 * static_cast<size_t>(source[i]);
  float* o = state_out + 13 * static_cast<size_t>(i);
  const uint32_t slot = noise_slot[i];
  if (slot == 0xffffffffu)
  {
#pragma unroll
    for (int k = 0; k < 13; ++k)
      o[k] = s[k];
    return;
  }
  const Quat r = qnormalized(state6dof_plus(s, noise13 + 13 * static_cast<size_t>(slot), o));
  o[3] = r.x;
  o[4] = r.y;
  o[5] = r.z;
  o[6] = r.w;
}
}  // namespace mcl3dl
