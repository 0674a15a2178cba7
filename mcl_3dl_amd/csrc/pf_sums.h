// pf_sums.h — the arithmetic of pf::ParticleFilter::measure (include/mcl_3dl/pf.h:252-279), stated once for the four kernels
// that run it: the split form and lik_pf_partial_kernel and pf_fused_kernel (pf_kernels.h), update_small_kernel
// (update_kernels.h). They give the same bits because they call the same functions in the same association; what a kernel
// keeps of its own is loads, stores, barriers and tickets.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"

#pragma clang fp contract(off)

namespace mcl3dl
{
// {sum w, sum w ln w, max ratio, -min ratio} of some particles; in memory, four consecutive doubles
struct PfSums
{
  double s, t, rmax, rneg;
};
// of no particle: match_ratio_max = 0, match_ratio_min = 1 (mcl_3dl.cpp:398-399)
__device__ inline PfSums pf_no_sums()
{
  return { 0.0, 0.0, 0.0, -1.0 };
}
__device__ inline PfSums pf_load(const double* p)
{
  return { p[0], p[1], p[2], p[3] };
}
__device__ inline void pf_store(double* p, const PfSums& v)
{
  p[0] = v.s;
  p[1] = v.t;
  p[2] = v.rmax;
  p[3] = v.rneg;
}

// w * (((1 * beam) * lik) * extra): the lambda's product (mcl_3dl.cpp:407-424) and pf.h:258. A factor the update does not have
// is passed as 1.0f (x * 1.0f is x in every bit).
__device__ inline float pf_weight(float w, float beam, float lik, float extra)
{
  float l = 1.0f;
  l *= beam;
  l *= lik;
  l = l * extra;
  return w * l;
}

// one particle's new weight: `sum += p.probability_` (pf.h:259) and its entropy term (0 ln 0 = 0)
__device__ inline void pf_add_weight(PfSums& a, float wn)
{
  a.s += static_cast<double>(wn);
  if (wn > 0.0f)
    a.t += static_cast<double>(wn) * log(static_cast<double>(wn));
}
// one particle's match ratio (mcl_3dl.cpp:417-420): the maximum, and the minimum as the maximum of the negated values
__device__ inline void pf_add_ratio(PfSums& a, float ratio)
{
  const double r = static_cast<double>(ratio);
  a.rmax = r > a.rmax ? r : a.rmax;
  a.rneg = -r > a.rneg ? -r : a.rneg;
}

// partial + partial: what the block combine and the strided reduction do with every partial they take
__device__ inline void pf_add_sums(PfSums& a, const PfSums& b)
{
  a.s += b.s;
  a.t += b.t;
  a.rmax = b.rmax > a.rmax ? b.rmax : a.rmax;
  a.rneg = b.rneg > a.rneg ? b.rneg : a.rneg;
}

// the lanes' sums -> the wavefront's, in lane 0
__device__ inline PfSums pf_wave_reduce(const PfSums& a)
{
  return { wave_sum(a.s), wave_sum(a.t), wave_max(a.rmax), wave_max(a.rneg) };
}

// A block's partial from its four wavefronts': 0 + w0 + w1 + w2 + w3, the maxima from wavefront 0's on. A wavefront the block
// does not have counts pf_no_sums(), what a wavefront without particles reduces to.
__device__ inline PfSums pf_block_combine(const PfSums* wv)
{
  PfSums b = { 0.0, 0.0, wv[0].rmax, wv[0].rneg };
#pragma unroll
  for (int k = 0; k < 4; ++k)
    pf_add_sums(b, wv[k]);
  return b;
}

// The sums of all blocks from the blocks' partials, by one wavefront (result in lane 0): lane l adds the blocks l, l + 64, ...
// in increasing order, then the wavefront reduction. load(k) = the partial of block k.
template <class Load>
__device__ inline PfSums pf_reduce_blocks(int n_blocks, int lane, Load load)
{
  PfSums a = pf_no_sums();
  for (int k = lane; k < n_blocks; k += 64)
    pf_add_sums(a, load(k));
  return pf_wave_reduce(a);
}

// The four statistics of an update: entropy ln S - T/S == -sum (w/S) ln (w/S) (NaN for a restored update), min ratio, max
// ratio, the restored flag (alive: S > 0 as a float, pf.h:262) — to the device array and to PfEmit's page-locked one (either
// may be null).
__device__ inline void pf_write_stats(const PfSums& tot, bool alive, float* stats4, float* emit_stats4)
{
  const double S = tot.s;
  const float st[4] = { alive ? static_cast<float>(log(S) - tot.t / S) : __builtin_nanf(""),
                        static_cast<float>(-tot.rneg), static_cast<float>(tot.rmax), alive ? 0.0f : 1.0f };
  for (int k = 0; k < 4; ++k)
  {
    if (stats4)
      stats4[k] = st[k];
    if (emit_stats4)
      emit_stats4[k] = st[k];
  }
}
}  // namespace mcl3dl
