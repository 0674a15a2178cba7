// resample_prefix_kernels.h — pf::resample / resizeParticle (include/mcl_3dl/pf.h:187-225, 399-436) without the host between
// the weights and the plan: the accumulated probabilities by float_prefix.h's wavefront chain, pstep and the engine's
// initial_p formed behind it in the same launch, `pscan += pstep` by the constant-term chain, and the lower_bound search fed
// from the device record. The kernels of pf_kernels.h behind the search (walk, slot, apply) are the ones the three-call
// sequence launches.
//
// The record and what fills it compile for the host too (tests/cpp/float_prefix_emul.cpp).
#pragma once
#include "float_prefix.h"
#include "rng_polar.h"

namespace mcl3dl
{
// what the prefix kernel leaves behind the keys
struct ResampleRecord
{
  float pstep, initial_p;  // pf.h:198-199 / 411 (initial_p: mode 0 only, else 0)
  uint32_t state;          // the engine state behind the draw (mode 1: the one handed in)
  uint32_t ties;           // some i > 0 has !(key[i - 1] < key[i]): std::sort has tie groups to order
  float total;             // the last accumulated probability
};

// pstep = accum / particles_.size() (a size_t converted to float, one correctly rounded float division), and for mode 0
// initial_p = std::uniform_real_distribution<float>(0, pstep)(engine_): one engine call, canonical * (b - a) + a
FPREFIX_HD inline void resample_record_fill(float total, unsigned long long n_out, int mode, uint32_t state, bool ties,
                                            ResampleRecord* rec)
{
  rec->total = total;
  rec->pstep = total / static_cast<float>(n_out);
  rec->initial_p = 0.0f;
  if (mode == 0)
  {
    state = rng::minstd_next(state);
    rec->initial_p = rng::canonical(state) * (rec->pstep - 0.0f) + 0.0f;
  }
  rec->state = state;
  rec->ties = ties ? 1u : 0u;
}

#if defined(__HIPCC__)
// ONE wavefront: keys[i] = the accumulated probability of particle i, in particle order; the record behind them
__global__ __launch_bounds__(64) void resample_prefix_kernel(const float* __restrict__ weight, int n, int n_out, int mode,
                                                             uint32_t state, float* __restrict__ keys,
                                                             ResampleRecord* __restrict__ rec)
{
  const int lane = threadIdx.x;
  bool ties = false;
  const float total = fprefix_wave(weight, 0.0f, keys, n, lane, &ties);
  if (lane == 0)
  {
    ResampleRecord r;
    resample_record_fill(total, static_cast<unsigned long long>(n_out), mode, state, ties, &r);
    *rec = r;
  }
}

// ONE wavefront: pscan[i] = fl(pscan[i - 1] + pstep) (pf.h:421), pstep from the record
__global__ __launch_bounds__(64) void resample_pscan_kernel(const ResampleRecord* __restrict__ rec, int n_out,
                                                            float* __restrict__ pscan)
{
  bool ties = false;
  (void)fprefix_wave(nullptr, rec->pstep, pscan, n_out, threadIdx.x, &ties);
}

// the chain on its own (mcl3dl_hip_float_prefix)
__global__ __launch_bounds__(64) void float_prefix_kernel(const float* __restrict__ term /*or null*/, float constant, long long n,
                                                          float* __restrict__ out)
{
  bool ties = false;
  (void)fprefix_wave(term, constant, out, n, threadIdx.x, &ties);
}

// resample_lower_bound_kernel with pstep / initial_p read from the record instead of passed by the host
__global__ void resample_lower_bound_record_kernel(const float* __restrict__ keys, int n, const float* __restrict__ pscan,
                                                   const ResampleRecord* __restrict__ rec, int n_out,
                                                   uint32_t* __restrict__ it_out, uint32_t* __restrict__ last_valid)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out)
    return;
  const float p = pscan ? pscan[i] : rec->pstep * static_cast<float>(static_cast<unsigned long long>(i)) + rec->initial_p;
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
    atomicMax(last_valid, static_cast<uint32_t>(lo));
}
#endif
}  // namespace mcl3dl
