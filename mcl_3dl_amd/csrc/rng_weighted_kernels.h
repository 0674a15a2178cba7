// rng_weighted_kernels.h — the normal-weighted sampler's draw on the device (rng_weighted.h holds the restatement and the steps,
// double_chain.h the cumulative recurrence; host side: api_sampler.inl).
//
//   weighted_cumulative_kernel   ONE wavefront: cum[i] = w[i] + cum[i - 1] with the serial loop's bits (dchain_prefix_wave)
//   weighted_fill_kernel         w[i] = v: the weights of a cloud in which nobody has a neighbour
//   weighted_iota_kernel         idx[i] = i: a cloud of at most `num` points is copied whole, in its own order
//   weighted_single_kernel       ONE work-group, no host round: up to two segments (cloud, count) back to back on one stream.
//                                Per segment passes of 256 lanes x 4 attempts — draw + lower_bound + atomicMin into the cloud's
//                                first_attempt words (global), new flags, a work-group scan, the inserted ids into LDS — until
//                                `num` ids are there, then the container's order phase by phase in LDS, the ids written in that
//                                order. The next segment continues behind the last attempt MADE; the engine state behind the last
//                                attempt of all and the attempt count go to result[].
//   weighted_draw / flag / emit  the general form, one launch per step over global buffers, any grid (the scans between them:
//   weighted_phase_* kernels     the cloud path's device_exclusive_scan_ws)
#pragma once
#include <hip/hip_runtime.h>

#include "double_chain.h"
#include "rng_weighted.h"

namespace mcl3dl
{
namespace rng
{
__global__ __launch_bounds__(64) void weighted_cumulative_kernel(const double* __restrict__ w, double* __restrict__ cum, long long n)
{
  dchain_prefix_wave(w, cum, n, static_cast<int>(threadIdx.x));
}

__global__ __launch_bounds__(256) void weighted_fill_kernel(double* __restrict__ w, long long n, double v)
{
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n)
    w[i] = v;
}

__global__ __launch_bounds__(256) void weighted_iota_kernel(uint32_t* __restrict__ idx, uint32_t n)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n)
    idx[i] = i;
}

// in-place exclusive scan of data[0 .. n) in LDS by the work-group; part: GROUP_THREADS words. Barriers inside, one in front
// is the caller's.
__device__ inline void weighted_group_scan(uint32_t* data, uint32_t n, uint32_t* part)
{
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + GROUP_THREADS - 1u) / GROUP_THREADS;
  const uint32_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  uint32_t sum = 0u;
  for (uint32_t i = lo; i < hi; ++i)
    sum += data[i];
  part[tid] = sum;
  __syncthreads();
  if (tid < 64u)
  {
    // four consecutive partials per lane of the first wavefront
    const uint32_t a = part[4u * tid], b = part[4u * tid + 1u], c = part[4u * tid + 2u], d = part[4u * tid + 3u];
    uint32_t v = a + b + c + d;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1)
    {
      const uint32_t o = __shfl_up(v, s);
      v = static_cast<int>(tid) >= s ? v + o : v;
    }
    const uint32_t ex = v - (a + b + c + d);
    part[4u * tid] = ex;
    part[4u * tid + 1u] = ex + a;
    part[4u * tid + 2u] = ex + a + b;
    part[4u * tid + 3u] = ex + a + b + c;
  }
  __syncthreads();
  uint32_t run = part[tid];
  for (uint32_t i = lo; i < hi; ++i)
  {
    const uint32_t v = data[i];
    data[i] = run;
    run += v;
  }
  __syncthreads();
}

struct WeightedSegment
{
  WeightedCloud cloud;
  uint32_t num;   // ids to draw, 0 < num < cloud.n and num <= WEIGHTED_SINGLE_MAX; 0: nothing is drawn, the stream does not move
  uint32_t* out;  // num ids in the container's iteration order
};

// result[0] = the engine state behind the last attempt made (x0 if nothing was drawn; 0 = the pass guard tripped),
// result[1], result[2] = the attempts segment 0 and segment 1 made
__global__ __launch_bounds__(GROUP_THREADS) void weighted_single_kernel(uint32_t x0, const uint32_t* __restrict__ table,
                                                                        WeightedSegment seg0, WeightedSegment seg1,
                                                                        uint32_t* __restrict__ result)
{
  constexpr uint32_t CAP = WEIGHTED_SINGLE_MAX + 1u;
  __shared__ uint32_t s_ins[CAP], s_cur[CAP], s_next[CAP], s_head[CAP], s_link[CAP], s_first_of[CAP], s_later[CAP], s_size[CAP + 1u];
  __shared__ uint32_t s_part[GROUP_THREADS];
  __shared__ uint32_t s_result[2];  // {state behind the num-th new attempt or 0, attempts made}
  static_assert(WEIGHTED_PASS + 1u <= CAP + 1u, "a pass's flags live in s_size, its ids in s_link");
  const uint32_t tid = threadIdx.x;
  uint32_t x = x0;  // uniform: the state the next pass (or segment) starts from
  for (int s = 0; s < 2; ++s)
  {
    const WeightedSegment sg = s ? seg1 : seg0;
    uint32_t made = 0u;
    if (sg.num != 0u)
    {
      uint32_t have = 0u;
      if (tid == 0u)
        s_result[0] = 0u;
      __syncthreads();
      for (uint32_t pass = 0u; have < sg.num; ++pass)
      {
        if (pass >= (1u << 21))
        {
          x = 0u;  // (2^31 attempts without `num` ids: not with weights the host admits)
          break;
        }
        uint32_t* att_id = s_link;
        uint32_t* flag = s_size;
        weighted_step_draw(tid, GROUP_THREADS, x, table, sg.cloud, made, WEIGHTED_PASS, att_id);
        __threadfence();  // the atomics have landed (device scope) before anyone reads the words back
        __syncthreads();
        weighted_step_flag(tid, GROUP_THREADS, sg.cloud, made, WEIGHTED_PASS, att_id, flag);
        __syncthreads();
        weighted_group_scan(flag, WEIGHTED_PASS + 1u, s_part);
        weighted_step_emit(tid, GROUP_THREADS, x, table, made, WEIGHTED_PASS, att_id, flag, have, sg.num, s_ins, s_result);
        __syncthreads();
        have += flag[WEIGHTED_PASS];
        if (have >= sg.num)
        {
          x = s_result[0];
          made = s_result[1];
        }
        else
        {
          x = minstd_jump(x, 2ull * WEIGHTED_PASS, table);
          made += WEIGHTED_PASS;
        }
        __syncthreads();
      }
      if (x == 0u)
        break;
      // the container's order
      const int phases = weighted_phase_count(sg.num);
      uint32_t *cur = s_cur, *next = s_next, m_prev = 0u;
      for (int j = 0; j < phases; ++j)
      {
        const uint32_t b = static_cast<uint32_t>(weighted_bucket_count(j));
        const WeightedPhase ph{ b, sg.num < b ? sg.num : b, m_prev, cur, s_ins, s_head, s_link, s_first_of, s_later, s_size, next };
        weighted_phase_clear(tid, GROUP_THREADS, ph);
        __syncthreads();
        weighted_phase_link(tid, GROUP_THREADS, ph);
        __syncthreads();
        weighted_phase_walk(tid, GROUP_THREADS, ph);
        __syncthreads();
        weighted_group_scan(s_size, ph.m + 1u, s_part);
        weighted_phase_place(tid, GROUP_THREADS, ph, s_size);
        __syncthreads();
        m_prev = ph.m;
        uint32_t* t = cur;
        cur = next;
        next = t;
      }
      for (uint32_t i = tid; i < sg.num; i += GROUP_THREADS)
        sg.out[i] = cur[i];
      __syncthreads();
    }
    if (tid == 0u)
      result[1 + s] = made;
  }
  if (tid == 0u)
    result[0] = x;
}

// ---- the general form: the same steps, one launch each ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void weighted_draw_kernel(uint32_t x0, const uint32_t* __restrict__ table, WeightedCloud cloud,
                                                            uint32_t t_base, uint32_t n_att, uint32_t* __restrict__ att_id)
{
  weighted_step_draw(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, x0, table, cloud, t_base, n_att, att_id);
}

__global__ __launch_bounds__(256) void weighted_flag_kernel(WeightedCloud cloud, uint32_t t_base, uint32_t n_att,
                                                            const uint32_t* __restrict__ att_id, uint32_t* __restrict__ flag)
{
  weighted_step_flag(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, cloud, t_base, n_att, att_id, flag);
}

__global__ __launch_bounds__(256) void weighted_emit_kernel(uint32_t x0, const uint32_t* __restrict__ table, uint32_t t_base,
                                                            uint32_t n_att, const uint32_t* __restrict__ att_id,
                                                            const uint32_t* __restrict__ scanned, uint32_t have, uint32_t num,
                                                            uint32_t* __restrict__ ins, uint32_t* __restrict__ result)
{
  weighted_step_emit(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, x0, table, t_base, n_att, att_id, scanned, have, num, ins,
                     result);
}

__global__ __launch_bounds__(256) void weighted_phase_clear_kernel(WeightedPhase ph)
{
  weighted_phase_clear(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, ph);
}
__global__ __launch_bounds__(256) void weighted_phase_link_kernel(WeightedPhase ph)
{
  weighted_phase_link(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, ph);
}
__global__ __launch_bounds__(256) void weighted_phase_walk_kernel(WeightedPhase ph)
{
  weighted_phase_walk(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, ph);
}
__global__ __launch_bounds__(256) void weighted_phase_place_kernel(WeightedPhase ph, const uint32_t* __restrict__ scanned)
{
  weighted_phase_place(blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u, ph, scanned);
}
}  // namespace rng
}  // namespace mcl3dl
