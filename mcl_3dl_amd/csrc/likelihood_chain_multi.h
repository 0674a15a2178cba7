// likelihood_chain_multi.h — strict_order = 3 (the reference's float recurrence inside the likelihood kernel,
// likelihood_kernels.h: LikChain) for FEW particles on LONG scans.
//
// The chain of a particle is n_tiles hand-offs long in likelihood_tiled_kernel<..., CHAIN> — ~2.2 us each, 0.14 ms for a
// 16 384-point scan whatever the particle count — and a hop is mostly the hand-off (a store and a polled load across XCDs,
// ~1.6 us), not the 256 dependent adds (~0.6 us). Below ~3000 particles the evaluation is shorter than the chain and the hops
// are what the launch costs (1024 particles: 0.152 ms against 0.080 ms with fp64 sums, profiles/r05f_chain_midsize.txt). Here
// a work-group evaluates PPL consecutive tiles for its G particles — every term stays in LDS, PPL x G x 260 floats — and only
// THEN takes the running sums over, adds its PPL x 256 terms and hands on: a quarter of the hand-offs for PPL = 4, the same
// adds in the same order, so the same bits. Built from the one-tile form's own pieces (likelihood_kernels.h): xcd_row_map with
// super-tiles as links (rows of eight, one per XCD; a producer always has a lower block index), stage_poses, the general pose
// loop's evaluation with defer_push / defer_flush, and chain_take, PPL x chain_add_row, chain_give — the same hand-off words
// and tags (tag0 + super-tile).
// Measured (profiles/r05r_chain_multi.txt, 16 384 points): 64 particles 0.122 -> 0.096 ms, 1024 particles 0.139 -> 0.122 ms (fp64
// sums: 0.072), 1024 x 65 536 points 0.480 -> 0.358 ms; SLOWER from 2048 particles (groups of four particles, a longer start-up),
// so the host uses it up to CHAIN_MULTI_MAX = 1536 particles (a constant: host_options.h).
// Only the default kernel family (packed 64-byte records, quad-cooperative fetch, deferred overflow rounds); everything else
// and every launch with enough particles stays with likelihood_tiled_kernel<..., CHAIN>.
#pragma once
#include <hip/hip_runtime.h>

#include "likelihood_kernels.h"

#pragma clang fp contract(off)

namespace mcl3dl
{
template <int G, int PPL>
__global__ __launch_bounds__(256, 8) void likelihood_chain_multi_kernel(const float* __restrict__ pose7, int n_p,
                                                                        const float4* __restrict__ scan, int n_s, int n_tiles,
                                                                        int n_super, int n_groups, RecGrid rg, LikParams prm,
                                                                        LikChain ch)
{
  constexpr int LD = 260;  // (rows padded: the chain's lanes read different rows at the same column, 16 bytes at a time)
  __shared__ float s_pose[G][8];
  __shared__ __attribute__((aligned(16))) float s_term[PPL][G][LD];
  __shared__ unsigned s_cnt[PPL][G][4];
  __shared__ DeferQueue s_q;
  int st, group;
  if (!xcd_row_map(blockIdx.x, n_groups, n_super, st, group))
    return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  stage_poses<G>(s_pose, pose7, n_p, group, t);
  __syncthreads();
  const int n_valid = min(G, n_p - group * G);
  const int first_tile = st * PPL;
  const int n_sub = min(PPL, n_tiles - first_tile);
  for (int m = 0; m < n_sub; ++m)
  {
    const int i = (first_tile + m) * 256 + t;
    const bool have_point = i < n_s;
    const float4 v = have_point ? scan[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    // (the general pose loop of likelihood_tiled_kernel<G, 2, 8, true, true>; the queue is empty again before the next tile's
    // point replaces v)
    uint32_t qn = 0;
    for (int k = 0; k < n_valid; ++k)
    {
      const Vec3f pos = { s_pose[k][0], s_pose[k][1], s_pose[k][2] };
      const Quat rot = { s_pose[k][3], s_pose[k][4], s_pose[k][5], s_pose[k][6] };
      bool matched, over;
      float best;
      uint32_t mine;
      unsigned long long over_m;
      const float term = eval_coop_first(rg, prm, pos, rot, v, have_point, lane, matched, over, best, mine, over_m);
      s_term[m][k][t] = over ? best : term;
      const unsigned long long mm = __builtin_amdgcn_ballot_w64(matched);
      if (lane == 0)
        s_cnt[m][k][wave] = static_cast<unsigned>(__popcll(mm));
      // (the mask from a ballot of `over`, not eval_coop_first's over_m: with over_m this kernel measured 1.5-2 % slower at 1024
      // particles, profiles/likelihood_dedup_ab.txt)
      const unsigned long long om = __builtin_amdgcn_ballot_w64(over);
      qn = defer_push<false>(rg, prm, s_pose, s_term[m], s_cnt[m], s_q, wave, lane, v, qn, om, over, mine, k);
    }
    if (qn != 0u)
      defer_flush<false>(rg, prm, s_pose, s_term[m], s_cnt[m], s_q, wave, lane, v, qn);
  }
  __syncthreads();
  if (wave != 0 || lane >= n_valid)
    return;
  // ---- the chain: one lane per particle, one link per super-tile
  const int k = lane;
  const size_t p = static_cast<size_t>(group) * G + k;
  unsigned long long* cw = ch.carry + 2 * p;
  float s;
  uint32_t cnt;
  chain_take(ch, cw, st, s, cnt);
  for (int m = 0; m < n_sub; ++m)
  {
    chain_add_row(&s_term[m][k][0], s);
    cnt += s_cnt[m][k][0] + s_cnt[m][k][1] + s_cnt[m][k][2] + s_cnt[m][k][3];
  }
  chain_give(ch, cw, p, st, st == n_super - 1, n_s, s, cnt);
}
}  // namespace mcl3dl
