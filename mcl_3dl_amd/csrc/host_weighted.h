// host_weighted.h — part of the single translation unit mcl3dl_hip.hip: the launches that drive rng_weighted_kernels.h on ONE
// context (entry points: api_sampler.inl; over a device group: api_group_state.inl, every rank the same call on its replica).
#pragma once

namespace
{
// d_w[0 .. n) -> ctx->wd_cum[slot] as the serial double recurrence; the slot's first-attempt words are reset
int weighted_cumulative(mcl3dl_hip_ctx* ctx, const double* d_w, size_t n, int slot, bool reset_first)
{
  TRY(ensure(ctx, ctx->wd_cum[slot], sizeof(double) * n));
  hipLaunchKernelGGL(rng::weighted_cumulative_kernel, dim3(1), dim3(64), 0, ctx->stream, d_w, ctx->wd_cum[slot].as<double>(),
                     static_cast<long long>(n));
  HIP_TRY(hipGetLastError());
  if (reset_first)
  {
    TRY(ensure(ctx, ctx->wd_first[slot], sizeof(uint32_t) * n));
    HIP_TRY(hipMemsetAsync(ctx->wd_first[slot].p, 0xff, sizeof(uint32_t) * n, ctx->stream));
  }
  return 0;
}

inline rng::WeightedCloud weighted_cloud(mcl3dl_hip_ctx* ctx, int slot, size_t n)
{
  return rng::WeightedCloud{ ctx->wd_cum[slot].as<double>(), static_cast<uint32_t>(n), ctx->wd_first[slot].as<uint32_t>() };
}

// strided kernels: enough work-groups for `items`, no more than fill the device a few times over
inline unsigned weighted_blocks(uint64_t items)
{
  return static_cast<unsigned>(std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 4096));
}

// The general form: `num` ids of the cloud in slot `slot` (n > num > 0 points, cumulative weights and reset first-attempt words in
// place) from engine state state_in, in the container's iteration order, into d_out (device). Rounds of
// weighted_attempt_budget attempts, the new total and the state come home each round; then the order phases, five launches each.
int weighted_draw_rounds(mcl3dl_hip_ctx* ctx, uint32_t state_in, int slot, size_t n, size_t num, uint32_t* d_out,
                         uint32_t* state_out, uint64_t* draws_out)
{
  TRY(rng_device_table(ctx));
  const uint32_t* d_table = ctx->rng_table.as<uint32_t>();
  const rng::WeightedCloud cloud = weighted_cloud(ctx, slot, n);
  TRY(ensure(ctx, ctx->wd_ins, sizeof(uint32_t) * num));
  uint32_t x = state_in, have = 0u;
  uint64_t made = 0;
  for (int round = 0;; ++round)
  {
    if (round >= 4096)
      return ctx->fail(-4, "internal: the weighted draw did not find %zu distinct points in 4096 rounds", num);
    uint64_t n_att = rng::weighted_attempt_budget(have, num, n);
    n_att = std::min<uint64_t>(n_att, 1ull << 28);
    if (made + n_att > rng::WEIGHTED_MAX_ATTEMPTS)
      return ctx->fail(-4, "internal: the weighted draw needs more than 2^32 attempts");
    // flag[0 .. n_att] | [n_att + 1], [n_att + 2] = the result words {state, attempts}
    TRY(ensure(ctx, ctx->wd_att, sizeof(uint32_t) * n_att));
    TRY(ensure(ctx, ctx->wd_flag, sizeof(uint32_t) * (n_att + 3)));
    TRY(ensure(ctx, ctx->wd_ws, sizeof(uint32_t) * ((std::max<uint64_t>(n_att, num) + 1) / 1023 + 8)));
    uint32_t* d_att = ctx->wd_att.as<uint32_t>();
    uint32_t* d_flag = ctx->wd_flag.as<uint32_t>();
    const uint32_t na = static_cast<uint32_t>(n_att), base = static_cast<uint32_t>(made);
    HIP_TRY(hipMemsetAsync(d_flag + n_att + 1, 0, sizeof(uint32_t) * 2, ctx->stream));
    hipLaunchKernelGGL(rng::weighted_draw_kernel, dim3(weighted_blocks(n_att / rng::WEIGHTED_E + 1)), dim3(256), 0, ctx->stream, x,
                       d_table, cloud, base, na, d_att);
    hipLaunchKernelGGL(rng::weighted_flag_kernel, dim3(weighted_blocks(n_att + 1)), dim3(256), 0, ctx->stream, cloud, base, na, d_att,
                       d_flag);
    HIP_TRY(hipGetLastError());
    TRY(device_exclusive_scan_ws(ctx, d_flag, static_cast<long long>(n_att) + 1, ctx->wd_ws.as<uint32_t>()));
    hipLaunchKernelGGL(rng::weighted_emit_kernel, dim3(weighted_blocks(n_att)), dim3(256), 0, ctx->stream, x, d_table, base, na,
                       d_att, d_flag, have, static_cast<uint32_t>(num), ctx->wd_ins.as<uint32_t>(), d_flag + n_att + 1);
    HIP_TRY(hipGetLastError());
    uint32_t home[3] = { 0u, 0u, 0u };  // {new attempts of this round, state behind the num-th id or 0, attempts made}
    TRY(d2h(ctx, home, d_flag + n_att, sizeof(home)));
    TRY(sync_stream(ctx));
    if (have + static_cast<uint64_t>(home[0]) >= num)
    {
      if (home[1] == 0u || home[1] >= rng::MINSTD_M || home[2] == 0u)
        return ctx->fail(-4, "internal: no lane reported the engine state behind the last weighted draw");
      x = home[1];
      made = home[2];
      break;
    }
    have += home[0];
    x = rng::minstd_jump(x, 2 * n_att, rng_host_table());
    made += n_att;
  }
  // the container's order, phase by phase
  const int phases = rng::weighted_phase_count(num);
  const size_t b_last = static_cast<size_t>(rng::weighted_bucket_count(phases - 1));
  TRY(ensure(ctx, ctx->wd_order[0], sizeof(uint32_t) * num));
  TRY(ensure(ctx, ctx->wd_order[1], sizeof(uint32_t) * num));
  TRY(ensure(ctx, ctx->wd_head, sizeof(uint32_t) * b_last));
  TRY(ensure(ctx, ctx->wd_link, sizeof(uint32_t) * num));
  TRY(ensure(ctx, ctx->wd_first_of, sizeof(uint32_t) * num));
  TRY(ensure(ctx, ctx->wd_later, sizeof(uint32_t) * num));
  TRY(ensure(ctx, ctx->wd_size, sizeof(uint32_t) * (num + 1)));
  TRY(ensure(ctx, ctx->wd_ws, sizeof(uint32_t) * ((num + 1) / 1023 + 8)));
  uint32_t m_prev = 0u;
  int cur = 0;
  for (int j = 0; j < phases; ++j)
  {
    const uint32_t b = static_cast<uint32_t>(rng::weighted_bucket_count(j));
    const uint32_t m = static_cast<uint32_t>(std::min<uint64_t>(num, b));
    const rng::WeightedPhase ph{ b,
                                 m,
                                 m_prev,
                                 ctx->wd_order[cur].as<uint32_t>(),
                                 ctx->wd_ins.as<uint32_t>(),
                                 ctx->wd_head.as<uint32_t>(),
                                 ctx->wd_link.as<uint32_t>(),
                                 ctx->wd_first_of.as<uint32_t>(),
                                 ctx->wd_later.as<uint32_t>(),
                                 ctx->wd_size.as<uint32_t>(),
                                 j + 1 == phases ? d_out : ctx->wd_order[cur ^ 1].as<uint32_t>() };
    hipLaunchKernelGGL(rng::weighted_phase_clear_kernel, dim3(weighted_blocks(b)), dim3(256), 0, ctx->stream, ph);
    hipLaunchKernelGGL(rng::weighted_phase_link_kernel, dim3(weighted_blocks(m)), dim3(256), 0, ctx->stream, ph);
    hipLaunchKernelGGL(rng::weighted_phase_walk_kernel, dim3(weighted_blocks(m + 1ull)), dim3(256), 0, ctx->stream, ph);
    HIP_TRY(hipGetLastError());
    TRY(device_exclusive_scan_ws(ctx, ctx->wd_size.as<uint32_t>(), static_cast<long long>(m) + 1, ctx->wd_ws.as<uint32_t>()));
    hipLaunchKernelGGL(rng::weighted_phase_place_kernel, dim3(weighted_blocks(m)), dim3(256), 0, ctx->stream, ph,
                       ctx->wd_size.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    m_prev = m;
    cur ^= 1;
  }
  *state_out = x;
  if (draws_out)
    *draws_out = made;
  return 0;
}

// The one-work-group form: segment 0 then segment 1 on one stream in ONE launch; d_result: {state, attempts 0, attempts 1}
int weighted_draw_single(mcl3dl_hip_ctx* ctx, uint32_t state_in, const rng::WeightedSegment& seg0, const rng::WeightedSegment& seg1,
                         uint32_t* d_result)
{
  TRY(rng_device_table(ctx));
  hipLaunchKernelGGL(rng::weighted_single_kernel, dim3(1), dim3(rng::GROUP_THREADS), 0, ctx->stream, state_in,
                     ctx->rng_table.as<uint32_t>(), seg0, seg1, d_result);
  HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace
