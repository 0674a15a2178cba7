// host_rng.h — part of the single translation unit mcl3dl_hip.hip: the rounds that drive rng_kernels.h on ONE context (the
// entry points over a device group are in api_rng.inl). A device group runs this on every rank with the same engine state:
// count pass and scan cover the whole stream (deterministic replicas, no collective, as the centroid filter of the global
// localisation), only the values of the rank's window [k_begin, k_end) of accepted attempts are written.
#pragma once

#include <array>

namespace
{
inline const uint32_t* rng_host_table()
{
  static const std::array<uint32_t, 64> table = []
  {
    std::array<uint32_t, 64> t{};
    rng::minstd_build_table(t.data());
    return t;
  }();
  return table.data();
}

// an engine state handed to a call on ONE context (api_rng.inl: rng_check_state is the group's form)
int rng_check_state_ctx(mcl3dl_hip_ctx* ctx, const uint32_t* engine_state)
{
  if (!engine_state)
    return ctx->fail(-3, "null engine_state");
  if (*engine_state < 1u || *engine_state > rng::MINSTD_M - 1u)
    return ctx->fail(-3, "engine_state %u is outside [1, 2^31 - 2]", *engine_state);
  return 0;
}

// the jump table on the device, uploaded once per context
int rng_device_table(mcl3dl_hip_ctx* ctx)
{
  if (ctx->rng_table_set)
    return 0;
  TRY(ensure(ctx, ctx->rng_table, sizeof(uint32_t) * 64));
  TRY(h2d(ctx, ctx->rng_table.p, rng_host_table(), sizeof(uint32_t) * 64));
  ctx->rng_table_set = true;
  return 0;
}

// k_total accepted attempts of the stream that starts at engine state `state_in`; the values of the accepted attempts
// [k_begin, k_end) go to ctx->rng_values (one per attempt, or the pair {y mult, x mult} with `pairs`); *state_out = the engine
// state behind the last of the k_total. Round r evaluates attempt_budget(what is still missing) attempts behind the last one
// evaluated; the accepted total comes home with the result word, in the one synchronisation the call needs anyway.
int rng_draw(mcl3dl_hip_ctx* ctx, uint32_t state_in, uint64_t k_total, bool pairs, uint64_t k_begin, uint64_t k_end,
             uint32_t* state_out)
{
  *state_out = state_in;
  if (k_total == 0)
    return 0;
  constexpr uint64_t PER_GROUP = static_cast<uint64_t>(rng::GROUP_THREADS) * rng::ATTEMPTS_PER_LANE;
  TRY(rng_device_table(ctx));
  k_end = std::min(k_end, k_total);
  k_begin = std::min(k_begin, k_end);
  TRY(ensure(ctx, ctx->rng_values, sizeof(float) * (pairs ? 2 : 1) * (k_end - k_begin)));
  const uint32_t* d_table = ctx->rng_table.as<uint32_t>();
  uint32_t x = state_in;
  uint64_t accepted = 0;
  for (int round = 0; accepted < k_total; ++round)
  {
    if (round >= 64)
      return ctx->fail(-4, "internal: the random stream did not yield %llu accepted attempts in 64 rounds",
                       static_cast<unsigned long long>(k_total));
    const uint64_t n_att = rng::attempt_budget(k_total - accepted);
    const uint64_t n_groups = (n_att + PER_GROUP - 1) / PER_GROUP;
    if (n_groups > 0x7fffffffull)
      return ctx->fail(-3, "%llu values are more than one call draws", static_cast<unsigned long long>(k_total));
    // counts[0 .. n_groups) | [n_groups] = 0, the total behind the scan | [n_groups + 1] = the result word
    TRY(ensure(ctx, ctx->rng_counts, sizeof(uint32_t) * (n_groups + 2)));
    TRY(ensure(ctx, ctx->rng_ws, sizeof(uint32_t) * (n_groups / 1023 + 8)));
    uint32_t* d_counts = ctx->rng_counts.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(d_counts + n_groups, 0, sizeof(uint32_t) * 2, ctx->stream));
    const dim3 grid(static_cast<unsigned>(n_groups)), block(rng::GROUP_THREADS);
    hipLaunchKernelGGL(rng::rng_polar_count_kernel, grid, block, 0, ctx->stream, x, d_table,
                       static_cast<unsigned long long>(n_att), d_counts);
    HIP_TRY(hipGetLastError());
    TRY(device_exclusive_scan_ws(ctx, d_counts, static_cast<long long>(n_groups) + 1, ctx->rng_ws.as<uint32_t>()));
    if (pairs)
      hipLaunchKernelGGL(rng::rng_polar_emit_kernel<true>, grid, block, 0, ctx->stream, x, d_table,
                         static_cast<unsigned long long>(n_att), d_counts, static_cast<unsigned long long>(accepted),
                         static_cast<unsigned long long>(k_total), static_cast<unsigned long long>(k_begin),
                         static_cast<unsigned long long>(k_end), ctx->rng_values.as<float>(), d_counts + n_groups + 1);
    else
      hipLaunchKernelGGL(rng::rng_polar_emit_kernel<false>, grid, block, 0, ctx->stream, x, d_table,
                         static_cast<unsigned long long>(n_att), d_counts, static_cast<unsigned long long>(accepted),
                         static_cast<unsigned long long>(k_total), static_cast<unsigned long long>(k_begin),
                         static_cast<unsigned long long>(k_end), ctx->rng_values.as<float>(), d_counts + n_groups + 1);
    HIP_TRY(hipGetLastError());
    uint32_t home[2] = { 0u, 0u };  // {accepted in this round, engine state behind the k_total-th or 0}
    TRY(d2h(ctx, home, d_counts + n_groups, sizeof(home)));
    TRY(sync_stream(ctx));
    accepted += home[0];
    if (accepted >= k_total)
    {
      if (home[1] == 0u || home[1] >= rng::MINSTD_M)
        return ctx->fail(-4, "internal: no lane reported the engine state behind the last value");
      *state_out = home[1];
    }
    else
      x = rng::minstd_jump(x, 2 * n_att, rng_host_table());
  }
  return 0;
}

// The uniform sampler's draws, rounds form (rng_index_kernels.h): `count` draws of uniform_int_distribution over `r` from engine
// state `state_in` into d_out (device, count words); *state_out = the engine state behind the last draw. rng_draw's scheme with
// one engine output per attempt: round r evaluates index_attempt_budget(what is still missing) attempts behind the last one
// evaluated, and the accepted total and the state come home each round.
int rng_index_rounds(mcl3dl_hip_ctx* ctx, uint32_t state_in, const rng::IndexRange& r, uint64_t count, uint32_t* d_out,
                     uint32_t* state_out)
{
  *state_out = state_in;
  if (count == 0)
    return 0;
  constexpr uint64_t PER_GROUP = static_cast<uint64_t>(rng::GROUP_THREADS) * rng::ATTEMPTS_PER_LANE;
  TRY(rng_device_table(ctx));
  const uint32_t* d_table = ctx->rng_table.as<uint32_t>();
  uint32_t x = state_in;
  uint64_t accepted = 0;
  for (int round = 0; accepted < count; ++round)
  {
    if (round >= 64)
      return ctx->fail(-4, "internal: the random stream did not yield %llu accepted attempts in 64 rounds",
                       static_cast<unsigned long long>(count));
    const uint64_t n_att = rng::index_attempt_budget(count - accepted, r);
    const uint64_t n_groups = (n_att + PER_GROUP - 1) / PER_GROUP;
    if (n_groups > 0x7fffffffull)
      return ctx->fail(-3, "%llu indices are more than one call draws", static_cast<unsigned long long>(count));
    // counts[0 .. n_groups) | [n_groups] = 0, the total behind the scan | [n_groups + 1] = the result word
    TRY(ensure(ctx, ctx->rng_counts, sizeof(uint32_t) * (n_groups + 2)));
    TRY(ensure(ctx, ctx->rng_ws, sizeof(uint32_t) * (n_groups / 1023 + 8)));
    uint32_t* d_counts = ctx->rng_counts.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(d_counts + n_groups, 0, sizeof(uint32_t) * 2, ctx->stream));
    const dim3 grid(static_cast<unsigned>(n_groups)), block(rng::GROUP_THREADS);
    hipLaunchKernelGGL(rng::rng_index_count_kernel, grid, block, 0, ctx->stream, x, d_table, r,
                       static_cast<unsigned long long>(n_att), d_counts);
    HIP_TRY(hipGetLastError());
    TRY(device_exclusive_scan_ws(ctx, d_counts, static_cast<long long>(n_groups) + 1, ctx->rng_ws.as<uint32_t>()));
    hipLaunchKernelGGL(rng::rng_index_emit_kernel, grid, block, 0, ctx->stream, x, d_table, r,
                       static_cast<unsigned long long>(n_att), d_counts, static_cast<unsigned long long>(accepted),
                       static_cast<unsigned long long>(count), d_out, d_counts + n_groups + 1);
    HIP_TRY(hipGetLastError());
    uint32_t home[2] = { 0u, 0u };  // {accepted in this round, engine state behind the count-th or 0}
    TRY(d2h(ctx, home, d_counts + n_groups, sizeof(home)));
    TRY(sync_stream(ctx));
    accepted += home[0];
    if (accepted >= count)
    {
      if (home[1] == 0u || home[1] >= rng::MINSTD_M)
        return ctx->fail(-4, "internal: no lane reported the engine state behind the last index");
      *state_out = home[1];
    }
    else
      x = rng::minstd_jump(x, n_att, rng_host_table());
  }
  return 0;
}

// The uniform sampler's draws, one-work-group form: segment 0 then segment 1 on one stream, in ONE launch and without a host
// round; the engine state behind the last draw goes to *d_state (device). count0 + count1 in [1, INDEX_SINGLE_MAX].
int rng_index_single(mcl3dl_hip_ctx* ctx, uint32_t state_in, const rng::IndexSegment& seg0, const rng::IndexSegment& seg1,
                     uint32_t* d_state)
{
  TRY(rng_device_table(ctx));
  hipLaunchKernelGGL(rng::rng_index_single_kernel, dim3(1), dim3(rng::GROUP_THREADS), 0, ctx->stream, state_in,
                     ctx->rng_table.as<uint32_t>(), seg0, seg1, d_state);
  HIP_TRY(hipGetLastError());
  return 0;
}

// n_rows rows of State6DOF::generateNoise behind DiagonalNoiseGenerator(gen), rows [row_begin, row_begin + n_rows) of the
// n_total the call draws in row order, into d_rows13 (device). All sigmas zero: nothing is drawn, every row is the mean's.
int rng_noise_rows(mcl3dl_hip_ctx* ctx, uint32_t state_in, const rng::NoiseGen6& gen, uint64_t n_total, uint64_t row_begin,
                   size_t n_rows, float* d_rows13, uint32_t* state_out)
{
  const uint64_t D = static_cast<uint64_t>(gen.dims);
  TRY(rng_draw(ctx, state_in, n_total * D, false, row_begin * D, (row_begin + n_rows) * D, state_out));
  if (n_rows == 0)
    return 0;
  hipLaunchKernelGGL(rng::rng_noise_state_kernel, dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0, ctx->stream,
                     ctx->rng_values.as<float>(), gen, static_cast<int>(n_rows), d_rows13);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Quat::getRPY (quat.h:191-201) of the mean's rotation, once on the host: float storage, double intermediates, atan2 / asin in
// double rounded to float (the rule of the landmark update)
inline void rng_mean6(const float* mean7, float* mean6)
{
  const RpyTerms t = quat_rpy_terms(Quat{ mean7[3], mean7[4], mean7[5], mean7[6] });
  mean6[0] = mean7[0];
  mean6[1] = mean7[1];
  mean6[2] = mean7[2];
  mean6[3] = static_cast<float>(std::atan2(static_cast<double>(t.t3), static_cast<double>(t.t4)));
  mean6[4] = static_cast<float>(std::asin(static_cast<double>(t.t2)));
  mean6[5] = static_cast<float>(std::atan2(static_cast<double>(t.t1), static_cast<double>(t.t0)));
}
}  // namespace
