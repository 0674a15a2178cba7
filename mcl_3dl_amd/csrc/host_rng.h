// host_rng.h — part of the single translation unit mcl3dl_hip.hip: the rounds that drive rng_stream_kernels.h on ONE context (the
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

// an engine state handed to a call on a context or a device group: anything that has `fail`
template <typename Owner>
int rng_check_state(Owner* owner, const uint32_t* engine_state)
{
  if (!engine_state)
    return owner->fail(-3, "null engine_state");
  if (*engine_state < 1u || *engine_state > rng::MINSTD_M - 1u)
    return owner->fail(-3, "engine_state %u is outside [1, 2^31 - 2]", *engine_state);
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

constexpr uint64_t RNG_PER_GROUP = static_cast<uint64_t>(rng::GROUP_THREADS) * rng::ATTEMPTS_PER_LANE;

inline uint64_t rng_groups(uint64_t n_att)
{
  return (n_att + RNG_PER_GROUP - 1) / RNG_PER_GROUP;
}

// The count pass over the n_att attempts behind engine state x and the exclusive scan of its counts, in ctx->rng_counts:
// counts[0 .. n_groups) | [n_groups] = the total behind the scan | `tail` more words, cleared, for the caller's result.
// total_home: the total comes home at once (one synchronisation); null: the caller brings it home with its result.
template <typename Policy>
int rng_count_scan(mcl3dl_hip_ctx* ctx, uint32_t x, const Policy& policy, uint64_t n_att, int tail, uint32_t* total_home)
{
  const uint64_t n_groups = rng_groups(n_att);
  TRY(ensure(ctx, ctx->rng_counts, sizeof(uint32_t) * (n_groups + 1 + tail)));
  TRY(ensure(ctx, ctx->rng_ws, sizeof(uint32_t) * (n_groups / 1023 + 8)));
  uint32_t* d_counts = ctx->rng_counts.as<uint32_t>();
  HIP_TRY(hipMemsetAsync(d_counts + n_groups, 0, sizeof(uint32_t) * (1 + tail), ctx->stream));
  hipLaunchKernelGGL(rng::stream_count_kernel<Policy>, dim3(static_cast<unsigned>(n_groups)), dim3(rng::GROUP_THREADS), 0,
                     ctx->stream, x, ctx->rng_table.as<uint32_t>(), policy, static_cast<unsigned long long>(n_att), d_counts);
  HIP_TRY(hipGetLastError());
  TRY(device_exclusive_scan_ws(ctx, d_counts, static_cast<long long>(n_groups) + 1, ctx->rng_ws.as<uint32_t>()));
  if (total_home)
  {
    TRY(d2h(ctx, total_home, d_counts + n_groups, sizeof(uint32_t)));
    TRY(sync_stream(ctx));
  }
  return 0;
}

// stream_emit_kernel behind rng_count_scan's counts: the accepted attempts go to the sink at rank_base + their rank in the
// round, below k_total; d_result takes the engine state behind the k_total-th
template <typename Policy, typename Sink>
int rng_emit(mcl3dl_hip_ctx* ctx, uint32_t x, const Policy& policy, uint64_t n_att, uint64_t rank_base, uint64_t k_total,
             const Sink& sink, uint32_t* d_result)
{
  hipLaunchKernelGGL((rng::stream_emit_kernel<Policy, Sink>), dim3(static_cast<unsigned>(rng_groups(n_att))),
                     dim3(rng::GROUP_THREADS), 0, ctx->stream, x, ctx->rng_table.as<uint32_t>(), policy,
                     static_cast<unsigned long long>(n_att), ctx->rng_counts.as<uint32_t>(),
                     static_cast<unsigned long long>(rank_base), static_cast<unsigned long long>(k_total), sink, d_result);
  HIP_TRY(hipGetLastError());
  return 0;
}

// k_total accepted attempts of the policy's stream from engine state `state_in`, handed to the sink at their ranks; *state_out =
// the engine state behind the last of them. Round r evaluates policy.budget(what is still missing) attempts behind the last one
// evaluated; the accepted total comes home with the result word, in the one synchronisation the call needs anyway. A round that
// falls short is part of the ordinary path. `plural`, `singular`: what the family's messages call an accepted attempt.
template <typename Policy, typename Sink>
int rng_rounds(mcl3dl_hip_ctx* ctx, uint32_t state_in, const Policy& policy, uint64_t k_total, const Sink& sink, const char* plural,
               const char* singular, uint32_t* state_out)
{
  TRY(rng_device_table(ctx));
  uint32_t x = state_in;
  uint64_t accepted = 0;
  for (int round = 0; accepted < k_total; ++round)
  {
    if (round >= 64)
      return ctx->fail(-4, "internal: the random stream did not yield %llu accepted attempts in 64 rounds",
                       static_cast<unsigned long long>(k_total));
    const uint64_t n_att = policy.budget(k_total - accepted);
    const uint64_t n_groups = rng_groups(n_att);
    if (n_groups > 0x7fffffffull)
      return ctx->fail(-3, "%llu %s are more than one call draws", static_cast<unsigned long long>(k_total), plural);
    TRY(rng_count_scan(ctx, x, policy, n_att, 1, nullptr));
    uint32_t* d_tail = ctx->rng_counts.as<uint32_t>() + n_groups;
    TRY(rng_emit(ctx, x, policy, n_att, accepted, k_total, sink, d_tail + 1));
    uint32_t home[2] = { 0u, 0u };  // {accepted in this round, engine state behind the k_total-th or 0}
    TRY(d2h(ctx, home, d_tail, sizeof(home)));
    TRY(sync_stream(ctx));
    accepted += home[0];
    if (accepted >= k_total)
    {
      if (home[1] == 0u || home[1] >= rng::MINSTD_M)
        return ctx->fail(-4, "internal: no lane reported the engine state behind the last %s", singular);
      *state_out = home[1];
    }
    else
      x = rng::minstd_jump(x, Policy::CALLS * n_att, rng_host_table());
  }
  return 0;
}

// k_total accepted polar attempts of the stream that starts at engine state `state_in`; the values of the accepted attempts
// [k_begin, k_end) go to ctx->rng_values (one per attempt, or the pair {y mult, x mult} with `pairs`); *state_out = the engine
// state behind the last of the k_total.
int rng_draw(mcl3dl_hip_ctx* ctx, uint32_t state_in, uint64_t k_total, bool pairs, uint64_t k_begin, uint64_t k_end,
             uint32_t* state_out)
{
  *state_out = state_in;
  if (k_total == 0)
    return 0;
  k_end = std::min(k_end, k_total);
  k_begin = std::min(k_begin, k_end);
  TRY(ensure(ctx, ctx->rng_values, sizeof(float) * (pairs ? 2 : 1) * (k_end - k_begin)));
  float* values = ctx->rng_values.as<float>();
  if (pairs)
    return rng_rounds(ctx, state_in, rng::PolarPolicy{}, k_total, rng::PolarSink<true>{ k_begin, k_end, values }, "values", "value",
                      state_out);
  return rng_rounds(ctx, state_in, rng::PolarPolicy{}, k_total, rng::PolarSink<false>{ k_begin, k_end, values }, "values", "value",
                    state_out);
}

// The uniform sampler's draws, rounds form: `count` draws of uniform_int_distribution over `r` from engine state `state_in` into
// d_out (device, count words); *state_out = the engine state behind the last draw.
int rng_index_rounds(mcl3dl_hip_ctx* ctx, uint32_t state_in, const rng::IndexRange& r, uint64_t count, uint32_t* d_out,
                     uint32_t* state_out)
{
  *state_out = state_in;
  if (count == 0)
    return 0;
  return rng_rounds(ctx, state_in, rng::IndexPolicy{ r }, count, rng::IndexSink{ r, d_out }, "indices", "index", state_out);
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

// n_rows rows of State6DOF::generateNoise behind MultivariateNoiseGenerator(gen), rows [row_begin, row_begin + n_rows) of the
// n_total the call draws in row order, into d_rows13 (device). One normal_distribution per particle called six times: the saved
// second value of every accepted attempt is used inside the particle, so the stream is that of one shared distribution, 3 n_total
// accepted attempts, attempt k giving values 2k and 2k + 1. Zero entries of the transform draw like any other.
int rng_multivariate_rows(mcl3dl_hip_ctx* ctx, uint32_t state_in, const rng::NoiseGenFull6& gen, uint64_t n_total,
                          uint64_t row_begin, size_t n_rows, float* d_rows13, uint32_t* state_out)
{
  TRY(rng_draw(ctx, state_in, 3 * n_total, true, 3 * row_begin, 3 * (row_begin + n_rows), state_out));
  if (n_rows == 0)
    return 0;
  hipLaunchKernelGGL(rng::rng_multivariate_state_kernel, dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0,
                     ctx->stream, ctx->rng_values.as<float>(), gen, static_cast<int>(n_rows), d_rows13);
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
