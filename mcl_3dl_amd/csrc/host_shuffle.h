// host_shuffle.h — part of the single translation unit mcl3dl_hip.hip: the first m entries of std::shuffle(iota(n), engine_) on
// ONE context (rng_shuffle.h holds the restatement, rng_shuffle_kernels.h the kernels; the entry points are in api_shuffle.inl).
//
//   n <= 46340   libstdc++'s pair path: the serial loop of rng_shuffle.h ON THE HOST (at most 27 000 engine calls); the caller
//                uploads the m indices where a device needs them
//   n >= 46341   the single path ON THE DEVICE: doubtful attempts counted, compacted and resolved (one small copy home per
//                launch group: their number, then {rejections, complete}), every step's target written, the pairs sorted with
//                the cloud path's stable radix sort, one chain walk per entry. A device group runs this on every rank with the
//                same engine state (deterministic replicas, no collective, as host_rng.h's draws).
#pragma once

namespace
{
// the whole shuffle on the host; the first m entries stay in `a`
void shuffle_prefix_host(uint64_t n, uint64_t m, uint32_t state_in, std::vector<uint32_t>& a, uint32_t* state_out)
{
  a.resize(n);
  uint32_t state = state_in;
  rng::shuffle_serial(n, &state, a.data(), false, nullptr);
  a.resize(m);
  *state_out = state;
}

// n >= 2, m in [1, n]: a[0 .. m) of the single path's shuffle into ctx->sh_idx (device); *state_out = the engine state behind
// the WHOLE shuffle. Nothing is synchronised behind the last launch.
int shuffle_prefix_device(mcl3dl_hip_ctx* ctx, uint64_t n, uint64_t m, uint32_t state_in, uint32_t* state_out)
{
  TRY(rng_device_table(ctx));
  const uint32_t* d_table = ctx->rng_table.as<uint32_t>();
  TRY(ensure(ctx, ctx->sh_target, sizeof(uint32_t) * n));
  TRY(ensure(ctx, ctx->sh_idx, sizeof(uint32_t) * m));
  const unsigned long long n_ull = n;
  const rng::DoubtPolicy policy{ n_ull };
  uint64_t n_att = 0, accepted = 0;
  uint32_t n_rejected = 0;
  for (int round = 0;; ++round)
  {
    if (round >= 64)
      return ctx->fail(-4, "internal: the random stream did not yield the %llu steps of the shuffle in 64 rounds", n_ull - 1);
    n_att = policy.budget(n_att, accepted);
    const uint64_t n_groups = rng_groups(n_att);
    if (n_att > 0xffffffffull || n_groups > 0x7fffffffull)
      return ctx->fail(-3, "a shuffle of %llu elements takes more attempts than the device path numbers in 32 bits", n_ull);
    // two tail words behind the total: the resolve kernel's result
    uint32_t n_doubt = 0;
    TRY(rng_count_scan(ctx, state_in, policy, n_att, 2, &n_doubt));
    uint32_t* d_result = ctx->rng_counts.as<uint32_t>() + n_groups + 1;
    n_rejected = 0;
    if (n_doubt == 0)
      break;  // every attempt is accepted wherever it arrives, and the budget is at least n - 1
    TRY(ensure(ctx, ctx->sh_doubt_t, sizeof(uint32_t) * n_doubt));
    TRY(ensure(ctx, ctx->sh_doubt_v, sizeof(uint32_t) * n_doubt));
    TRY(ensure(ctx, ctx->sh_rejected, sizeof(uint32_t) * n_doubt));
    // (the emit kernel's result word is not used: the resolve kernel behind it overwrites it)
    TRY(rng_emit(ctx, state_in, policy, n_att, 0, n_doubt,
                 rng::DoubtSink{ ctx->sh_doubt_t.as<uint32_t>(), ctx->sh_doubt_v.as<uint32_t>() }, d_result));
    hipLaunchKernelGGL(rng::shuffle_resolve_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->sh_doubt_t.as<uint32_t>(),
                       ctx->sh_doubt_v.as<uint32_t>(), n_doubt, n_ull, static_cast<unsigned long long>(n_att),
                       ctx->sh_rejected.as<uint32_t>(), d_result);
    HIP_TRY(hipGetLastError());
    uint32_t home[2] = { 0u, 0u };  // {rejections among the steps, 1 = the attempts hold every step}
    TRY(d2h(ctx, home, d_result, sizeof(home)));
    TRY(sync_stream(ctx));
    if (home[0] > n_doubt)
      return ctx->fail(-4, "internal: %u rejections among %u doubtful attempts", home[0], n_doubt);
    n_rejected = home[0];
    if (home[1])
      break;
    accepted = n_att - n_rejected;
  }
  const uint64_t n_used = (n - 1) + n_rejected;
  hipLaunchKernelGGL(rng::shuffle_targets_kernel, dim3(static_cast<unsigned>(rng_groups(n_used))),
                     dim3(rng::GROUP_THREADS), 0, ctx->stream, state_in, d_table, n_ull, static_cast<unsigned long long>(n_used),
                     ctx->sh_rejected.as<uint32_t>(), n_rejected, ctx->sh_target.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  // (j_i, i - 1) by j_i: the keys are target[1 ..], the values the sort's own index; keys are at most n - 1
  RsKeyGen kg{};
  kg.keys = ctx->sh_target.as<uint32_t>() + 1;
  TRY(radix_sort<RS_KEY_ARRAY>(ctx, kg, static_cast<long long>(n - 1), bits_for(n - 1), nullptr));
  hipLaunchKernelGGL(rng::shuffle_chain_kernel, dim3(blocks_for(static_cast<long long>(m))), dim3(256), 0, ctx->stream,
                     ctx->cl_key[1].as<uint32_t>(), ctx->cl_val[1].as<uint32_t>(), ctx->sh_target.as<uint32_t>(),
                     static_cast<uint32_t>(n), static_cast<uint32_t>(m), ctx->sh_idx.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  *state_out = rng::minstd_jump(state_in, n_used, rng_host_table());
  return 0;
}
}  // namespace
