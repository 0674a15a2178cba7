// api_shuffle.inl — included inside the extern "C" block of mcl3dl_hip.hip after api_rng.inl: pf::covariance(1.0, ratio) with
// ratio < 1 (pf.h:304-360) on the resident particles of a device group — the case in which the reference shuffles iota(p_num)
// with std::shuffle(.., engine_) and sums over the first p_num * ratio indices (src/mcl_3dl.cpp:373 and :706, while there are more
// particles than num_particles).
//
//   mcl3dl_hip_rng_shuffle_prefix                     the first m entries of that shuffle and the engine state behind it
//   mcl3dl_hip_covariance_window_partial_device       one shard's 22 sums over a list that names particles of the whole set
//   mcl3dl_hip_group_covariance_sampled               the covariance over a list the caller drew
//   mcl3dl_hip_group_covariance_drawn                 the same with the shuffle made from *engine_state
//
// The shuffle (rng_shuffle.h): n <= 46340 is libstdc++'s pair path and is made ON THE HOST by the serial loop (at most 27 000
// engine calls), its m indices uploaded; n >= 46341 is the single path and is made ON THE DEVICE, by every rank for itself
// (deterministic replicas, no collective). Either way the list is in the shuffle's order, so _drawn and _sampled feed the same
// list to the same reduction. p_num is n: the early `break` of pf.h:316 is not reproduced, as in every covariance here.
namespace
{
// Every rank reduces its share of ONE list of m particle numbers: host_list (uploaded), or what `make` leaves on the rank's device.
int group_covariance_over(mcl3dl_hip_group* g, const float* mean7, const uint32_t* host_list, size_t m,
                          const std::function<int(mcl3dl_hip_ctx*, int, const uint32_t**)>* make, float* out_cov36)
{
  // (an empty shard holds no entry of the list; rank 0 is never empty: the state behind a draw comes from it)
  return group_covariance_with(
      g, out_cov36,
      [&](mcl3dl_hip_ctx* ctx, int r, size_t lo, size_t n) -> int
      {
        const uint32_t* d_list = nullptr;
        if (host_list)
        {
          TRY(ensure(ctx, ctx->subset, sizeof(uint32_t) * m));
          TRY(h2d(ctx, ctx->subset.p, host_list, sizeof(uint32_t) * m));
          d_list = ctx->subset.as<uint32_t>();
        }
        else
          TRY((*make)(ctx, r, &d_list));
        return mcl3dl_hip_covariance_window_partial_device(ctx, ctx->pose.as<float>(), ctx->gs_weight.as<float>(), n, d_list, m, lo,
                                                           mean7, ctx->gs_rec.as<double>());
      });
}
}  // namespace

int mcl3dl_hip_rng_shuffle_prefix(mcl3dl_hip_ctx* ctx, size_t n, size_t m, uint32_t* engine_state, uint32_t* out_idx)
{
  if (!ctx)
    return -1;
  if (n < 1 || n > rng::SHUFFLE_MAX_N)
    return ctx->fail(-3, "a shuffle of %zu elements is outside [1, 2147483646]", n);
  if (m > n)
    return ctx->fail(-3, "%zu entries of a shuffle of %zu elements asked for", m, n);
  TRY(rng_check_state(ctx, engine_state));
  if (m && !out_idx)
    return ctx->fail(-3, "null out_idx");
  uint32_t state = *engine_state;
  if (rng::shuffle_pair_path(n))
  {
    std::vector<uint32_t> a;
    shuffle_prefix_host(n, m, state, a, &state);
    if (m)
      memcpy(out_idx, a.data(), sizeof(uint32_t) * m);
    *engine_state = state;
    return 0;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  // (m == 0: the stream still moves behind the whole shuffle; one entry is walked and dropped)
  TRY(shuffle_prefix_device(ctx, n, std::max<size_t>(m, 1), state, &state));
  TRY(d2h(ctx, out_idx, ctx->sh_idx.p, sizeof(uint32_t) * m));
  TRY(sync_stream(ctx));
  *engine_state = state;
  return 0;
}

int mcl3dl_hip_covariance_window_partial_device(mcl3dl_hip_ctx* ctx, const float* d_pose, const float* d_weight,
                                                size_t n_window, const uint32_t* d_subset, size_t n_subset, size_t window_lo,
                                                const float* mean7, double* d_out22)
{
  if (!ctx)
    return -1;
  if (n_subset > 0x7fffffffu || n_window > 0xffffffffu || window_lo > 0xffffffffu || !mean7 || !d_out22)
    return ctx->fail(-3, "bad arguments to covariance_window_partial");
  HIP_TRY(hipSetDevice(ctx->device));
  if (n_subset == 0 || n_window == 0)
  {
    HIP_TRY(hipMemsetAsync(d_out22, 0, sizeof(double) * COV_N, ctx->stream));
    return 0;
  }
  if (!d_pose || !d_weight || !d_subset)
    return ctx->fail(-3, "bad arguments to covariance_window_partial");
  const int nb = pf_blocks(n_subset);  // the grid of the unwindowed kernel over the same list: the same lane sums the same entry
  TRY(ensure(ctx, ctx->mom_blocks, sizeof(double) * COV_N * nb));
  const Vec3f exp_rpy = quat_get_rpy(Quat{ mean7[3], mean7[4], mean7[5], mean7[6] });
  hipLaunchKernelGGL(pf_covariance_window_kernel, dim3(nb), dim3(PF_BLOCK), 0, ctx->stream, d_pose, d_weight, d_subset,
                     static_cast<int>(n_subset), static_cast<uint32_t>(window_lo), static_cast<uint32_t>(n_window), mean7[0],
                     mean7[1], mean7[2], exp_rpy, ctx->mom_blocks.as<double>());
  hipLaunchKernelGGL(pf_covariance_reduce_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->mom_blocks.as<double>(), nb, d_out22);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mcl3dl_hip_group_covariance_sampled(mcl3dl_hip_group* g, const float* mean7, const uint32_t* subset, size_t n_subset,
                                        float* out_cov36)
{
  if (!g)
    return -1;
  const size_t n_p = g->n_resident;
  TRY(group_resident(g));
  if (!mean7 || !out_cov36)
    return g->fail(-3, "null mean / covariance array");
  if (!subset || n_subset == 0 || n_subset > 0x7fffffffu)
    return g->fail(-3, "a list of %zu sampled particles", subset ? n_subset : size_t(0));
  for (size_t k = 0; k < n_subset; ++k)
    if (subset[k] >= n_p)
      return g->fail(-3, "subset[%zu] = %u, %zu particles are resident", k, subset[k], n_p);
  return group_covariance_over(g, mean7, subset, n_subset, nullptr, out_cov36);
}

int mcl3dl_hip_group_covariance_drawn(mcl3dl_hip_group* g, const float* mean7, float random_sample_ratio, uint32_t* engine_state,
                                      size_t* out_n_sampled, float* out_cov36)
{
  if (!g)
    return -1;
  const size_t n_p = g->n_resident;
  TRY(group_resident(g));
  if (!mean7 || !out_cov36)
    return g->fail(-3, "null mean / covariance array");
  if (std::isnan(random_sample_ratio) || random_sample_ratio < 0.f)
    return g->fail(-3, "random_sample_ratio must be a number >= 0");
  TRY(rng_check_state(g, engine_state));
  if (n_p > rng::SHUFFLE_MAX_N)
    return g->fail(-3, "a shuffle of %zu elements is outside [1, 2147483646]", n_p);
  if (!(random_sample_ratio < 1.0f))
  {
    // pf.h:322: no shuffle, no draw, every particle in order
    if (out_n_sampled)
      *out_n_sampled = n_p;
    return mcl3dl_hip_group_covariance(g, mean7, out_cov36);
  }
  const size_t m = rng::shuffle_sample_count(n_p, random_sample_ratio);
  if (m == 0)
    return g->fail(-3, "random_sample_ratio %g samples none of %zu particles (the reference divides by zero)",
                   static_cast<double>(random_sample_ratio), n_p);
  uint32_t state = *engine_state;
  if (rng::shuffle_pair_path(n_p))
  {
    std::vector<uint32_t> a;
    shuffle_prefix_host(n_p, m, state, a, &state);
    TRY(group_covariance_over(g, mean7, a.data(), m, nullptr, out_cov36));
  }
  else
  {
    const int N = g->n();
    std::vector<uint32_t> states(N, 0u);
    std::vector<char> drew(N, 0);
    const std::function<int(mcl3dl_hip_ctx*, int, const uint32_t**)> make =
        [&](mcl3dl_hip_ctx* ctx, int r, const uint32_t** d_list) -> int
    {
      TRY(shuffle_prefix_device(ctx, n_p, m, state, &states[r]));
      drew[r] = 1;
      *d_list = ctx->sh_idx.as<uint32_t>();
      return 0;
    };
    TRY(group_covariance_over(g, mean7, nullptr, m, &make, out_cov36));
    TRY(rng_hand_back(g, states, drew, &state));
  }
  *engine_state = state;
  if (out_n_sampled)
    *out_n_sampled = m;
  return 0;
}
