// api_sampler.inl — included inside the extern "C" block of mcl3dl_hip.hip: the reference's second scan sampler,
// PointCloudSamplerWithNormal (include/mcl_3dl/point_cloud_random_samplers/point_cloud_sampler_with_normal.h). Device code:
// sampler_kernels.h (normals and weights), rng_weighted_kernels.h (cumulative weights, draws, the sampled scan's order).
//
//   mcl3dl_hip_sampler_normal_direction   setParticleStatistics + the max_weight ladder + fpc_local (:75-89, :110-129), on the host
//   mcl3dl_hip_scan_normal_weights        normals, weights and cumulative weights (:130-158) of a cloud mcl3dl_hip_scan_begin left
//                                         on the device, downloaded: the caller draws (:159-177) with its own
//                                         std::default_random_engine and hands the indices to mcl3dl_hip_scan_finish
//   mcl3dl_hip_rng_draw_weighted          :139-177 on weights handed in: cumulative weights, draws, lower_bound, duplicates, the
//                                         unordered_set's order, on the device (rng_weighted_kernels.h, host_weighted.h)
//   mcl3dl_hip_scan_finish_drawn_normal   sample() for both models, nothing but the engine state crossing the bus
//
// The neighbour search runs over a cell grid of the scan's own (build_transient_cell_grid, plain
// metric) in buffers of this file's own: neither the map's index nor global localisation's point set is touched.
namespace
{
// Symmetric 3x3 eigen-decomposition in double (cyclic Jacobi to convergence), eigenvalues ascending, vec[k] = eigenvector of
// val[k]. Only the lower triangle of `a` is read, as Eigen::SelfAdjointEigenSolver does.
void sn_host_eigen3(const double a_in[3][3], double val[3], double vec[3][3])
{
  double a[3][3], v[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      a[i][j] = i >= j ? a_in[i][j] : a_in[j][i];
  for (int sweep = 0; sweep < 32; ++sweep)
  {
    if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0)
      break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q)
      {
        if (a[p][q] == 0.0)
          continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        const int r = 3 - p - q;
        a[p][p] -= t * a[p][q];
        a[q][q] += t * a[p][q];
        a[p][q] = a[q][p] = 0.0;
        const double rp = a[r][p], rq = a[r][q];
        a[r][p] = a[p][r] = c * rp - s * rq;
        a[r][q] = a[q][r] = s * rp + c * rq;
        for (int k = 0; k < 3; ++k)
        {
          const double vp = v[k][p], vq = v[k][q];
          v[k][p] = c * vp - s * vq;
          v[k][q] = s * vp + c * vq;
        }
      }
  }
  int order[3] = { 0, 1, 2 };
  std::sort(order, order + 3, [&](int x, int y) { return a[x][x] < a[y][y]; });
  for (int k = 0; k < 3; ++k)
  {
    val[k] = a[order[k]][order[k]];
    for (int i = 0; i < 3; ++i)
      vec[k][i] = v[i][order[k]];
  }
}
}  // namespace

int mcl3dl_hip_sampler_normal_direction(const float* mean7, const float* cov36, double perform_weighting_ratio,
                                        double max_weight_ratio, double max_weight, float* out_fpc_local3, double* out_max_weight,
                                        double* out_eigen_value_ratio)
{
  if (!mean7 || !cov36 || !out_fpc_local3 || !out_max_weight)
    return -3;
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(mean7[k]))
      return -3;
  if (!std::isfinite(perform_weighting_ratio) || !std::isfinite(max_weight_ratio) || !std::isfinite(max_weight))
    return -3;
  // pos_cov(i, j) = std::abs(covariances[i][j]), :78-85
  double pos_cov[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
    {
      if (!std::isfinite(cov36[6 * i + j]))
        return -3;
      pos_cov[i][j] = std::abs(static_cast<double>(cov36[6 * i + j]));
    }
  double val[3], vec[3][3];
  sn_host_eigen3(pos_cov, val, vec);
  // :110-127, branch for branch (a NaN ratio fails both comparisons and takes the interpolation)
  const double eigen_value_ratio = std::sqrt(val[2] / val[1]);
  double mw = 1.0;
  if (eigen_value_ratio < perform_weighting_ratio)
  {
    mw = 1.0;
  }
  else if (eigen_value_ratio > max_weight_ratio)
  {
    mw = max_weight;
  }
  else
  {
    const double weight_ratio = (eigen_value_ratio - perform_weighting_ratio) / (max_weight_ratio - perform_weighting_ratio);
    mw = 1.0 + (max_weight - 1.0) * weight_ratio;
  }
  // :128-129: Vec3 holds floats; fpc_local = mean_.rot_.inv() * fpc_global in Quat's float arithmetic (quat.h:139-143, 187-190)
  const Vec3f fpc_global{ static_cast<float>(vec[2][0]), static_cast<float>(vec[2][1]), static_cast<float>(vec[2][2]) };
  const Vec3f fpc_local = qrot(qinv(Quat{ mean7[3], mean7[4], mean7[5], mean7[6] }), fpc_global);
  out_fpc_local3[0] = fpc_local.x;
  out_fpc_local3[1] = fpc_local.y;
  out_fpc_local3[2] = fpc_local.z;
  *out_max_weight = mw;
  if (out_eigen_value_ratio)
    *out_eigen_value_ratio = eigen_value_ratio;
  return 0;
}

namespace
{
// the argument checks of mcl3dl_hip_scan_normal_weights that do not depend on the cloud
int scan_normal_weights_check(mcl3dl_hip_ctx* ctx, double normal_search_range, const float* fpc_local3, double max_weight)
{
  const float radius = static_cast<float>(normal_search_range);
  const float r2 = static_cast<float>(normal_search_range * normal_search_range);  // radiusSearch(p, double radius, ...)
  if (!(normal_search_range > 0.0) || !std::isfinite(normal_search_range) || !(radius > 0.f) || !std::isfinite(radius) ||
      !(r2 > 0.f) || !std::isfinite(r2))
    return ctx->fail(-3, "normal_search_range must be positive and finite (got %g)", normal_search_range);
  if (!fpc_local3 || !std::isfinite(fpc_local3[0]) || !std::isfinite(fpc_local3[1]) || !std::isfinite(fpc_local3[2]))
    return ctx->fail(-3, "fpc_local is null or not finite");
  if (!std::isfinite(max_weight))
    return ctx->fail(-3, "max_weight is not finite");
  return 0;
}

// mcl3dl_hip_scan_normal_weights up to and with its kernel launch: the weights of the `cnt` > 0 points at src are left in
// ctx->sn_weight (the normals in ctx->sn_normal with want_normals, the count of points without one in ctx->sn_count[0]).
// *on_device = false: the cloud holds nothing but non-finite points, nobody has a neighbour and nothing was launched — every
// weight is 1 (with fill_ones they are written to ctx->sn_weight all the same).
int scan_normal_weights_launch(mcl3dl_hip_ctx* ctx, const float4* src, size_t cnt, double normal_search_range,
                               const float* fpc_local3, double max_weight, bool want_normals, bool fill_ones, bool* on_device)
{
  const float radius = static_cast<float>(normal_search_range);
  const float r2 = static_cast<float>(normal_search_range * normal_search_range);
  LikGrid lg{};
  int reach = 1;
  unsigned long long n_finite = 0;
  TRY(build_transient_cell_grid(ctx, src, cnt, nullptr, radius, false, "scan", ctx->sn_sorted, ctx->sn_cells, &lg, &reach,
                                &n_finite));
  *on_device = n_finite != 0;
  const long long nn = static_cast<long long>(cnt);
  if (n_finite == 0)
  {
    if (fill_ones)
    {
      TRY(ensure(ctx, ctx->sn_weight, sizeof(double) * cnt));
      hipLaunchKernelGGL(rng::weighted_fill_kernel, dim3(blocks_for(nn)), dim3(256), 0, ctx->stream, ctx->sn_weight.as<double>(), nn,
                         1.0);
      HIP_TRY(hipGetLastError());
    }
    return 0;
  }
  TRY(ensure(ctx, ctx->sn_weight, sizeof(double) * cnt));
  TRY(ensure(ctx, ctx->sn_count, sizeof(uint32_t) * 4));
  if (want_normals)
    TRY(ensure(ctx, ctx->sn_normal, sizeof(float) * 3 * cnt));
  HIP_TRY(hipMemsetAsync(ctx->sn_count.p, 0, sizeof(uint32_t) * 4, ctx->stream));
  SnParams prm{};
  prm.r2 = r2;
  prm.reach = reach;
  prm.fx = static_cast<double>(fpc_local3[0]);
  prm.fy = static_cast<double>(fpc_local3[1]);
  prm.fz = static_cast<double>(fpc_local3[2]);
  prm.max_weight_m1 = max_weight - 1.0;
  hipLaunchKernelGGL(sampler_normal_weight_kernel, dim3(blocks_for(nn)), dim3(256), 0, ctx->stream, lg, nn, prm,
                     ctx->sn_weight.as<double>(), want_normals ? ctx->sn_normal.as<float>() : nullptr,
                     ctx->sn_count.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace

int mcl3dl_hip_scan_normal_weights(mcl3dl_hip_ctx* ctx, int which, double normal_search_range, const float* fpc_local3,
                                   double max_weight, double* out_cumulative, float* out_normal_xyz, size_t capacity, size_t* n,
                                   size_t* n_without_normal)
{
  if (!ctx)
    return -1;
  if (n)
    *n = 0;
  if (n_without_normal)
    *n_without_normal = 0;
  if (which < 0 || which > 2)
    return ctx->fail(-3, "which must be 0..2");
  if (!ctx->sp_ready)
    return ctx->fail(-5, "no prepared scan: call mcl3dl_hip_scan_begin first");
  TRY(scan_normal_weights_check(ctx, normal_search_range, fpc_local3, max_weight));
  const float4* src = which == 0 ? ctx->sp_full.as<float4>() : ctx->sp_clip[which - 1].as<float4>();
  const size_t cnt = which == 0 ? ctx->sp_n_full : ctx->sp_n_clip[which - 1];
  if (n)
    *n = cnt;
  if (cnt == 0)
    return 0;
  if ((out_cumulative || out_normal_xyz) && capacity < cnt)
    return ctx->fail(-3, "capacity %zu < %zu points", capacity, cnt);
  if (cnt > 0x7ffffff0u)
    return ctx->fail(-3, "too many points (%zu)", cnt);
  HIP_TRY(hipSetDevice(ctx->device));
  bool on_device = false;
  TRY(scan_normal_weights_launch(ctx, src, cnt, normal_search_range, fpc_local3, max_weight, out_normal_xyz != nullptr, false,
                                 &on_device));
  uint32_t without = static_cast<uint32_t>(cnt);
  if (!on_device)
  {
    // nothing but non-finite points: nobody has a neighbour
    if (out_cumulative)
      std::fill(out_cumulative, out_cumulative + cnt, 1.0);
    if (out_normal_xyz)
      std::fill(out_normal_xyz, out_normal_xyz + 3 * cnt, std::numeric_limits<float>::quiet_NaN());
  }
  else
  {
    if (out_cumulative)
      TRY(d2h(ctx, out_cumulative, ctx->sn_weight.p, sizeof(double) * cnt));
    if (out_normal_xyz)
      TRY(d2h(ctx, out_normal_xyz, ctx->sn_normal.p, sizeof(float) * 3 * cnt));
    TRY(d2h(ctx, &without, ctx->sn_count.p, sizeof(uint32_t)));
    TRY(sync_stream(ctx));
  }
  if (n_without_normal)
    *n_without_normal = without;
  // cumulative_weight[i] = weight + ((i == 0) ? 0.0 : cumulative_weight[i - 1]), :157 — the reference's sequential double
  // recurrence, run here over the downloaded weights: given the weights, its bits
  if (out_cumulative)
    for (size_t i = 1; i < cnt; ++i)
      out_cumulative[i] = out_cumulative[i] + out_cumulative[i - 1];
  return 0;
}

// Replaces: lines :139-177 of PointCloudSamplerWithNormal::sample on weights the caller hands in — the cumulative recurrence,
// the uniform_real_distribution<double> draws, std::lower_bound, the duplicate rejection and the unordered_set's iteration
// order — for introspection and general use. num == 0: only the cumulative array is formed, of ANY doubles.
int mcl3dl_hip_rng_draw_weighted(mcl3dl_hip_ctx* ctx, const double* weight, size_t n, size_t num, uint32_t* engine_state,
                                 uint32_t* out_idx, double* out_cumulative, uint64_t* out_draws)
{
  if (!ctx)
    return -1;
  if (n && !weight)
    return ctx->fail(-3, "null weights");
  if (n > 0x7ffffff0u)
    return ctx->fail(-3, "too many points (%zu)", n);
  if (num)
  {
    TRY(rng_check_state(ctx, engine_state));
    if (!out_idx)
      return ctx->fail(-3, "null out_idx");
    if (n <= num)
      return ctx->fail(-3, "num = %zu of n = %zu points: a cloud of at most num points is copied, not drawn from", num, n);
    for (size_t i = 0; i < n; ++i)
      if (!(weight[i] >= 1.0) || !std::isfinite(weight[i]))
        return ctx->fail(-3, "weight[%zu] = %g: the draw loop is only known to end for finite weights >= 1", i, weight[i]);
  }
  if (out_draws)
    *out_draws = 0;
  if (n == 0)
    return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(ensure(ctx, ctx->wd_w, sizeof(double) * n));
  TRY(h2d(ctx, ctx->wd_w.p, weight, sizeof(double) * n));
  TRY(weighted_cumulative(ctx, ctx->wd_w.as<double>(), n, 0, num != 0));
  if (out_cumulative)
    TRY(d2h(ctx, out_cumulative, ctx->wd_cum[0].p, sizeof(double) * n));
  double total = 0.0;
  TRY(d2h(ctx, &total, ctx->wd_cum[0].as<double>() + (n - 1), sizeof(double)));
  TRY(sync_stream(ctx));
  if (num == 0)
    return 0;
  if (!(total < rng::WEIGHTED_MAX_TOTAL))
    return ctx->fail(-3, "the weights sum to %g: the draw loop is only known to end below 2^50", total);
  TRY(ensure(ctx, ctx->wd_out, sizeof(uint32_t) * num));
  uint32_t state = *engine_state;
  uint64_t draws = 0;
  if (num <= rng::WEIGHTED_SINGLE_MAX)
  {
    TRY(ensure(ctx, ctx->wd_result, sizeof(uint32_t) * 4));
    const rng::WeightedSegment seg{ weighted_cloud(ctx, 0, n), static_cast<uint32_t>(num), ctx->wd_out.as<uint32_t>() };
    const rng::WeightedSegment none{ rng::WeightedCloud{ nullptr, 0u, nullptr }, 0u, nullptr };
    TRY(weighted_draw_single(ctx, state, seg, none, ctx->wd_result.as<uint32_t>()));
    uint32_t home[3] = { 0u, 0u, 0u };
    TRY(d2h(ctx, home, ctx->wd_result.p, sizeof(home)));
    TRY(d2h(ctx, out_idx, ctx->wd_out.p, sizeof(uint32_t) * num));
    TRY(sync_stream(ctx));
    if (home[0] < 1u || home[0] > rng::MINSTD_M - 1u)
      return ctx->fail(-4, "internal: the weighted draw left no engine state");
    state = home[0];
    draws = home[1];
  }
  else
  {
    TRY(weighted_draw_rounds(ctx, state, 0, n, num, ctx->wd_out.as<uint32_t>(), &state, &draws));
    TRY(d2h(ctx, out_idx, ctx->wd_out.p, sizeof(uint32_t) * num));
    TRY(sync_stream(ctx));
  }
  *engine_state = state;
  if (out_draws)
    *out_draws = draws;
  return 0;
}

// Replaces: PointCloudSamplerWithNormal::sample (point_cloud_sampler_with_normal.h:91-185) for both models of measure()
// (src/mcl_3dl.cpp:377-383: "beam" before "likelihood" on one engine stream) + what mcl3dl_hip_scan_finish replaces. Per model:
// an empty clipped cloud or a count of 0 installs an empty scan and draws nothing (:100-103); a clipped cloud of at most the
// count is installed whole in its own order, nothing drawn, no normals computed (:104-108); otherwise normals -> weights ->
// cumulative weights -> draws -> the container's order, all on the device. From the index buffer on it is mcl3dl_hip_scan_finish.
int mcl3dl_hip_scan_finish_drawn_normal(mcl3dl_hip_ctx* ctx, size_t n_s, size_t n_b, const float* origins, size_t n_o,
                                        double normal_search_range, const float* fpc_local3, double max_weight,
                                        uint32_t* engine_state, size_t* out_n_s, size_t* out_n_b)
{
  if (!ctx)
    return -1;
  if (!ctx->sp_ready)
    return ctx->fail(-5, "no prepared scan: call mcl3dl_hip_scan_begin first");
  TRY(rng_check_state(ctx, engine_state));
  if (n_b && (!origins || n_o == 0))
    return ctx->fail(-3, "n_b = %zu beam points asked for but no origins given", n_b);
  TRY(scan_normal_weights_check(ctx, normal_search_range, fpc_local3, max_weight));
  if (!(max_weight >= 1.0))
    return ctx->fail(-3, "max_weight = %g < 1: the draw loop is only known to end for weights >= 1", max_weight);
  // model 0 = beam (clip 1), model 1 = likelihood (clip 0): the order of the draws
  const size_t want[2] = { n_b, n_s };
  size_t cnt[2], inst[2];
  bool drawn[2];
  for (int k = 0; k < 2; ++k)
  {
    cnt[k] = ctx->sp_n_clip[1 - k];
    if (cnt[k] > 0x7ffffff0u)
      return ctx->fail(-3, "too many points (%zu)", cnt[k]);
    inst[k] = (cnt[k] == 0 || want[k] == 0) ? 0 : std::min(cnt[k], want[k]);
    drawn[k] = inst[k] != 0 && cnt[k] > want[k];
    if (drawn[k] && !(static_cast<double>(cnt[k]) * max_weight < rng::WEIGHTED_MAX_TOTAL))
      return ctx->fail(-3, "%zu points of weight up to %g: the draw loop is only known to end for a total below 2^50", cnt[k],
                       max_weight);
  }
  TRY(scan_finish_prepare(ctx, inst[1], inst[0]));
  uint32_t* d_head = ctx->cl_idx.as<uint32_t>();
  uint32_t* d_idx[2] = { d_head + 4 + inst[1], d_head + 4 };  // [error, state, attempts x2][idx_lik][idx_beam]
  HIP_TRY(hipMemsetAsync(d_head, 0, 16, ctx->stream));
  rng::WeightedSegment seg[2];
  for (int k = 0; k < 2; ++k)
  {
    seg[k] = rng::WeightedSegment{ rng::WeightedCloud{ nullptr, 0u, nullptr }, 0u, nullptr };
    if (inst[k] != 0 && !drawn[k])
    {
      hipLaunchKernelGGL(rng::weighted_iota_kernel, dim3(blocks_for(static_cast<long long>(inst[k]))), dim3(256), 0, ctx->stream,
                         d_idx[k], static_cast<uint32_t>(inst[k]));
      HIP_TRY(hipGetLastError());
    }
    if (!drawn[k])
      continue;
    bool on_device = false;
    TRY(scan_normal_weights_launch(ctx, ctx->sp_clip[1 - k].as<float4>(), cnt[k], normal_search_range, fpc_local3, max_weight, false,
                                   true, &on_device));
    TRY(weighted_cumulative(ctx, ctx->sn_weight.as<double>(), cnt[k], k, true));
    seg[k] = rng::WeightedSegment{ weighted_cloud(ctx, k, cnt[k]), static_cast<uint32_t>(inst[k]), d_idx[k] };
  }
  uint32_t state = *engine_state;
  if (!drawn[0] && !drawn[1])
    TRY(scan_finish_launch(ctx, inst[1], inst[0], origins, n_o, nullptr));
  else if (seg[0].num <= rng::WEIGHTED_SINGLE_MAX && seg[1].num <= rng::WEIGHTED_SINGLE_MAX)
  {
    // one launch; the state rides home in the pad word behind the error word
    TRY(weighted_draw_single(ctx, state, seg[0], seg[1], d_head + 1));
    TRY(scan_finish_launch(ctx, inst[1], inst[0], origins, n_o, &state));
    if (state < 1u || state > rng::MINSTD_M - 1u)
      return ctx->fail(-4, "internal: the weighted draw left no engine state");
  }
  else
  {
    // per model: one launch where the count allows it (its state comes home before the next model starts), rounds otherwise
    for (int k = 0; k < 2; ++k)
    {
      if (!drawn[k])
        continue;
      if (seg[k].num <= rng::WEIGHTED_SINGLE_MAX)
      {
        const rng::WeightedSegment none{ rng::WeightedCloud{ nullptr, 0u, nullptr }, 0u, nullptr };
        TRY(weighted_draw_single(ctx, state, seg[k], none, d_head + 1));
        TRY(d2h(ctx, &state, d_head + 1, sizeof(uint32_t)));
        TRY(sync_stream(ctx));
        if (state < 1u || state > rng::MINSTD_M - 1u)
          return ctx->fail(-4, "internal: the weighted draw left no engine state");
      }
      else
        TRY(weighted_draw_rounds(ctx, state, k, cnt[k], inst[k], d_idx[k], &state, nullptr));
    }
    TRY(scan_finish_launch(ctx, inst[1], inst[0], origins, n_o, nullptr));
  }
  *engine_state = state;
  if (out_n_s)
    *out_n_s = inst[1];
  if (out_n_b)
    *out_n_b = inst[0];
  return 0;
}
