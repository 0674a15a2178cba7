// api_sampler.inl — included inside the extern "C" block of mcl3dl_hip.hip: the reference's second scan sampler,
// PointCloudSamplerWithNormal (include/mcl_3dl/point_cloud_random_samplers/point_cloud_sampler_with_normal.h), up to its first
// random draw. Device code: sampler_kernels.h.
//
//   mcl3dl_hip_sampler_normal_direction   setParticleStatistics + the max_weight ladder + fpc_local (:75-89, :110-129), on the host
//   mcl3dl_hip_scan_normal_weights        normals, weights and cumulative weights (:130-158) of a cloud mcl3dl_hip_scan_begin left
//                                         on the device
//
// The draw itself (:159-177) stays with the caller and its std::default_random_engine; the indices it draws go to
// mcl3dl_hip_scan_finish. The neighbour search runs over a cell grid of the scan's own (build_transient_cell_grid, plain
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
  const float radius = static_cast<float>(normal_search_range);
  const float r2 = static_cast<float>(normal_search_range * normal_search_range);  // radiusSearch(p, double radius, ...)
  if (!(normal_search_range > 0.0) || !std::isfinite(normal_search_range) || !(radius > 0.f) || !std::isfinite(radius) ||
      !(r2 > 0.f) || !std::isfinite(r2))
    return ctx->fail(-3, "normal_search_range must be positive and finite (got %g)", normal_search_range);
  if (!fpc_local3 || !std::isfinite(fpc_local3[0]) || !std::isfinite(fpc_local3[1]) || !std::isfinite(fpc_local3[2]))
    return ctx->fail(-3, "fpc_local is null or not finite");
  if (!std::isfinite(max_weight))
    return ctx->fail(-3, "max_weight is not finite");
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
  LikGrid lg{};
  int reach = 1;
  unsigned long long n_finite = 0;
  TRY(build_transient_cell_grid(ctx, src, cnt, nullptr, radius, false, "scan", ctx->sn_sorted, ctx->sn_cells, &lg, &reach,
                                &n_finite));
  uint32_t without = static_cast<uint32_t>(cnt);
  if (n_finite == 0)
  {
    // nothing but non-finite points: nobody has a neighbour
    if (out_cumulative)
      std::fill(out_cumulative, out_cumulative + cnt, 1.0);
    if (out_normal_xyz)
      std::fill(out_normal_xyz, out_normal_xyz + 3 * cnt, std::numeric_limits<float>::quiet_NaN());
  }
  else
  {
    TRY(ensure(ctx, ctx->sn_weight, sizeof(double) * cnt));
    TRY(ensure(ctx, ctx->sn_count, sizeof(uint32_t) * 4));
    if (out_normal_xyz)
      TRY(ensure(ctx, ctx->sn_normal, sizeof(float) * 3 * cnt));
    HIP_TRY(hipMemsetAsync(ctx->sn_count.p, 0, sizeof(uint32_t) * 4, ctx->stream));
    SnParams prm{};
    prm.r2 = r2;
    prm.reach = reach;
    prm.fx = static_cast<double>(fpc_local3[0]);
    prm.fy = static_cast<double>(fpc_local3[1]);
    prm.fz = static_cast<double>(fpc_local3[2]);
    prm.max_weight_m1 = max_weight - 1.0;
    const long long nn = static_cast<long long>(cnt);
    hipLaunchKernelGGL(sampler_normal_weight_kernel, dim3(blocks_for(nn)), dim3(256), 0, ctx->stream, lg, nn, prm,
                       ctx->sn_weight.as<double>(), out_normal_xyz ? ctx->sn_normal.as<float>() : nullptr,
                       ctx->sn_count.as<uint32_t>());
    HIP_TRY(hipGetLastError());
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
