// api_group_motion.inl — included inside the extern "C" block of mcl3dl_hip.hip after api_group_state.inl: what the node does to
// every particle between two scans, on the particles RESIDENT on the group's devices (motion_kernels.h):
//
//   mcl3dl_hip_group_set_odom_noise / _download_odom_noise   State6DOF's noise_ll_ / la_ / al_ / aa_ (src/mcl_3dl.cpp:817-825)
//   mcl3dl_hip_group_predict                                 cbOdom's pf_->predict (:227-232), differential-drive model
//   mcl3dl_hip_group_reset_odom_integ                        integ_reset_func (:190-195, :652-658)
//   mcl3dl_hip_group_add_noise                               pf_->noise (:850-860; pf.h:226-237) with caller-drawn noise
//   mcl3dl_hip_group_measure_imu                             cbImu's pf_->measure (:997-1002), gravity model
//   mcl3dl_hip_group_set_odom_error_sigma                    measure()'s odometry factor (:420-423) formed on the devices
//   mcl3dl_hip_group_measure_landmark                        cbLandmark's pf_->measure (:899-929), NormalLikelihoodNd<float, 6>
//
// Everything but the IMU and the landmark update is shard-local (one launch per rank, no collective). Those two are pf::measure:
// the same partial sums / one all-reduce / apply as mcl3dl_hip_group_update_resident (group_measure_resident), the IMU
// likelihood formed in the partial-sum pass, the landmark likelihood by a launch of its own in front (landmark_kernels.h).
namespace
{
// MotionPredictionModelDifferentialDrive::setOdoms (motion_prediction_model_differential_drive.h:46-54) in float, once per
// call, + the two decay factors of predict (:66-67)
MotionStep motion_step(const float* prev7, const float* cur7, float time_diff, float lin_tc, float ang_tc)
{
  const Quat prev_rot = { prev7[3], prev7[4], prev7[5], prev7[6] };
  const Quat cur_rot = { cur7[3], cur7[4], cur7[5], cur7[6] };
  const Quat pinv = qinv(prev_rot);
  MotionStep m;
  m.t = qrot(pinv, vsub(Vec3f{ cur7[0], cur7[1], cur7[2] }, Vec3f{ prev7[0], prev7[1], prev7[2] }));
  m.rq = qmul(pinv, cur_rot);
  // Quat::getAxisAng (quat.h:226-238): the angle only; std::acos of a float is the host libm's acosf
  if (std::fabs(m.rq.w) >= 1.0 - 0.000001)
    m.ang = 0.0f;
  else
  {
    m.ang = static_cast<float>(std::acos(m.rq.w) * 2.0);
    if (m.ang > M_PI)
      m.ang = static_cast<float>(m.ang - 2.0 * M_PI);
  }
  m.t_norm = std::sqrt(vdot(m.t, m.t));
  m.decay_lin = static_cast<float>(1.0 - static_cast<double>(time_diff / lin_tc));
  m.decay_ang = static_cast<float>(1.0 - static_cast<double>(time_diff / ang_tc));
  return m;
}

inline dim3 grid_of(size_t n)
{
  return dim3(static_cast<unsigned>((n + 255) / 256));
}

// room for the noise of the LARGEST shard on every rank, an empty one included: the resampling step's all-gather sends that many
int odom_noise_room(mcl3dl_hip_ctx* ctx, size_t n_p, int world)
{
  return ensure(ctx, ctx->gs_noise[ctx->gs_cur], sizeof(float) * 4 * shard_capacity(n_p, world));
}
}  // namespace

int mcl3dl_hip_group_set_odom_noise(mcl3dl_hip_group* g, const float* noise4, size_t n_p)
{
  if (!g)
    return -1;
  if (!noise4)
    return g->fail(-3, "null noise array");
  if (g->n_resident == 0 || g->n_resident != n_p)
    return g->fail(-5, "%zu particles are resident, %zu noise records given", g->n_resident, n_p);
  const int rc = group_run_shards(
      g, n_p,
      [&](const Shard& s) -> int
      {
        mcl3dl_hip_ctx* ctx = s.ctx;
        HIP_TRY(hipSetDevice(ctx->device));
        TRY(odom_noise_room(ctx, n_p, g->n()));
        if (s.n == 0)
          return 0;
        TRY(h2d(ctx, ctx->gs_noise[ctx->gs_cur].p, noise4 + 4 * s.lo, sizeof(float) * 4 * s.n));
        return sync_stream(ctx);
      });
  if (rc)
  {
    g->noise_on = false;  // (some shards may hold the new noise, others none: the caller sets it again)
    return rc;
  }
  g->noise_on = true;
  return 0;
}

int mcl3dl_hip_group_download_odom_noise(mcl3dl_hip_group* g, float* noise4, size_t n_p)
{
  if (!g)
    return -1;
  if (!noise4)
    return g->fail(-3, "null noise array");
  if (g->n_resident == 0 || g->n_resident != n_p)
    return g->fail(-5, "%zu particles are resident, %zu asked for", g->n_resident, n_p);
  if (!g->noise_on)
  {
    std::fill(noise4, noise4 + 4 * n_p, 0.0f);
    return 0;
  }
  return group_each_shard(g,
                          [&](mcl3dl_hip_ctx* ctx, int, size_t lo, size_t n) -> int
                          {
                            TRY(d2h(ctx, noise4 + 4 * lo, ctx->gs_noise[ctx->gs_cur].p, sizeof(float) * 4 * n));
                            return sync_stream(ctx);
                          });
}

int mcl3dl_hip_group_predict(mcl3dl_hip_group* g, const float* odom_prev7, const float* odom_cur7, float time_diff,
                             float odom_err_integ_lin_tc, float odom_err_integ_ang_tc)
{
  if (!g)
    return -1;
  if (!odom_prev7 || !odom_cur7)
    return g->fail(-3, "null odometry pose");
  const MotionStep m = motion_step(odom_prev7, odom_cur7, time_diff, odom_err_integ_lin_tc, odom_err_integ_ang_tc);
  const bool noise = g->noise_on;
  return group_each_shard(g,
                          [&](mcl3dl_hip_ctx* ctx, int, size_t, size_t n) -> int
                          {
                            // the pose mirror is written by the same launch (resident_poses() then finds it current)
                            TRY(ensure(ctx, ctx->pose, sizeof(float) * 7 * n));
                            hipLaunchKernelGGL(predict_kernel, grid_of(n), dim3(256), 0, ctx->stream,
                                               ctx->gs_state[ctx->gs_cur].as<float>(),
                                               noise ? ctx->gs_noise[ctx->gs_cur].as<float>() : static_cast<float*>(nullptr),
                                               static_cast<int>(n), m, ctx->pose.as<float>());
                            HIP_TRY(hipGetLastError());
                            pose_mirror_stamp(ctx, n);
                            return sync_stream(ctx);
                          });
}

int mcl3dl_hip_group_reset_odom_integ(mcl3dl_hip_group* g)
{
  if (!g)
    return -1;
  return group_each_shard(g,
                          [&](mcl3dl_hip_ctx* ctx, int, size_t, size_t n) -> int
                          {
                            hipLaunchKernelGGL(reset_odom_integ_kernel, grid_of(n), dim3(256), 0, ctx->stream,
                                               ctx->gs_state[ctx->gs_cur].as<float>(), static_cast<int>(n));
                            HIP_TRY(hipGetLastError());
                            return sync_stream(ctx);
                          });
}

namespace
{
// pf::noise behind the noise rows' arrival in ctx->rs_d_noise (copied from the host, or drawn there: api_rng.inl)
int add_noise_launch(mcl3dl_hip_ctx* ctx, size_t n)
{
  TRY(ensure(ctx, ctx->pose, sizeof(float) * 7 * n));
  hipLaunchKernelGGL(add_noise_kernel, grid_of(n), dim3(256), 0, ctx->stream, ctx->gs_state[ctx->gs_cur].as<float>(),
                     ctx->rs_d_noise.as<float>(), static_cast<int>(n), ctx->pose.as<float>());
  HIP_TRY(hipGetLastError());
  pose_mirror_stamp(ctx, n);
  return sync_stream(ctx);
}
}  // namespace

int mcl3dl_hip_group_add_noise(mcl3dl_hip_group* g, const float* noise13, size_t n_p)
{
  if (!g)
    return -1;
  if (!noise13)
    return g->fail(-3, "null noise array");
  if (g->n_resident == 0 || g->n_resident != n_p)
    return g->fail(-5, "%zu particles are resident, %zu noise states given", g->n_resident, n_p);
  const int rc = group_each_shard(g,
                                  [&](mcl3dl_hip_ctx* ctx, int, size_t lo, size_t n) -> int
                                  {
                                    TRY(ensure(ctx, ctx->rs_d_noise, sizeof(float) * 13 * n));
                                    TRY(h2d(ctx, ctx->rs_d_noise.p, noise13 + 13 * lo, sizeof(float) * 13 * n));
                                    return add_noise_launch(ctx, n);
                                  });
  // operator+ returns a fresh State6DOF: every particle's odometry noise is 0 now (the node redraws it after the next scan)
  g->noise_on = false;
  return rc;
}

int mcl3dl_hip_group_set_odom_error_sigma(mcl3dl_hip_group* g, float sigma)
{
  if (!g)
    return -1;
  if (!(sigma >= 0.f) || std::isinf(sigma))
    return g->fail(-3, "odometry error sigma must be finite and >= 0 (0 = no factor)");
  g->odom_sigma = sigma;
  return 0;
}

namespace
{
// What a likelihood model does on one shard ahead of pf::measure, ctx->lik holding room for the shard's n likelihoods: either
// it fills *imu (the likelihood is then formed inside the partial-sum pass) or it enqueues a launch of its own that writes
// ctx->lik and points *lik there.
using ShardModel = std::function<int(mcl3dl_hip_ctx*, size_t, const float**, ImuGravity*)>;

// pf::measure (pf.h:252-279) over the resident particles with the likelihoods of `model`: one device — the fused work-group up
// to PF_FUSED_MAX_PARTICLES particles, else partial + apply; N shards — the round of mcl3dl_hip_group_update_resident
// (group_allreduce_record: partial sums, the 2 + 2N-double record summed, apply). `what` names the update in error texts.
int group_measure_resident(mcl3dl_hip_group* g, const char* what, const ShardModel& model, float* out_weight, float* out_lik,
                           float* entropy, int* restored)
{
  const size_t n_p = g->n_resident;
  const int N = g->n();
  std::vector<float> stats(4 * static_cast<size_t>(N), 0.f);
  // the results of a rank home
  const auto fetch = [&](const Shard& s) -> int
  {
    mcl3dl_hip_ctx* ctx = s.ctx;
    TRY(d2h(ctx, &stats[4 * s.r], ctx->stats4.p, sizeof(float) * 4));
    if (out_weight)
      TRY(d2h(ctx, out_weight + s.lo, ctx->gs_weight.p, sizeof(float) * s.n));
    if (out_lik)
      TRY(d2h(ctx, out_lik + s.lo, ctx->lik.p, sizeof(float) * s.n));
    return sync_stream(ctx);
  };
  if (g->route() == ROUTE_DIRECT)
    // one device: pf::measure as mcl3dl_hip_group_update_resident's single-GPU form runs it (pf_one_gpu: the fused
    // work-group up to PF_FUSED_MAX_PARTICLES particles, else partial + apply), the likelihood formed inside — one or two launches
    TRY(group_forward(
        g,
        [&](mcl3dl_hip_ctx* ctx, int) -> int
        {
          HIP_TRY(hipSetDevice(ctx->device));
          TRY(rank_holds(ctx, n_p));
          TRY(ensure(ctx, ctx->lik, sizeof(float) * n_p));
          TRY(ensure(ctx, ctx->partial4, sizeof(double) * 4));
          TRY(ensure(ctx, ctx->stats4, sizeof(float) * 4));
          ImuGravity m{};
          const float* d_lik = nullptr;
          TRY(model(ctx, n_p, &d_lik, &m));
          // (the first kernel reads the likelihoods only)
          PfCall c{ ctx, ctx->gs_weight.as<float>(), const_cast<float*>(d_lik), nullptr, nullptr, nullptr, n_p,
                    ctx->stats4.as<float>() };
          c.model = &m;
          TRY(pf_one_gpu(c));
          return fetch(Shard{ ctx, 0, 0, n_p });
        }));
  else
    TRY(group_allreduce_record(
        g, what, n_p,
        [&](const Shard& s) -> int
        {
          mcl3dl_hip_ctx* ctx = s.ctx;
          TRY(ensure(ctx, ctx->stats4, sizeof(float) * 4));
          if (s.n == 0)
            return pf_first_half_empty(ctx, s.r, N, ctx->packed.as<double>());
          TRY(rank_holds(ctx, s.n));
          TRY(ensure(ctx, ctx->lik, sizeof(float) * s.n));
          ImuGravity m{};
          const float* d_lik = nullptr;
          TRY(model(ctx, s.n, &d_lik, &m));
          PfCall c{ ctx, ctx->gs_weight.as<float>(), const_cast<float*>(d_lik), nullptr, nullptr, nullptr, s.n, nullptr };
          c.model = &m;
          c.timed = false;
          return pf_first_half(c, s.r, N, ctx->packed.as<double>());
        },
        [&](const Shard& s) -> int
        {
          if (s.n == 0)
            return sync_stream(s.ctx);
          PfCall c{ s.ctx, s.ctx->gs_weight.as<float>(), nullptr, nullptr, nullptr, nullptr, s.n, s.ctx->stats4.as<float>() };
          c.timed = false;
          TRY(pf_second_half(c, N, s.ctx->packed.as<double>()));
          return fetch(s);
        }));
  // every rank computed the same scalars from the same record; rank 0 always holds a particle
  unpack_stats4(&stats[0], entropy, nullptr, nullptr, restored);
  return 0;
}
}  // namespace

int mcl3dl_hip_group_measure_imu(mcl3dl_hip_group* g, const float* acc3, float acc_var, float* out_weight, float* out_lik,
                                 float* entropy, int* restored)
{
  if (!g)
    return -1;
  if (!acc3)
    return g->fail(-3, "null acceleration");
  TRY(group_resident(g));
  // ImuMeasurementModelGravity(acc_var) + setAccMeasure(acc) (imu_measurement_model_gravity.h:41-48)
  ImuGravity imu{};
  imu.acc = Vec3f{ acc3[0], acc3[1], acc3[2] };
  imu.acc_norm = std::sqrt(vdot(imu.acc, imu.acc));
  normal_likelihood_constants(acc_var, &imu.a, &imu.sq2);
  return group_measure_resident(
      g, "IMU update",
      [&](mcl3dl_hip_ctx* ctx, size_t, const float**, ImuGravity* m) -> int
      {
        *m = imu;
        m->state13 = ctx->gs_state[ctx->gs_cur].as<float>();
        m->lik_out = ctx->lik.as<float>();
        return 0;
      },
      out_weight, out_lik, entropy, restored);
}

namespace
{
// NormalLikelihoodNd<float, 6>'s constructor (nd.h:67-71) on sigma(r, c) = (float)cov36[6 * c + r]: determinant and inverse of
// the FLOAT matrix by LU with partial pivoting in double (Doolittle, rows swapped for the largest |pivot|, the first of equals),
// each rounded to float once — Eigen's own float LU is not pinned by the reference ("What is not reproduced").
// false: a non-finite entry, a zero pivot, det <= 0 or NaN, or a non-finite inverse.
bool landmark_normal_constants(const double* cov36, float* a, float* sinv36)
{
  double A[6][6];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c)
    {
      if (!std::isfinite(cov36[6 * c + r]))
        return false;
      const float f = static_cast<float>(cov36[6 * c + r]);
      if (!std::isfinite(f))
        return false;
      A[r][c] = static_cast<double>(f);
    }
  int perm[6] = { 0, 1, 2, 3, 4, 5 };
  double det = 1.0;
  for (int k = 0; k < 6; ++k)
  {
    int p = k;
    for (int i = k + 1; i < 6; ++i)
      if (std::fabs(A[i][k]) > std::fabs(A[p][k]))
        p = i;
    if (A[p][k] == 0.0)
      return false;
    if (p != k)
    {
      for (int j = 0; j < 6; ++j)
        std::swap(A[k][j], A[p][j]);
      std::swap(perm[k], perm[p]);
      det = -det;
    }
    for (int i = k + 1; i < 6; ++i)
    {
      A[i][k] = A[i][k] / A[k][k];
      for (int j = k + 1; j < 6; ++j)
        A[i][j] = A[i][j] - A[i][k] * A[k][j];
    }
  }
  for (int k = 0; k < 6; ++k)
    det = det * A[k][k];
  const float det_f = static_cast<float>(det);
  if (!(det_f > 0.0f))
    return false;
  for (int c = 0; c < 6; ++c)
  {
    double y[6], x[6];
    for (int i = 0; i < 6; ++i)
    {
      double s = perm[i] == c ? 1.0 : 0.0;
      for (int j = 0; j < i; ++j)
        s = s - A[i][j] * y[j];
      y[i] = s;
    }
    for (int i = 5; i >= 0; --i)
    {
      double s = y[i];
      for (int j = i + 1; j < 6; ++j)
        s = s - A[i][j] * x[j];
      x[i] = s / A[i][i];
    }
    for (int r = 0; r < 6; ++r)
    {
      sinv36[6 * r + c] = static_cast<float>(x[r]);
      if (!std::isfinite(sinv36[6 * r + c]))
        return false;
    }
  }
  // a_ = 1.0 / (pow(2 pi, 0.5 * 6) * sqrt(det)) (nd.h:69): the square root of a float is a float; det_f = inf gives a_ = 0
  *a = static_cast<float>(1.0 / (std::pow(2.0 * M_PI, 3.0) * static_cast<double>(std::sqrt(det_f))));
  return true;
}
}  // namespace

int mcl3dl_hip_group_measure_landmark(mcl3dl_hip_group* g, const float* measured7, const double* cov36, float* out_weight,
                                      float* out_lik, float* entropy, int* restored)
{
  if (!g)
    return -1;
  if (!measured7 || !cov36)
    return g->fail(-3, "null landmark pose / covariance");
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(measured7[k]))
      return g->fail(-3, "non-finite landmark pose");
  TRY(group_resident(g));
  LandmarkModel lm{};
  if (!landmark_normal_constants(cov36, &lm.a, lm.sinv))
    return g->fail(-3, "landmark covariance: non-finite, singular or without a positive determinant");
  lm.pos = Vec3f{ measured7[0], measured7[1], measured7[2] };
  lm.rot_inv = qinv(Quat{ measured7[3], measured7[4], measured7[5], measured7[6] });
  return group_measure_resident(
      g, "landmark update",
      [&](mcl3dl_hip_ctx* ctx, size_t n, const float** lik, ImuGravity*) -> int
      {
        hipLaunchKernelGGL(landmark_likelihood_kernel, grid_of(n), dim3(256), 0, ctx->stream,
                           ctx->gs_state[ctx->gs_cur].as<float>(), static_cast<int>(n), lm, ctx->lik.as<float>());
        HIP_TRY(hipGetLastError());
        *lik = ctx->lik.as<float>();
        return 0;
      },
      out_weight, out_lik, entropy, restored);
}
