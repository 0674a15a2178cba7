// api_rng.inl — included inside the extern "C" block of mcl3dl_hip.hip after api_group_motion.inl: the filter's noise drawn ON THE
// DEVICES from the reference's engine (rng_polar.h: libstdc++'s minstd_rand0 + normal_distribution<float>, restated per attempt;
// host_rng.h: the rounds). Each call equals its counterpart fed with the host-drawn array — the same kernels behind the noise
// buffer, the same pose-mirror refresh, the same noise_on bookkeeping — and leaves *engine_state where the reference's engine_
// would stand.
//
//   mcl3dl_hip_rng_seed / _rng_uniform          engine(seed) / uniform_real_distribution<float>(a, b)(engine): host arithmetic
//   mcl3dl_hip_group_add_noise_drawn            pf::noise (pf.h:226-237)
//   mcl3dl_hip_group_init_drawn                 pf::init (pf.h:169-181)
//   mcl3dl_hip_noise_transform6                 MultivariateNoiseGenerator::setCovariance (noise_transform.h), on the host
//   mcl3dl_hip_group_init_drawn_multivariate    cbPosition's initUsingNoiseGenerator + integ_reset_func (src/mcl_3dl.cpp:186-195)
//   mcl3dl_hip_group_draw_odom_noise            update_noise_func (src/mcl_3dl.cpp:817-825)
//   mcl3dl_hip_group_resample_apply_drawn       pf::resample's generateNoise per duplicated slot, in slot order (pf.h:216)
namespace
{
// DiagonalNoiseGenerator(mean, sigma) for State6DOF; mean6 == null: State6DOF(). The engine state it will draw from is checked too.
int rng_generator(mcl3dl_hip_group* g, const float* mean6, const float* sigma6, const uint32_t* engine_state, rng::NoiseGen6* gen)
{
  if (!sigma6)
    return g->fail(-3, "null sigma6");
  gen->dims = 0;
  for (int k = 0; k < 6; ++k)
  {
    if (!std::isfinite(sigma6[k]) || sigma6[k] < 0.f)
      return g->fail(-3, "sigma6[%d] must be finite and >= 0", k);
    gen->sigma[k] = sigma6[k];
    gen->mean[k] = mean6 ? mean6[k] : 0.0f;
    gen->dims += sigma6[k] != 0.f ? 1 : 0;
  }
  return rng_check_state(g, engine_state);
}

// every rank that drew ran the same count pass over the same stream: one engine state
int rng_hand_back(mcl3dl_hip_group* g, const std::vector<uint32_t>& states, const std::vector<char>& drew,
                  uint32_t* engine_state)
{
  TRY(group_agree(g, "the engine state behind the draw", states.data(), 1, drew.data()));
  if (drew[0])
    *engine_state = states[0];
  return 0;
}
}  // namespace

uint32_t mcl3dl_hip_rng_seed(uint32_t seed)
{
  return rng::minstd_seed(seed);
}

float mcl3dl_hip_rng_uniform(uint32_t* state, float a, float b)
{
  if (!state || *state < 1u || *state > rng::MINSTD_M - 1u)
    return std::numeric_limits<float>::quiet_NaN();
  return rng::uniform_draw(state, a, b);
}

int mcl3dl_hip_group_add_noise_drawn(mcl3dl_hip_group* g, const float* sigma6, uint32_t* engine_state)
{
  if (!g)
    return -1;
  rng::NoiseGen6 gen;
  TRY(rng_generator(g, nullptr, sigma6, engine_state, &gen));
  const size_t n_p = g->n_resident;
  std::vector<uint32_t> states(g->n(), 0u);
  std::vector<char> drew(g->n(), 0);
  const uint32_t x0 = *engine_state;
  const int rc = group_each_shard(g,
                                  [&](mcl3dl_hip_ctx* ctx, int r, size_t lo, size_t n) -> int
                                  {
                                    TRY(ensure(ctx, ctx->rs_d_noise, sizeof(float) * 13 * n));
                                    TRY(rng_noise_rows(ctx, x0, gen, n_p, lo, n, ctx->rs_d_noise.as<float>(), &states[r]));
                                    drew[r] = 1;
                                    return add_noise_launch(ctx, n);
                                  });
  if (n_p)
    g->noise_on = false;  // as mcl3dl_hip_group_add_noise: operator+ returns a fresh State6DOF
  if (rc)
    return rc;
  return rng_hand_back(g, states, drew, engine_state);
}

int mcl3dl_hip_group_draw_odom_noise(mcl3dl_hip_group* g, const float* odom_err4, uint32_t* engine_state)
{
  if (!g)
    return -1;
  if (!odom_err4)
    return g->fail(-3, "null odom_err4");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(odom_err4[k]))
      return g->fail(-3, "odom_err4[%d] is not finite", k);
  TRY(rng_check_state(g, engine_state));
  const size_t n_p = g->n_resident;
  const int N = g->n();
  std::vector<uint32_t> states(N, 0u);
  std::vector<char> drew(N, 0);
  const uint32_t x0 = *engine_state;
  const int rc = group_each_shard(
      g,
      [&](mcl3dl_hip_ctx* ctx, int r, size_t lo, size_t n) -> int
      {
        TRY(odom_noise_room(ctx, n_p, N));
        // one shared normal_distribution: accepted attempt k yields values 2k and 2k + 1, four values per particle
        TRY(rng_draw(ctx, x0, 2 * static_cast<uint64_t>(n_p), true, 2 * static_cast<uint64_t>(lo),
                     2 * static_cast<uint64_t>(lo + n), &states[r]));
        drew[r] = 1;
        hipLaunchKernelGGL(rng::rng_odom_noise_kernel, grid_of(n), dim3(256), 0, ctx->stream, ctx->rng_values.as<float>(),
                           odom_err4[0], odom_err4[1], odom_err4[2], odom_err4[3], static_cast<int>(n),
                           ctx->gs_noise[ctx->gs_cur].as<float>());
        HIP_TRY(hipGetLastError());
        return sync_stream(ctx);
      });
  if (rc)
  {
    if (n_p)
      g->noise_on = false;  // (some shards may hold the new noise, others none: the caller draws it again)
    return rc;
  }
  // an empty shard still needs its buffer for the all-gather
  const int rc_e = group_forward(g,
                                 [&](mcl3dl_hip_ctx* ctx, int r) -> int
                                 {
                                   if (drew[r])
                                     return 0;
                                   HIP_TRY(hipSetDevice(ctx->device));
                                   return odom_noise_room(ctx, n_p, N);
                                 });
  if (rc_e)
  {
    g->noise_on = false;
    return rc_e;
  }
  TRY(rng_hand_back(g, states, drew, engine_state));
  g->noise_on = true;
  return 0;
}

int mcl3dl_hip_group_init_drawn(mcl3dl_hip_group* g, const float* mean7, const float* sigma6, size_t n_p, uint32_t* engine_state)
{
  if (!g)
    return -1;
  if (!mean7)
    return g->fail(-3, "null mean7");
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(mean7[k]))
      return g->fail(-3, "mean7[%d] is not finite", k);
  float mean6[6];
  rng_mean6(mean7, mean6);
  rng::NoiseGen6 gen;
  TRY(rng_generator(g, mean6, sigma6, engine_state, &gen));
  if (n_p == 0 || n_p > 0x7fffffffu / 16)
    return g->fail(-3, "init_drawn: %zu particles asked for", n_p);
  generation_begin(g);
  const int N = g->n();
  std::vector<uint32_t> states(N, 0u);
  std::vector<char> drew(N, 0);
  const uint32_t x0 = *engine_state;
  const float weight = static_cast<float>(1.0 / static_cast<double>(n_p));  // pf.h:179
  TRY(group_run_shards(g, n_p,
                       [&](const Shard& s) -> int
                       {
                         mcl3dl_hip_ctx* ctx = s.ctx;
                         TRY(generation_rank_begin(ctx, n_p, N));
                         if (s.n == 0)
                           return 0;
                         // p.state_ = generateNoise(engine_, generator): the row IS the state
                         TRY(rng_noise_rows(ctx, x0, gen, n_p, s.lo, s.n, ctx->gs_state[0].as<float>(), &states[s.r]));
                         drew[s.r] = 1;
                         TRY(uniform_weights(ctx, s.n, weight));
                         TRY(generation_rank_installed(ctx, s.n, false));
                         return sync_stream(ctx);
                       }));
  TRY(rng_hand_back(g, states, drew, engine_state));
  generation_installed(g, n_p);
  return 0;
}

int mcl3dl_hip_noise_transform6(const double* cov36, float* transform36, float* eigenvalues6)
{
  char msg[192] = "";
  const int rc = noise_transform6(cov36, transform36, eigenvalues6, nullptr, msg, sizeof(msg));
  if (rc)
    fprintf(stderr, "mcl3dl_hip_noise_transform6: %s\n", msg);  // no handle to keep the message in
  return rc;
}

int mcl3dl_hip_group_init_drawn_multivariate(mcl3dl_hip_group* g, const float* mean7, const float* transform36, size_t n_p,
                                             int reset_odom_integ, uint32_t* engine_state)
{
  if (!g)
    return -1;
  if (!mean7)
    return g->fail(-3, "null mean7");
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(mean7[k]))
      return g->fail(-3, "mean7[%d] is not finite", k);
  if (!transform36)
    return g->fail(-3, "null transform36");
  rng::NoiseGenFull6 gen;
  for (int k = 0; k < 36; ++k)
  {
    if (!std::isfinite(transform36[k]))
      return g->fail(-3, "transform36[%d] is not finite", k);
    gen.t[k] = transform36[k];
  }
  rng_mean6(mean7, gen.mean);
  TRY(rng_check_state(g, engine_state));
  if (n_p == 0 || n_p > 0x7fffffffu / 16)
    return g->fail(-3, "init_drawn_multivariate: %zu particles asked for", n_p);
  if (reset_odom_integ != 0 && reset_odom_integ != 1)
    return g->fail(-3, "reset_odom_integ must be 0 or 1, not %d", reset_odom_integ);
  gen.reset_odom_integ = reset_odom_integ;
  generation_begin(g);
  const int N = g->n();
  std::vector<uint32_t> states(N, 0u);
  std::vector<char> drew(N, 0);
  const uint32_t x0 = *engine_state;
  const float weight = static_cast<float>(1.0 / static_cast<double>(n_p));  // pf.h:179
  TRY(group_run_shards(g, n_p,
                       [&](const Shard& s) -> int
                       {
                         mcl3dl_hip_ctx* ctx = s.ctx;
                         TRY(generation_rank_begin(ctx, n_p, N));
                         if (s.n == 0)
                           return 0;
                         TRY(rng_multivariate_rows(ctx, x0, gen, n_p, s.lo, s.n, ctx->gs_state[0].as<float>(), &states[s.r]));
                         drew[s.r] = 1;
                         TRY(uniform_weights(ctx, s.n, weight));
                         TRY(generation_rank_installed(ctx, s.n, false));
                         return sync_stream(ctx);
                       }));
  TRY(rng_hand_back(g, states, drew, engine_state));
  generation_installed(g, n_p);
  return 0;
}

int mcl3dl_hip_group_resample_apply_drawn(mcl3dl_hip_group* g, const float* sigma6, uint32_t* engine_state)
{
  if (!g)
    return -1;
  rng::NoiseGen6 gen;
  TRY(rng_generator(g, nullptr, sigma6, engine_state, &gen));
  TRY(group_resident(g));
  if (!g->rs_planned)
    return g->fail(-5, "group_resample_apply_drawn before group_resample_plan");
  const size_t n_dup = g->rs_n_dup, n_out = g->rs_n_out;
  std::vector<uint32_t> states(g->n(), 0u);
  std::vector<char> drew(g->n(), 0);
  const uint32_t x0 = *engine_state;
  const ShardNoise drawn = [&](mcl3dl_hip_ctx* ctx, int r, size_t olo, size_t n_new) -> int
  {
    // the duplicates among this rank's slots are rows [d_lo, d_hi) of the n_dup the reference draws in slot order: the
    // exclusive scan of the duplicate flags is still where resample_plan left it
    uint32_t d_lo = 0, d_hi = 0;
    TRY(d2h(ctx, &d_lo, ctx->rs_d_flag.as<uint32_t>() + olo, sizeof(uint32_t)));
    TRY(d2h(ctx, &d_hi, ctx->rs_d_flag.as<uint32_t>() + olo + n_new, sizeof(uint32_t)));
    TRY(sync_stream(ctx));
    if (d_lo > d_hi || d_hi > n_dup || olo + n_new > n_out)
      return ctx->fail(-4, "internal: duplicate rows [%u, %u) of %zu", d_lo, d_hi, n_dup);
    // resample_apply_kernel indexes the rows by their global number
    TRY(ensure(ctx, ctx->rs_d_noise, sizeof(float) * 13 * n_dup));
    if (d_hi == d_lo && r != 0)
      return 0;
    TRY(rng_noise_rows(ctx, x0, gen, n_dup, d_lo, d_hi - d_lo, ctx->rs_d_noise.as<float>() + 13 * static_cast<size_t>(d_lo),
                       &states[r]));
    drew[r] = 1;
    return 0;
  };
  TRY(group_resample_apply_impl(g, nullptr, 0, &drawn));
  return rng_hand_back(g, states, drew, engine_state);
}

// Replaces: all of pf::resample(sigma) (pf.h:187-225) on the resident particles — group_resample_begin(0), rng_uniform(state, 0,
// pstep), group_resample_plan(0, initial_p), group_resample_apply_drawn(sigma6, state) — with nothing but the engine state going
// in and coming out: prefixes, pstep and initial_p are formed on the devices (api_group_state.inl: group_plan_device).
int mcl3dl_hip_group_resample_drawn(mcl3dl_hip_group* g, const float* sigma6, uint32_t* engine_state, float* out_pstep,
                                    float* out_initial_p, size_t* out_n_duplicates, int* out_route)
{
  if (!g)
    return -1;
  rng::NoiseGen6 gen;
  TRY(rng_generator(g, nullptr, sigma6, engine_state, &gen));
  TRY(group_resident(g));
  GroupPlan plan;
  TRY(group_plan_device(g, g->n_resident, 0, *engine_state, &plan));
  uint32_t state = plan.state;  // behind initial_p's engine call
  TRY(mcl3dl_hip_group_resample_apply_drawn(g, sigma6, &state));
  *engine_state = state;
  if (out_pstep)
    *out_pstep = plan.pstep;
  if (out_initial_p)
    *out_initial_p = plan.initial_p;
  if (out_n_duplicates)
    *out_n_duplicates = plan.n_dup;
  if (out_route)
    *out_route = plan.route;
  return 0;
}

// Replaces: `count` calls of std::uniform_int_distribution<size_t>(0, range - 1)(engine_) — PointCloudUniformSampler::sample's
// draws (point_cloud_uniform_sampler.h:66-71) on their own, for introspection and general use. The rounds form of
// rng_index_kernels.h; the indices come home.
int mcl3dl_hip_rng_draw_indices(mcl3dl_hip_ctx* ctx, uint64_t range, size_t count, uint32_t* engine_state, uint32_t* out_idx)
{
  if (!ctx)
    return -1;
  if (range < 1 || range > rng::INDEX_MAX_RANGE)
    return ctx->fail(-3, "range %llu is outside [1, 2147483646]", static_cast<unsigned long long>(range));
  TRY(rng_check_state(ctx, engine_state));
  if (count > 0x7fffffffu)
    return ctx->fail(-3, "count %zu is more than one call draws", count);
  if (count && !out_idx)
    return ctx->fail(-3, "null out_idx");
  if (count == 0)
    return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(ensure(ctx, ctx->rng_values, sizeof(uint32_t) * count));
  uint32_t state = *engine_state;
  TRY(rng_index_rounds(ctx, state, rng::index_range(range), count, ctx->rng_values.as<uint32_t>(), &state));
  TRY(d2h(ctx, out_idx, ctx->rng_values.p, sizeof(uint32_t) * count));
  TRY(sync_stream(ctx));
  *engine_state = state;
  return 0;
}
