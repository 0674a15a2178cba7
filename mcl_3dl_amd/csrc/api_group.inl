// api_group.inl — included inside the extern "C" block of mcl3dl_hip.hip: the device group (host_group.h) behind the C ABI.
int mcl3dl_hip_group_create(mcl3dl_hip_group** out, const int* device_ids, int n_devices)
{
  if (!out)
    return -1;
  *out = nullptr;
  if (!device_ids || n_devices < 1 || n_devices > ROUND_MAX_RANKS)
    return -3;
  mcl3dl_hip_group* g = new mcl3dl_hip_group;
  for (int r = 0; r < n_devices; ++r)
  {
    mcl3dl_hip_ctx* c = nullptr;
    const int rc = mcl3dl_hip_create(&c, device_ids[r]);
    if (rc != 0)
    {
      for (mcl3dl_hip_ctx* p : g->ctx)
        mcl3dl_hip_destroy(p);
      delete g;
      return rc;
    }
    for (int q = 0; q < r; ++q)
      if (device_ids[q] == device_ids[r])
        g->devices_distinct = false;
    g->ctx.push_back(c);
    g->devices.push_back(device_ids[r]);
  }
  const char* env = getenv("MCL3DL_HIP_COLLECTIVE");
  if (env && std::string(env) == "host")
    g->collective = 1;
  g->host_packed.resize(n_devices);
  if (n_devices > 1)
    g->pool.start(n_devices);
  g->vote.resize(n_devices);
  *out = g;
  return 0;
}

void mcl3dl_hip_group_destroy(mcl3dl_hip_group* g)
{
  if (!g)
    return;
  g->pool.stop();
  for (mcl3dl_hip_ctx* c : g->ctx)
  {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
  }
  for (ncclComm_t c : g->comms)
    if (c)
      (void)g->rccl.CommDestroy(c);
  g->comms.clear();
  for (mcl3dl_hip_ctx* c : g->ctx)
    mcl3dl_hip_destroy(c);
  delete g;
}

const char* mcl3dl_hip_group_last_error(const mcl3dl_hip_group* g)
{
  return g ? g->err.c_str() : "null group";
}

int mcl3dl_hip_group_size(const mcl3dl_hip_group* g)
{
  return g ? g->n() : 0;
}

mcl3dl_hip_ctx* mcl3dl_hip_group_context(mcl3dl_hip_group* g, int rank)
{
  return (g && rank >= 0 && rank < g->n()) ? g->ctx[rank] : nullptr;
}

int mcl3dl_hip_group_shard(size_t n_p, int n_devices, int rank, size_t* begin, size_t* count)
{
  if (n_devices < 1 || rank < 0 || rank >= n_devices || !begin || !count)
    return -3;
  size_t lo, hi;
  shard_bounds(n_p, n_devices, rank, &lo, &hi);
  *begin = lo;
  *count = hi - lo;
  return 0;
}

int mcl3dl_hip_group_set_map(mcl3dl_hip_group* g, const float* xyz, const uint32_t* label, size_t n_m, uint64_t stamp,
                             const float* dist_weight)
{
  if (!g)
    return -1;
  return group_run(g, [&](int r) { return mcl3dl_hip_set_map(g->ctx[r], xyz, label, n_m, stamp, dist_weight); });
}

int mcl3dl_hip_group_set_likelihood_params(mcl3dl_hip_group* g, float match_dist_min, float match_dist_flat,
                                           float match_weight)
{
  if (!g)
    return -1;
  return group_forward(g, [&](mcl3dl_hip_ctx* ctx, int)
                       { return mcl3dl_hip_set_likelihood_params(ctx, match_dist_min, match_dist_flat, match_weight); });
}

int mcl3dl_hip_group_set_beam_params(mcl3dl_hip_group* g, float map_grid_x, float map_grid_y, float map_grid_z,
                                     float dda_grid_size, float ray_angle_half, float hit_range,
                                     float beam_likelihood_min, uint32_t num_points, float ang_total_ref,
                                     uint32_t filter_label_max, int add_penalty_short_only_mode)
{
  if (!g)
    return -1;
  return group_forward(g,
                       [&](mcl3dl_hip_ctx* ctx, int)
                       {
                         return mcl3dl_hip_set_beam_params(ctx, map_grid_x, map_grid_y, map_grid_z, dda_grid_size, ray_angle_half,
                                                           hit_range, beam_likelihood_min, num_points, ang_total_ref,
                                                           filter_label_max, add_penalty_short_only_mode);
                       });
}

int mcl3dl_hip_group_set_beam_raycast(mcl3dl_hip_group* g, int mode)
{
  if (!g)
    return -1;
  return group_forward(g, [&](mcl3dl_hip_ctx* ctx, int) { return mcl3dl_hip_set_beam_raycast(ctx, mode); });
}

int mcl3dl_hip_group_set_option(mcl3dl_hip_group* g, const char* name, double value)
{
  if (!g || !name)
    return -1;
  if (std::string(name) == "collective")
  {
    if (value != 0.0 && value != 1.0)
      return g->fail(-3, "collective must be 0 (RCCL all-reduce) or 1 (host combine)");
    g->collective = static_cast<int>(value);
    return 0;
  }
  if (std::string(name) == "direct_single")
  {
    g->direct_single = value != 0.0;
    return 0;
  }
  if (std::string(name) == "inject_failure_rank")
  {
    // test hook (only with MCL3DL_HIP_TEST_HOOKS=1 in the environment): the next sharded call that enters a collective fails on
    // that rank after its kernels are enqueued and before the collective (group_voted_call)
    if (!test_hooks_enabled())
      return g->fail(-3, "inject_failure_rank is a test hook: set MCL3DL_HIP_TEST_HOOKS=1 in the environment to enable it");
    g->inject_failure_rank = static_cast<int>(value);
    return 0;
  }
  return group_forward(g, [&](mcl3dl_hip_ctx* ctx, int) { return mcl3dl_hip_set_option(ctx, name, value); });
}

int mcl3dl_hip_group_collective_stats(const mcl3dl_hip_group* g, uint64_t* rccl_all_reduces, uint64_t* host_combines)
{
  if (!g)
    return -1;
  if (rccl_all_reduces)
    *rccl_all_reduces = g->collectives_rccl;
  if (host_combines)
    *host_combines = g->collectives_host;
  return 0;
}

int mcl3dl_hip_group_upload_poses(mcl3dl_hip_group* g, const float* pose, size_t n_p)
{
  if (!g)
    return -1;
  if (!pose || n_p == 0 || n_p > 0x7fffffffu)
    return g->fail(-3, "bad pose array");
  g->n_pose_uploaded = 0;
  TRY(group_run_shards(g, n_p,
                       [&](const Shard& s) -> int
                       {
                         s.ctx->poses_set(0);
                         if (s.n == 0)
                           return 0;
                         return mcl3dl_hip_upload_poses(s.ctx, pose + 7 * s.lo, s.n);
                       }));
  g->n_pose_uploaded = n_p;
  return 0;
}

int mcl3dl_hip_group_measure_batch(mcl3dl_hip_group* g, const float* pose, size_t n_p, const float* scan_lik_xyz,
                                   size_t n_s, const float* scan_beam_xyz, const uint32_t* scan_beam_origin, size_t n_b,
                                   const float* origins, size_t n_o, float* out_lik, float* out_match_ratio,
                                   float* out_beam)
{
  if (!g)
    return -1;
  if (n_p == 0)
    return 0;
  if (!pose && g->n_pose_uploaded != n_p)
    return g->fail(-3, "null pose array (and mcl3dl_hip_group_upload_poses holds %zu poses, not %zu)", g->n_pose_uploaded,
                   n_p);
  if (g->route() == ROUTE_DIRECT)
    return group_forward(g, [&](mcl3dl_hip_ctx* ctx, int) {
      return mcl3dl_hip_measure_batch(ctx, pose, n_p, scan_lik_xyz, n_s, scan_beam_xyz, scan_beam_origin, n_b, origins, n_o,
                                      out_lik, out_match_ratio, out_beam);
    });
  const bool device_order = scan_ordered_on_device(g->ctx[0]->opt, n_s, n_b);
  const HostScan scan{ scan_lik_xyz, n_s, scan_beam_xyz, scan_beam_origin, n_b, origins, n_o };
  std::string err;
  if (!device_order && order_scan(err, scan, g->scan, g->ctx[0]->opt.scan_presorted != 0) != 0)
    return g->fail(-3, "%s", err.c_str());
  if (pose)
    g->n_pose_uploaded = 0;
  TRY(group_run_shards(
      g, n_p,
      [&](const Shard& s) -> int
      {
        mcl3dl_hip_ctx* ctx = s.ctx;
        if (device_order)
          TRY(upload_scan_impl(ctx, scan, false));
        else
          TRY(push_scan(ctx, g->scan, false));
        if (s.n == 0)
          return sync_stream(ctx);
        if (!pose && ctx->n_pose_uploaded != s.n)
          return ctx->fail(-3, "uploaded pose shard holds %zu poses, not %zu", ctx->n_pose_uploaded, s.n);
        return measure_batch_general(ctx, pose ? pose + 7 * s.lo : nullptr, s.n, s.lo, out_lik, out_match_ratio, out_beam);
      }));
  if (pose)
    g->n_pose_uploaded = n_p;
  return 0;
}

// Progressive form. One device: the context's own slices (api_core.inl). N devices (round 5): every
// rank takes its shard of the batch as a progressive batch of its own — poses, scans and kernels enqueued by its worker
// thread, nothing waited for — and the shards' results land in the caller's arrays shard by shard, slice by slice, through
// each rank's page-locked emission + polled completion word. _wait(particle) is answered by the rank that owns the particle
// (after the ranks in front of it: the reference's loop consumes the particles in order, pf.h:255-260), from the caller's
// thread; the other ranks keep computing. Results are those of mcl3dl_hip_group_measure_batch bit for bit.
int mcl3dl_hip_group_measure_batch_begin(mcl3dl_hip_group* g, const float* pose, size_t n_p, const float* scan_lik_xyz,
                                         size_t n_s, const float* scan_beam_xyz, const uint32_t* scan_beam_origin,
                                         size_t n_b, const float* origins, size_t n_o, float* out_lik,
                                         float* out_match_ratio, float* out_beam, size_t slice_particles)
{
  if (!g)
    return -1;
  TRY(mcl3dl_hip_group_measure_batch_end(g));  // (a batch still open is ended first, like the context form does)
  g->prog_n_p = 0;
  g->prog_direct = false;
  g->prog_sharded = false;
  if (!pose && n_p && g->n_pose_uploaded != n_p)
    return g->fail(-3, "null pose array (and mcl3dl_hip_group_upload_poses holds %zu poses, not %zu)", g->n_pose_uploaded,
                   n_p);
  if (g->route() == ROUTE_DIRECT)
  {
    TRY(group_forward(g, [&](mcl3dl_hip_ctx* ctx, int) {
      return mcl3dl_hip_measure_batch_begin(ctx, pose, n_p, scan_lik_xyz, n_s, scan_beam_xyz, scan_beam_origin, n_b, origins, n_o,
                                            out_lik, out_match_ratio, out_beam, slice_particles);
    }));
    g->prog_n_p = n_p;
    g->prog_direct = true;
    return 0;
  }
  if (n_p == 0)
    return 0;
  const int N = g->n();
  if (pose)
    g->n_pose_uploaded = 0;
  const int rc = group_run_shards(
      g, n_p,
      [&](const Shard& s) -> int
      {
        mcl3dl_hip_ctx* ctx = s.ctx;
        const size_t lo = s.lo, n = s.n;
        HIP_TRY(hipSetDevice(ctx->device));
        if (n == 0)
          return 0;
        // (the context form slices a shard of >= 1024 particles in four by default; shorter shards, and shards whose shape the
        // staged path does not take, are evaluated whole before this returns — they are short)
        return mcl3dl_hip_measure_batch_begin(ctx, pose ? pose + 7 * lo : nullptr, n, scan_lik_xyz, n_s, scan_beam_xyz,
                                              scan_beam_origin, n_b, origins, n_o, out_lik ? out_lik + lo : nullptr,
                                              out_match_ratio ? out_match_ratio + lo : nullptr,
                                              out_beam ? out_beam + lo : nullptr, slice_particles);
      });
  g->prog_done.assign(static_cast<size_t>(N), false);
  if (rc)
  {
    for (int r = 0; r < N; ++r)  // the other ranks' batches are drained before the caller gets control back
    {
      (void)hipSetDevice(g->ctx[r]->device);
      (void)mcl3dl_hip_measure_batch_end(g->ctx[r]);
    }
    return rc;
  }
  if (pose)
    g->n_pose_uploaded = n_p;
  g->prog_n_p = n_p;
  g->prog_sharded = true;
  return 0;
}

int mcl3dl_hip_group_measure_batch_wait(mcl3dl_hip_group* g, size_t particle, size_t* n_ready)
{
  if (!g)
    return -1;
  if (particle >= g->prog_n_p)
    return g->fail(-3, "particle %zu is not part of the batch (%zu particles)", particle, g->prog_n_p);
  if (g->prog_direct)
    return group_forward(g, [&](mcl3dl_hip_ctx* ctx, int) { return mcl3dl_hip_measure_batch_wait(ctx, particle, n_ready); });
  if (!g->prog_sharded)
  {
    if (n_ready)
      *n_ready = g->prog_n_p;
    return 0;
  }
  const int N = g->n();
  for (int r = 0; r < N; ++r)
  {
    const Shard s = shard_of(g, g->prog_n_p, r);
    if (s.n == 0)
      continue;
    mcl3dl_hip_ctx* ctx = s.ctx;
    const size_t lo = s.lo, hi = s.lo + s.n;
    if (particle >= hi)
    {
      // a rank in front of the owner: all of it must have arrived for the particles up to `particle` to be a leading run
      if (!g->prog_done[static_cast<size_t>(r)])
      {
        (void)hipSetDevice(ctx->device);
        const int rc = mcl3dl_hip_measure_batch_wait(ctx, hi - lo - 1, nullptr);
        if (rc)
          return g->fail_rank(rc, r);
        g->prog_done[static_cast<size_t>(r)] = true;
      }
      continue;
    }
    (void)hipSetDevice(ctx->device);
    size_t n = 0;
    const int rc = mcl3dl_hip_measure_batch_wait(ctx, particle - lo, &n);
    if (rc)
      return g->fail_rank(rc, r);
    if (n >= hi - lo)
      g->prog_done[static_cast<size_t>(r)] = true;
    if (n_ready)
      *n_ready = lo + n;
    return 0;
  }
  return g->fail(-3, "particle %zu belongs to no shard", particle);
}

int mcl3dl_hip_group_measure_batch_end(mcl3dl_hip_group* g)
{
  if (!g)
    return -1;
  if (g->prog_direct)
  {
    g->prog_direct = false;
    const int rc = mcl3dl_hip_measure_batch_end(g->ctx[0]);
    if (rc)
      return g->fail_rank(rc, 0);
  }
  if (g->prog_sharded)
  {
    g->prog_sharded = false;
    int first_rc = 0, first_r = 0;
    for (int r = 0; r < g->n(); ++r)
    {
      (void)hipSetDevice(g->ctx[r]->device);
      const int rc = mcl3dl_hip_measure_batch_end(g->ctx[r]);
      if (rc && !first_rc)
      {
        first_rc = rc;
        first_r = r;
      }
    }
    if (first_rc)
      return g->fail_rank(first_rc, first_r);
  }
  return 0;
}

namespace
{
int resident_poses(mcl3dl_hip_ctx* ctx);  // api_group_state.inl

// NormalLikelihood<float>(sigma)'s constants as nd.h:46-48 forms them: a_ from a double expression; sq2_ = (sigma * sigma) in
// float, * 2.0 in double, narrowed to float
void normal_likelihood_constants(float sigma, float* a, float* sq2)
{
  *a = static_cast<float>(1.0 / std::sqrt(2.0 * M_PI * sigma * sigma));
  *sq2 = static_cast<float>(sigma * sigma * 2.0);
}

// where an update's results go (null = not wanted). weight: for the non-resident update the prior weights on the way in
struct UpdateOutputs
{
  float* weight;
  float* lik;
  float* match_ratio;
  float* beam;
  float* entropy;
  float* match_ratio_min;
  float* match_ratio_max;
  int* restored;
};

// One update over the group's shards: its arguments and what its ranks share.
struct GroupUpdate
{
  mcl3dl_hip_group* g;
  bool resident, prepared;
  const float* pose;
  const float* extra;
  size_t n_p;
  HostScan scan;
  UpdateOutputs out;
  // Large scans are ordered by every device for itself (upload_scan_impl: raw points up, keys / stable radix sort / gather
  // there — the same order as the host's, bit for bit): N redundant sorts of ~0.05 ms that run side by side, instead of
  // 0.15 ms of one host core at 16 k points ahead of any GPU work. Small scans are ordered once on the host and pushed.
  bool device_order;
  // (a rank whose staging launch is not eligible and whose scan is small pushes a copy ordered ONCE on the host, by whichever
  // rank needs it first)
  std::once_flag host_order_once;
  std::string host_order_error;
  bool host_ordered = false;
  // the node's odometry factor formed on the devices from the resident states (mcl3dl_hip_group_set_odom_error_sigma)
  bool device_extra;
  float nd_a = 0.f, nd_sq2 = 0.f;
  std::vector<float*> rank_weights;  // where each rank's prior weights are on its device
  std::vector<float> stats;          // the four scalars of every rank
};

// phase A of a rank (group_allreduce_record): the shard and the scans go up, measure, the rank's partial sums
int update_phase_a(GroupUpdate& u, const Shard& s)
{
  mcl3dl_hip_group* g = u.g;
  mcl3dl_hip_ctx* ctx = s.ctx;
  const int N = g->n();
  const size_t lo = s.lo, n = s.n, fb = sizeof(float) * n;
  const bool resident = u.resident, prepared = u.prepared;
  const float* extra = u.extra;
  if (resident && n)
  {
    TRY(rank_holds(ctx, n));
    // ctx->pose is shared with the non-resident calls (uploads, mcl3dl_hip_group_measure_update, moments of explicit
    // states): whoever wrote it last, the poses evaluated here are those of the resident states
    TRY(resident_poses(ctx));
  }
  // ONE launch takes the rank's inputs over — the raw scans (every rank orders them for itself, side by side), its
  // pose / weight / odometry-factor shard — out of page-locked memory (stage_kernels.h); where that form is not
  // eligible: uploads + the ordering launches, or the scans ordered once on the host and pushed
  bool staged = false;
  if (n && !prepared)
  {
    const int st = stage_inputs(ctx, resident ? nullptr : u.pose + 7 * lo, extra ? extra + lo : nullptr,
                                resident ? nullptr : u.out.weight + lo, n, u.scan);
    if (st < 0)
      return st;
    staged = st != 0;
  }
  if (!staged && !prepared)
  {
    if (u.device_order)
      TRY(upload_scan_impl(ctx, u.scan, false));
    else
    {
      std::call_once(u.host_order_once,
                     [&]
                     {
                       u.host_ordered = order_scan(u.host_order_error, u.scan, g->scan, g->ctx[0]->opt.scan_presorted != 0) == 0;
                     });
      if (!u.host_ordered)
        return ctx->fail(-3, "%s", u.host_order_error.c_str());
      TRY(push_scan(ctx, g->scan, false));
    }
  }
  if (!resident && !staged)
    ctx->poses_set(0);
  if (n == 0)
    return pf_first_half_empty(ctx, s.r, N, ctx->packed.as<double>());
  TRY(ensure(ctx, ctx->lik, fb));
  TRY(ensure(ctx, ctx->ratio, fb));
  TRY(ensure(ctx, ctx->beam, fb));
  TRY(ensure(ctx, ctx->extra, fb));
  if (!resident && !staged)
  {
    TRY(ensure(ctx, ctx->weightb, fb));
    TRY(poses_upload(ctx, u.pose + 7 * lo, n));
    TRY(h2d(ctx, ctx->weightb.p, u.out.weight + lo, fb));
  }
  float* d_w = resident ? ctx->gs_weight.as<float>() : (staged ? staged_weights(ctx, n) : ctx->weightb.as<float>());
  u.rank_weights[s.r] = d_w;
  if (extra && !staged)
    TRY(h2d(ctx, ctx->extra.p, extra + lo, fb));
  if (u.device_extra)
  {
    hipLaunchKernelGGL(odom_factor_kernel, dim3((static_cast<int>(n) + 255) / 256), dim3(256), 0, ctx->stream,
                       ctx->gs_state[ctx->gs_cur].as<float>(), static_cast<int>(n), u.nd_a, u.nd_sq2, ctx->extra.as<float>());
    HIP_TRY(hipGetLastError());
  }
  // (the sum over the tiled kernel's per-tile partials and the beam model's last step ride in the first pf::measure kernel,
  // as on one GPU: one launch less per model and rank)
  LikTail tail;
  tail.want = pf_tiles_fit(n);
  tail.want_beam = true;
  TRY(launch_measure(ctx, ctx->pose.as<float>(), n, ctx->lik.as<float>(), ctx->ratio.as<float>(), ctx->beam.as<float>(), &tail));
  PfCall c{ ctx, d_w, ctx->lik.as<float>(), ctx->beam.as<float>(), (extra || u.device_extra) ? ctx->extra.as<float>() : nullptr,
            ctx->ratio.as<float>(), n, nullptr };
  c.tail = &tail;
  return pf_first_half(c, s.r, N, ctx->packed.as<double>());
}

// phase B of a rank: normalise with the total, the rank's results home
int update_phase_b(GroupUpdate& u, const Shard& s)
{
  mcl3dl_hip_ctx* ctx = s.ctx;
  const size_t lo = s.lo, n = s.n, fb = sizeof(float) * n;
  const UpdateOutputs& out = u.out;
  TRY(ensure(ctx, ctx->stats4, sizeof(float) * 4));
  if (n == 0)
    return sync_stream(ctx);
  float* d_w = u.rank_weights[s.r];
  // the normalising kernel writes the shard's results straight into page-locked memory (the caller's arrays where they
  // are page-locked, a staging block otherwise) and the rank learns of its completion from a polled word — instead of up
  // to five D2H copies and a hipStreamSynchronize per rank
  void* blk = (ctx->zero_copy() && ctx->poll_mode() && UpdBlock::bytes(n) <= STAGE_MAX_COPY) ? stage_alloc(ctx, UpdBlock::bytes(n)) :
                                                                                                nullptr;
  PfCall c{ ctx, d_w, ctx->lik.as<float>(), ctx->beam.as<float>(), nullptr, ctx->ratio.as<float>(), n, ctx->stats4.as<float>() };
  PfEmit e{};
  if (blk)
  {
    const UpdBlock ub(blk, n);
    e.stats4 = ub.stats4();
    ctx->stage_out.push_back({ &u.stats[4 * s.r], e.stats4, sizeof(float) * 4 });
    float* const user[4] = { out.weight, out.lik, out.match_ratio, out.beam };
    float** const slot[4] = { &e.w, &e.lik, &e.ratio, &e.beam };
    for (int k = 0; k < 4; ++k)
      if (user[k])
        *slot[k] = host_target(ctx, user[k] + lo, ub.part(k), fb, true);
    c.emit = &e;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(pf_second_half(c, u.g->n(), ctx->packed.as<double>()));
  if (blk)
    return sync_stream(ctx, true);
  if (out.weight)
    TRY(d2h(ctx, out.weight + lo, d_w, fb));
  TRY(d2h(ctx, &u.stats[4 * s.r], ctx->stats4.p, sizeof(float) * 4));
  float* const user[3] = { out.lik, out.match_ratio, out.beam };
  const float* const dev[3] = { ctx->lik.as<float>(), ctx->ratio.as<float>(), ctx->beam.as<float>() };
  TRY(models_home(ctx, user, dev, lo, n));
  return sync_stream(ctx);
}

// One update over the group's shards. resident = false: mcl3dl_hip_group_measure_update (poses and prior weights come from the
// host, the weights go back). resident = true: the particles mcl3dl_hip_group_upload_state / _resample_apply left on the
// devices (pose = first 7 floats of each 13-float state, kept as ctx->pose; weights in ctx->gs_weight, updated in place);
// out.weight is then an optional OUTPUT (may be null: nothing but four scalars comes back). prepared (with resident): every
// rank's scans are those mcl3dl_hip_group_scan_finish installed — nothing is taken over, the context's scan state is left alone
// (stage_inputs would record the scan it is given), an `extra` shard goes up by a plain copy.
int group_update_impl(mcl3dl_hip_group* g, bool resident, const float* pose, const float* extra, size_t n_p, const HostScan& scan,
                      const UpdateOutputs& out, bool prepared = false)
{
  if (resident)
    TRY(group_resident(g));
  if (n_p == 0)
    return g->fail(-3, "no particles");
  if (!resident && (!pose || !out.weight))
    return g->fail(-3, "null pose / weight array");
  if (resident && g->n_resident != n_p)
    return g->fail(-5, "%zu particles are resident on the group's devices, not %zu (mcl3dl_hip_group_upload_state first)",
                   g->n_resident, n_p);
  if (!resident && g->route() == ROUTE_DIRECT)
    return group_forward(g, [&](mcl3dl_hip_ctx* ctx, int) {
      return mcl3dl_hip_measure_update(ctx, pose, extra, out.weight, n_p, scan.scan_lik_xyz, scan.n_s, scan.scan_beam_xyz,
                                       scan.scan_beam_origin, scan.n_b, scan.origins, scan.n_o, out.lik, out.match_ratio, out.beam,
                                       out.entropy, out.match_ratio_min, out.match_ratio_max, out.restored);
    });
  const size_t N = static_cast<size_t>(g->n());
  GroupUpdate u{ g, resident, prepared, pose, extra, n_p, scan, out };
  u.device_order = scan_ordered_on_device(g->ctx[0]->opt, scan.n_s, scan.n_b);
  u.device_extra = resident && !extra && g->odom_sigma > 0.f;
  if (u.device_extra)
    normal_likelihood_constants(g->odom_sigma, &u.nd_a, &u.nd_sq2);
  u.rank_weights.assign(N, nullptr);
  u.stats.assign(4 * N, 0.f);
  if (!resident)
    g->n_pose_uploaded = 0;
  // the round of DESIGN.md, "One round for every collective"
  TRY(group_allreduce_record(
      g, "update", n_p, [&u](const Shard& s) { return update_phase_a(u, s); }, [&u](const Shard& s) { return update_phase_b(u, s); }));
  g->n_pose_uploaded = n_p;
  // (every rank computed the same scalars from the same record; rank 0 always holds a particle)
  unpack_stats4(&u.stats[0], out.entropy, out.match_ratio_min, out.match_ratio_max, out.restored);
  return 0;
}
}  // namespace

int mcl3dl_hip_group_measure_update(mcl3dl_hip_group* g, const float* pose, const float* extra, float* weight_inout,
                                    size_t n_p, const float* scan_lik_xyz, size_t n_s, const float* scan_beam_xyz,
                                    const uint32_t* scan_beam_origin, size_t n_b, const float* origins, size_t n_o,
                                    float* out_lik, float* out_match_ratio, float* out_beam, float* entropy,
                                    float* match_ratio_min, float* match_ratio_max, int* restored)
{
  if (!g)
    return -1;
  return group_update_impl(g, false, pose, extra, n_p, HostScan{ scan_lik_xyz, n_s, scan_beam_xyz, scan_beam_origin, n_b, origins, n_o },
                           UpdateOutputs{ weight_inout, out_lik, out_match_ratio, out_beam, entropy, match_ratio_min, match_ratio_max,
                                          restored });
}
