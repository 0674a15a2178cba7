// api_group_state.inl — included inside the extern "C" block of mcl3dl_hip.hip: a device group's particles RESIDENT on its
// GPUs between updates, and the steps either side of pf::measure over the shards (SURVEY.md 8f-1, 8f-3 for N GPUs behind the
// C ABI — the reference's process is C++ and cannot bind the torch.distributed helpers of mcl_3dl_amd/distributed.py):
//
//   mcl3dl_hip_group_upload_state / _download_state    std::vector<Particle<State6DOF>> <-> shards (include/mcl_3dl/pf.h:457)
//   mcl3dl_hip_group_update_resident                   pf::measure over the resident particles: nothing but the scan goes up
//   mcl3dl_hip_group_expectation / _covariance         pf.h:294-303,361-390 / :304-360: one record per shard, combined on the host
//   mcl3dl_hip_group_resample_begin / _plan / _apply   pf.h:187-225 / 399-436: the float prefix recurrence runs ONCE, in particle
//                                                      order (it is not associative: per-shard prefixes plus offsets would not
//                                                      reproduce the reference's accum_probability_), every rank plans all slots
//                                                      and writes its slice of the new generation from the all-gathered states
//                                                      (RCCL ncclAllGather over xGMI, or through the host with collective = 1)
namespace
{
__global__ void state13_to_pose7_kernel(const float* __restrict__ state13, int n, float* __restrict__ pose7)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
#pragma unroll
  for (int k = 0; k < 7; ++k)
    pose7[7 * static_cast<size_t>(i) + k] = state13[13 * static_cast<size_t>(i) + k];
}

// ctx->pose holds the poses of this rank's n resident states: the launch that wrote the states wrote it too, or rebuild_pose did
void pose_mirror_stamp(mcl3dl_hip_ctx* ctx, size_t n)
{
  ctx->poses_set(n);
  ctx->pose_resident = true;
}

int rebuild_pose(mcl3dl_hip_ctx* ctx, size_t n)
{
  ctx->poses_set(0);
  if (n == 0)
    return 0;
  TRY(ensure(ctx, ctx->pose, sizeof(float) * 7 * n));
  const int ni = static_cast<int>(n);
  hipLaunchKernelGGL(state13_to_pose7_kernel, dim3((ni + 255) / 256), dim3(256), 0, ctx->stream,
                     ctx->gs_state[ctx->gs_cur].as<float>(), ni, ctx->pose.as<float>());
  HIP_TRY(hipGetLastError());
  pose_mirror_stamp(ctx, n);
  return 0;
}

// the resident calls read the poses from ctx->pose: re-derived from the resident states whenever another call (an upload, a
// non-resident update, a moments call with its own states) has written that buffer since
int resident_poses(mcl3dl_hip_ctx* ctx)
{
  if (ctx->gs_n && (!ctx->pose_resident || ctx->n_pose_uploaded != ctx->gs_n))
    return rebuild_pose(ctx, ctx->gs_n);
  return 0;
}

// every one of the rank's n resident particles weighs `value`
int uniform_weights(mcl3dl_hip_ctx* ctx, size_t n, float value)
{
  hipLaunchKernelGGL(fill_kernel, dim3((static_cast<int>(n) + 255) / 256), dim3(256), 0, ctx->stream, ctx->gs_weight.as<float>(),
                     value, static_cast<float*>(nullptr), 0.0f, static_cast<int>(n));
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- a new generation of resident particles is installed in four steps: the group forgets the old one (with it the plan made
// for it and the odometry noise: fresh State6DOFs carry none); every rank does, and makes room; every rank that filled its shard
// marks it; the group takes the new count.
void generation_begin(mcl3dl_hip_group* g)
{
  g->n_resident = 0;
  g->rs_begun = g->rs_planned = false;
  g->noise_on = false;
}

// (room for the LARGEST shard on every rank, an empty one included: the resampling step's all-gathers send that many from each)
int generation_rank_begin(mcl3dl_hip_ctx* ctx, size_t n_p, int world)
{
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->gs_n = 0;
  ctx->gs_cur = 0;
  const size_t cap = shard_capacity(n_p, world);
  TRY(ensure(ctx, ctx->gs_state[0], sizeof(float) * 13 * cap));
  return ensure(ctx, ctx->gs_weight, sizeof(float) * cap);
}

// gs_state[gs_cur] holds the rank's n new states. pose_written: the launch that filled them wrote the pose mirror as well.
int generation_rank_installed(mcl3dl_hip_ctx* ctx, size_t n, bool pose_written)
{
  if (pose_written)
    pose_mirror_stamp(ctx, n);
  else
    TRY(rebuild_pose(ctx, n));
  ctx->gs_n = n;
  return 0;
}

void generation_installed(mcl3dl_hip_group* g, size_t n_p)
{
  g->n_resident = n_p;
  g->n_pose_uploaded = n_p;
}

// what the three gathers of the resampling steps bring into particle order (host_group_gather.h)
ShardedArray resident_states(mcl3dl_hip_group* g, mcl3dl_hip_ctx* ctx)
{
  return { 13, &ctx->gs_state[ctx->gs_cur], &ctx->gs_pad, &ctx->gs_all, &g->h_state, "shard", "ncclAllGather" };
}

ShardedArray resident_noise(mcl3dl_hip_group* g, mcl3dl_hip_ctx* ctx)
{
  return { 4,       &ctx->gs_noise[ctx->gs_cur],     &ctx->gs_noise_pad, &ctx->gs_noise_all, &g->h_noise,
           "noise", "ncclAllGather (odometry noise)" };
}

ShardedArray resident_weights(mcl3dl_hip_group* g, mcl3dl_hip_ctx* ctx)
{
  return { 1, &ctx->gs_weight, &ctx->rs_d_wpad, &ctx->rs_d_w, &g->h_weight, "weight", "ncclAllGather (weights)" };
}
}  // namespace

int mcl3dl_hip_group_upload_state(mcl3dl_hip_group* g, const float* state13, const float* weight, size_t n_p)
{
  if (!g)
    return -1;
  if (!state13 || n_p == 0 || n_p > 0x7fffffffu / 16)
    return g->fail(-3, "bad state array");
  generation_begin(g);
  TRY(group_run_shards(g, n_p,
                       [&](const Shard& s) -> int
                       {
                         mcl3dl_hip_ctx* ctx = s.ctx;
                         TRY(generation_rank_begin(ctx, n_p, g->n()));
                         if (s.n == 0)
                           return 0;
                         TRY(h2d(ctx, ctx->gs_state[0].p, state13 + 13 * s.lo, sizeof(float) * 13 * s.n));
                         if (weight)
                           TRY(h2d(ctx, ctx->gs_weight.p, weight + s.lo, sizeof(float) * s.n));
                         else
                           TRY(uniform_weights(ctx, s.n, 1.0f / static_cast<float>(n_p)));
                         TRY(generation_rank_installed(ctx, s.n, false));
                         return sync_stream(ctx);
                       }));
  generation_installed(g, n_p);
  return 0;
}

int mcl3dl_hip_group_download_state(mcl3dl_hip_group* g, float* state13, float* weight, size_t n_p)
{
  if (!g)
    return -1;
  if (g->n_resident == 0 || g->n_resident != n_p)
    return g->fail(-5, "%zu particles are resident, %zu asked for", g->n_resident, n_p);
  return group_each_shard(g,
                          [&](mcl3dl_hip_ctx* ctx, int, size_t lo, size_t n) -> int
                          {
                            if (state13)
                              TRY(d2h(ctx, state13 + 13 * lo, ctx->gs_state[ctx->gs_cur].p, sizeof(float) * 13 * n));
                            if (weight)
                              TRY(d2h(ctx, weight + lo, ctx->gs_weight.p, sizeof(float) * n));
                            return sync_stream(ctx);
                          });
}

size_t mcl3dl_hip_group_resident(const mcl3dl_hip_group* g)
{
  return g ? g->n_resident : 0;
}

int mcl3dl_hip_group_update_resident(mcl3dl_hip_group* g, const float* extra, const float* scan_lik_xyz, size_t n_s,
                                     const float* scan_beam_xyz, const uint32_t* scan_beam_origin, size_t n_b,
                                     const float* origins, size_t n_o, float* out_weight, float* out_lik,
                                     float* out_match_ratio, float* out_beam, float* entropy, float* match_ratio_min,
                                     float* match_ratio_max, int* restored)
{
  if (!g)
    return -1;
  return group_update_impl(g, true, nullptr, extra, g->n_resident,
                           HostScan{ scan_lik_xyz, n_s, scan_beam_xyz, scan_beam_origin, n_b, origins, n_o },
                           UpdateOutputs{ out_weight, out_lik, out_match_ratio, out_beam, entropy, match_ratio_min, match_ratio_max,
                                          restored });
}

// ---- scan preparation on a group: every rank prepares its own replica of the cloud (deterministic, no collective, as the
// centroid filter of the global localisation and the count pass of the drawn noise); what comes home must agree ----------------
namespace
{
// f(ctx, rank) on every rank; a group of one device that may call its context directly makes the plain call
int group_scan_each(mcl3dl_hip_group* g, const std::function<int(mcl3dl_hip_ctx*, int)>& f)
{
  return g->route() == ROUTE_DIRECT ? group_forward(g, f) : group_run(g, [&](int r) -> int { return f(g->ctx[r], r); });
}

// f(ctx, the rank's three sizes) on every rank -> the caller's a, b, c, when all ranks agree on `what`
int group_scan_sizes(mcl3dl_hip_group* g, const char* what, const std::function<int(mcl3dl_hip_ctx*, size_t*)>& f, size_t* a,
                     size_t* b, size_t* c)
{
  std::vector<size_t> got(3 * static_cast<size_t>(g->n()), 0);
  TRY(group_scan_each(g, [&](mcl3dl_hip_ctx* ctx, int r) -> int { return f(ctx, &got[3 * r]); }));
  TRY(group_agree(g, what, got.data(), 3));
  size_t* out[3] = { a, b, c };
  for (int k = 0; k < 3; ++k)
    if (out[k])
      *out[k] = got[k];
  return 0;
}

// ... for the samplers that draw: f(ctx, engine state, n_s installed, n_b installed), every rank from the same engine state
int group_scan_drawn(mcl3dl_hip_group* g, uint32_t* engine_state, size_t* out_n_s, size_t* out_n_b,
                     const std::function<int(mcl3dl_hip_ctx*, uint32_t*, size_t*, size_t*)>& f)
{
  if (!engine_state)
    return g->fail(-3, "null engine_state");
  size_t state = 0;
  TRY(group_scan_sizes(
      g, "the drawn scans or the engine state behind them",
      [&](mcl3dl_hip_ctx* ctx, size_t* got) -> int
      {
        uint32_t st = *engine_state;
        TRY(f(ctx, &st, &got[0], &got[1]));
        got[2] = st;
        return 0;
      },
      out_n_s, out_n_b, &state));
  *engine_state = static_cast<uint32_t>(state);
  return 0;
}
}  // namespace

// Replaces: what mcl3dl_hip_scan_begin replaces (src/mcl_3dl.cpp:335-372), for the measurement of a device group
int mcl3dl_hip_group_scan_begin(mcl3dl_hip_group* g, const float* xyz, const uint32_t* label, size_t n, const float* leaf3,
                                const float* clip_lik4, const float* clip_beam4, size_t* n_full, size_t* n_lik_clipped,
                                size_t* n_beam_clipped)
{
  if (!g)
    return -1;
  return group_scan_sizes(
      g, "the sizes of the prepared clouds", [&](mcl3dl_hip_ctx* ctx, size_t* got) -> int
      { return mcl3dl_hip_scan_begin(ctx, xyz, label, n, leaf3, clip_lik4, clip_beam4, &got[0], &got[1], &got[2]); },
      n_full, n_lik_clipped, n_beam_clipped);
}

int mcl3dl_hip_group_scan_begin_pointcloud2(mcl3dl_hip_group* g, const uint8_t* data, size_t n_points, uint32_t point_step,
                                            int off_x, int off_y, int off_z, int off_label, uint32_t label_override,
                                            const float* leaf3, const float* clip_lik4, const float* clip_beam4, size_t* n_full,
                                            size_t* n_lik_clipped, size_t* n_beam_clipped)
{
  if (!g)
    return -1;
  return group_scan_sizes(
      g, "the sizes of the prepared clouds",
      [&](mcl3dl_hip_ctx* ctx, size_t* got) -> int
      {
        return mcl3dl_hip_scan_begin_pointcloud2(ctx, data, n_points, point_step, off_x, off_y, off_z, off_label, label_override,
                                                 leaf3, clip_lik4, clip_beam4, &got[0], &got[1], &got[2]);
      },
      n_full, n_lik_clipped, n_beam_clipped);
}

// ---- the accumulation of clouds on a group: every rank holds its replica (accumClear / accumCloud, src/mcl_3dl.cpp:267-302).
// There is no group download: mcl3dl_hip_scan_accum_download on mcl3dl_hip_group_context(g, r) serves that.
int mcl3dl_hip_group_scan_accum_clear(mcl3dl_hip_group* g)
{
  if (!g)
    return -1;
  return group_scan_each(g, [&](mcl3dl_hip_ctx* ctx, int) -> int { return mcl3dl_hip_scan_accum_clear(ctx); });
}

int mcl3dl_hip_group_scan_accum_push(mcl3dl_hip_group* g, const float* xyz, size_t n, const float* affine12,
                                     size_t* out_cloud_index, size_t* out_total_points)
{
  if (!g)
    return -1;
  return group_scan_sizes(  // {cloud index, total points, -}
      g, "the accumulated clouds", [&](mcl3dl_hip_ctx* ctx, size_t* got) -> int
      { return mcl3dl_hip_scan_accum_push(ctx, xyz, n, affine12, &got[0], &got[1]); }, out_cloud_index, out_total_points, nullptr);
}

int mcl3dl_hip_group_scan_accum_push_pointcloud2(mcl3dl_hip_group* g, const uint8_t* data, size_t n_points, uint32_t point_step,
                                                 int off_x, int off_y, int off_z, const float* affine12, size_t* out_cloud_index,
                                                 size_t* out_total_points)
{
  if (!g)
    return -1;
  return group_scan_sizes(
      g, "the accumulated clouds",
      [&](mcl3dl_hip_ctx* ctx, size_t* got) -> int
      {
        return mcl3dl_hip_scan_accum_push_pointcloud2(ctx, data, n_points, point_step, off_x, off_y, off_z, affine12, &got[0],
                                                      &got[1]);
      },
      out_cloud_index, out_total_points, nullptr);
}

int mcl3dl_hip_group_scan_accum_size(mcl3dl_hip_group* g, size_t* n_clouds, size_t* n_points)
{
  if (!g)
    return -1;
  return group_scan_sizes(
      g, "the accumulated clouds", [&](mcl3dl_hip_ctx* ctx, size_t* got) -> int
      { return mcl3dl_hip_scan_accum_size(ctx, &got[0], &got[1]); }, n_clouds, n_points, nullptr);
}

// Replaces: what mcl3dl_hip_scan_begin_accumulated replaces, for the measurement of a device group
int mcl3dl_hip_group_scan_begin_accumulated(mcl3dl_hip_group* g, const float* affine12, const float* leaf3, const float* clip_lik4,
                                            const float* clip_beam4, size_t* n_full, size_t* n_lik_clipped, size_t* n_beam_clipped)
{
  if (!g)
    return -1;
  return group_scan_sizes(
      g, "the sizes of the prepared clouds", [&](mcl3dl_hip_ctx* ctx, size_t* got) -> int
      { return mcl3dl_hip_scan_begin_accumulated(ctx, affine12, leaf3, clip_lik4, clip_beam4, &got[0], &got[1], &got[2]); },
      n_full, n_lik_clipped, n_beam_clipped);
}

// Replaces: what mcl3dl_hip_scan_finish replaces, on every rank: the sampler's push_back loop (point_cloud_uniform_sampler.h:
// 66-71, or sampler_with_normal's) with caller-drawn indices, and the scans installed where the group's update reads them
int mcl3dl_hip_group_scan_finish(mcl3dl_hip_group* g, const uint32_t* idx_lik, size_t n_s, const uint32_t* idx_beam, size_t n_b,
                                 const float* origins, size_t n_o)
{
  if (!g)
    return -1;
  return group_scan_each(g, [&](mcl3dl_hip_ctx* ctx, int) -> int
                         { return mcl3dl_hip_scan_finish(ctx, idx_lik, n_s, idx_beam, n_b, origins, n_o); });
}

// Replaces: PointCloudUniformSampler::sample for both models (point_cloud_uniform_sampler.h:58-75; beam first,
// src/mcl_3dl.cpp:377-383) on every rank, each from the same engine state
int mcl3dl_hip_group_scan_finish_drawn(mcl3dl_hip_group* g, size_t n_s, size_t n_b, const float* origins, size_t n_o,
                                       uint32_t* engine_state, size_t* out_n_s, size_t* out_n_b)
{
  if (!g)
    return -1;
  return group_scan_drawn(g, engine_state, out_n_s, out_n_b,
                          [&](mcl3dl_hip_ctx* ctx, uint32_t* state, size_t* got_s, size_t* got_b) -> int
                          { return mcl3dl_hip_scan_finish_drawn(ctx, n_s, n_b, origins, n_o, state, got_s, got_b); });
}

// Replaces: PointCloudSamplerWithNormal::sample for both models (point_cloud_sampler_with_normal.h:91-185; beam first) on
// every rank, each from the same engine state. (mcl3dl_hip_scan_finish_drawn_normal is defined in api_sampler.inl.)
int mcl3dl_hip_group_scan_finish_drawn_normal(mcl3dl_hip_group* g, size_t n_s, size_t n_b, const float* origins, size_t n_o,
                                              double normal_search_range, const float* fpc_local3, double max_weight,
                                              uint32_t* engine_state, size_t* out_n_s, size_t* out_n_b)
{
  if (!g)
    return -1;
  return group_scan_drawn(g, engine_state, out_n_s, out_n_b,
                          [&](mcl3dl_hip_ctx* ctx, uint32_t* state, size_t* got_s, size_t* got_b) -> int
                          {
                            return mcl3dl_hip_scan_finish_drawn_normal(ctx, n_s, n_b, origins, n_o, normal_search_range, fpc_local3,
                                                                       max_weight, state, got_s, got_b);
                          });
}

// Replaces: what mcl3dl_hip_group_update_resident replaces (measure(), src/mcl_3dl.cpp:377-470), on the scans the group's
// scan_finish installed: no scan argument, nothing but the optional odometry factors goes up
int mcl3dl_hip_group_update_resident_prepared(mcl3dl_hip_group* g, const float* extra, float* out_weight, float* out_lik,
                                              float* out_match_ratio, float* out_beam, float* entropy, float* match_ratio_min,
                                              float* match_ratio_max, int* restored)
{
  if (!g)
    return -1;
  TRY(group_resident(g));
  for (int r = 0; r < g->n(); ++r)
  {
    const mcl3dl_hip_ctx* c = g->ctx[r];
    if (!c->has_scan)
      return g->fail(-5, "rank %d holds no installed scan (mcl3dl_hip_group_scan_finish first)", r);
    const mcl3dl_hip_ctx* c0 = g->ctx[0];
    if (c->n_s != c0->n_s || c->n_b != c0->n_b || c->n_o != c0->n_o)
      return g->fail(-5, "rank %d holds a scan of %zu + %zu points and %zu origins, rank 0 one of %zu + %zu and %zu", r, c->n_s,
                     c->n_b, c->n_o, c0->n_s, c0->n_b, c0->n_o);
  }
  return group_update_impl(g, true, nullptr, extra, g->n_resident,
                           HostScan{ nullptr, g->ctx[0]->n_s, nullptr, nullptr, g->ctx[0]->n_b, nullptr, g->ctx[0]->n_o },
                           UpdateOutputs{ out_weight, out_lik, out_match_ratio, out_beam, entropy, match_ratio_min, match_ratio_max,
                                          restored },
                           true);
}

namespace
{
// pf::expectationBiased + max + maxBiased over the shards. jump == null: probability_bias_ is the caller's array (or 1);
// else it is formed from each resident pose inside the moments pass, and fetched into out_bias only when asked for.
int group_expectation_impl(mcl3dl_hip_group* g, const float* bias, const JumpBias* jump, float* out_bias, float* out_mean7,
                           float* out_total, int64_t* out_max_index, int64_t* out_max_biased_index)
{
  const size_t n_p = g->n_resident;
  TRY(group_resident(g));
  const int N = g->n();
  g->h_parts.assign(16 * static_cast<size_t>(N), 0.0);
  std::vector<uint64_t> offsets(N, 0);
  TRY(group_run_shards(
      g, n_p,
      [&](const Shard& s) -> int
      {
        mcl3dl_hip_ctx* ctx = s.ctx;
        const int r = s.r;
        const size_t lo = s.lo, n = s.n;
        offsets[r] = lo;
        double* rec = &g->h_parts[16 * static_cast<size_t>(r)];
        if (n == 0)
        {
          rec[10] = -1.0;  // an empty shard never holds the maximum
          rec[12] = -1.0;
          return 0;
        }
        HIP_TRY(hipSetDevice(ctx->device));
        TRY(ensure(ctx, ctx->gs_rec, sizeof(double) * 32));
        const float* d_bias = nullptr;
        if (bias)
        {
          TRY(ensure(ctx, ctx->extra, sizeof(float) * n));
          TRY(h2d(ctx, ctx->extra.p, bias + lo, sizeof(float) * n));
          d_bias = ctx->extra.as<float>();
        }
        JumpBias jb{};
        if (jump)
        {
          TRY(rank_holds(ctx, n));
          jb = *jump;
          if (out_bias)
          {
            TRY(ensure(ctx, ctx->extra, sizeof(float) * n));
            jb.bias_out = ctx->extra.as<float>();
          }
        }
        TRY(resident_poses(ctx));  // (the mirror of the RESIDENT states: re-derived when another call wrote the pose buffer)
        TRY(moments_partial_launch(ctx, ctx->pose.as<float>(), ctx->gs_weight.as<float>(), d_bias, jump ? &jb : nullptr, n,
                                   ctx->gs_rec.as<double>()));
        TRY(d2h(ctx, rec, ctx->gs_rec.p, sizeof(double) * 16));
        if (jump && out_bias)
          TRY(d2h(ctx, out_bias + lo, ctx->extra.p, sizeof(float) * n));
        return sync_stream(ctx);
      }));
  if (mcl3dl_hip_moments_finish(g->h_parts.data(), N, offsets.data(), out_mean7, out_total, out_max_index,
                                out_max_biased_index) != 0)
    return g->fail(-3, "moments_finish rejected the records");
  return 0;
}
}  // namespace

int mcl3dl_hip_group_expectation(mcl3dl_hip_group* g, const float* bias, float* out_mean7, float* out_total,
                                 int64_t* out_max_index, int64_t* out_max_biased_index)
{
  if (!g)
    return -1;
  return group_expectation_impl(g, bias, nullptr, nullptr, out_mean7, out_total, out_max_index, out_max_biased_index);
}

int mcl3dl_hip_group_expectation_jump_bias(mcl3dl_hip_group* g, const float* prev7, float bias_var_dist, float bias_var_ang,
                                           float* out_bias, float* out_mean7, float* out_total, int64_t* out_max_index,
                                           int64_t* out_max_biased_index)
{
  if (!g)
    return -1;
  if (!prev7)
    return g->fail(-3, "null previous pose");
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(prev7[k]))
      return g->fail(-3, "non-finite previous pose");
  if (!(bias_var_dist > 0.f) || !(bias_var_ang > 0.f) || std::isinf(bias_var_dist) || std::isinf(bias_var_ang))
    return g->fail(-3, "bias_var_dist / bias_var_ang must be finite and > 0");
  // NormalLikelihood<float> nl_lin(bias_var_dist_), nl_ang(bias_var_ang_); state_prev_.rot_.inv() (src/mcl_3dl.cpp:438-445)
  JumpBias jb{};
  jb.prev_pos = Vec3f{ prev7[0], prev7[1], prev7[2] };
  jb.prev_rot_inv = qinv(Quat{ prev7[3], prev7[4], prev7[5], prev7[6] });
  normal_likelihood_constants(bias_var_dist, &jb.a_lin, &jb.sq2_lin);
  normal_likelihood_constants(bias_var_ang, &jb.a_ang, &jb.sq2_ang);
  return group_expectation_impl(g, nullptr, &jb, out_bias, out_mean7, out_total, out_max_index, out_max_biased_index);
}

int mcl3dl_hip_group_download_particle(mcl3dl_hip_group* g, int64_t index, float* out_state13, float* out_weight)
{
  if (!g)
    return -1;
  const size_t n_p = g->n_resident;
  TRY(group_resident(g));
  if (index < 0 || static_cast<uint64_t>(index) >= n_p)
    return g->fail(-3, "particle %lld of %zu asked for", static_cast<long long>(index), n_p);
  // the one rank that holds it, 52 + 4 bytes, no collective: on the calling thread
  const ShardSlot at = shard_slot(shard_layout(n_p, g->n()), static_cast<size_t>(index));
  const Shard s = shard_of(g, n_p, static_cast<int>(at.rank));
  mcl3dl_hip_ctx* ctx = s.ctx;
  const int rc = [&]() -> int
  {
    HIP_TRY(hipSetDevice(ctx->device));
    TRY(rank_holds(ctx, s.n));
    if (out_state13)
      TRY(d2h(ctx, out_state13, ctx->gs_state[ctx->gs_cur].as<float>() + 13 * at.offset, sizeof(float) * 13));
    if (out_weight)
      TRY(d2h(ctx, out_weight, ctx->gs_weight.as<float>() + at.offset, sizeof(float)));
    return sync_stream(ctx);
  }();
  return rc ? g->fail_rank(rc, s.r) : 0;
}

namespace
{
// pf::covariance over the shards: `partial` leaves a rank's 22 sums in ctx->gs_rec (the pose mirror is current), the records
// are summed in rank order and finished on the host
int group_covariance_with(mcl3dl_hip_group* g, float* out_cov36,
                          const std::function<int(mcl3dl_hip_ctx*, int, size_t, size_t)>& partial)
{
  g->h_parts.assign(22 * static_cast<size_t>(g->n()), 0.0);
  TRY(group_each_shard(g,
                       [&](mcl3dl_hip_ctx* ctx, int r, size_t lo, size_t n) -> int
                       {
                         TRY(ensure(ctx, ctx->gs_rec, sizeof(double) * 32));
                         TRY(resident_poses(ctx));
                         TRY(partial(ctx, r, lo, n));
                         TRY(d2h(ctx, &g->h_parts[22 * static_cast<size_t>(r)], ctx->gs_rec.p, sizeof(double) * 22));
                         return sync_stream(ctx);
                       }));
  double total[22] = { 0 };
  for (int r = 0; r < g->n(); ++r)  // rank order: deterministic
    for (int k = 0; k < 22; ++k)
      total[k] += g->h_parts[22 * static_cast<size_t>(r) + k];
  return mcl3dl_hip_covariance_finish(total, out_cov36);
}
}  // namespace

int mcl3dl_hip_group_covariance(mcl3dl_hip_group* g, const float* mean7, float* out_cov36)
{
  if (!g)
    return -1;
  TRY(group_resident(g));
  if (!mean7 || !out_cov36)
    return g->fail(-3, "null mean / covariance array");
  return group_covariance_with(g, out_cov36,
                               [&](mcl3dl_hip_ctx* ctx, int, size_t, size_t n) -> int
                               {
                                 return mcl3dl_hip_covariance_partial_device(ctx, ctx->pose.as<float>(),
                                                                             ctx->gs_weight.as<float>(), n, nullptr, 0, mean7,
                                                                             ctx->gs_rec.as<double>());
                               });
}

int mcl3dl_hip_group_resample_begin(mcl3dl_hip_group* g, size_t n_out, float* out_pstep)
{
  if (!g)
    return -1;
  const size_t n_p = g->n_resident;
  TRY(group_resident(g));
  if (n_out == 0)
    n_out = n_p;
  g->rs_begun = g->rs_planned = false;
  // every weight comes to the host once (4 bytes per particle): the prefix recurrence of pf.h:193-197 is sequential
  g->h_weight.resize(n_p);
  TRY(mcl3dl_hip_group_download_state(g, nullptr, g->h_weight.data(), n_p));
  const int N = g->n();
  std::vector<float> pstep(N, 0.f);
  TRY(group_run(g, [&](int r) -> int { return mcl3dl_hip_resample_begin(g->ctx[r], g->h_weight.data(), n_p, n_out, &pstep[r]); }));
  g->rs_n_out = n_out;
  g->rs_begun = true;
  if (out_pstep)
    *out_pstep = pstep[0];
  return 0;
}

int mcl3dl_hip_group_resample_plan(mcl3dl_hip_group* g, int mode, float initial_p, uint32_t* out_source,
                                   uint8_t* out_duplicate, size_t* out_n_duplicates)
{
  if (!g)
    return -1;
  if (!g->rs_begun)
    return g->fail(-5, "group_resample_plan before group_resample_begin");
  std::vector<size_t> n_dup(g->n(), 0);
  TRY(group_run(g,
                [&](int r) -> int
                {
                  return mcl3dl_hip_resample_plan(g->ctx[r], mode, initial_p, r == 0 ? out_source : nullptr,
                                                  r == 0 ? out_duplicate : nullptr, &n_dup[r]);
                }));
  TRY(group_agree(g, "the resampling plan's duplicated particles", n_dup.data(), 1));
  g->rs_n_dup = n_dup[0];
  g->rs_planned = true;
  if (out_n_duplicates)
    *out_n_duplicates = n_dup[0];
  return 0;
}

namespace
{
// fills ctx->rs_d_noise of rank r with the noise rows its output slots [olo, olo + n_new) read (api_rng.inl draws them there)
using ShardNoise = std::function<int(mcl3dl_hip_ctx*, int, size_t, size_t)>;

// drawn == null: the rows are the caller's noise13; else every rank forms its own rows in device memory
int group_resample_apply_impl(mcl3dl_hip_group* g, const float* noise13, size_t n_noise, const ShardNoise* drawn)
{
  const size_t n_p = g->n_resident, n_out = g->rs_n_out;
  const int N = g->n();
  const GroupRoute route = g->route();
  if (route == ROUTE_RCCL)
    TRY(group_comms(g));
  // the odometry noise travels with the states once it has been installed (api_group_motion.inl); without it this call issues
  // the same collectives and launches as it always did
  const bool with_noise = g->noise_on;
  TRY(gather_to_host(g, resident_states));
  if (with_noise)
    TRY(gather_to_host(g, resident_noise));
  // everything ahead of the collective; the all-gather is entered by all ranks or by none (group_voted_call)
  const auto prepare = [&](const Shard& s) -> int
  {
    mcl3dl_hip_ctx* ctx = s.ctx;
    const int other = ctx->gs_cur ^ 1;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t cap_new = shard_capacity(n_out, N);
    TRY(ensure(ctx, ctx->gs_state[other], sizeof(float) * 13 * cap_new));
    TRY(ensure(ctx, ctx->gs_weight, sizeof(float) * cap_new));
    if (with_noise)
    {
      TRY(ensure(ctx, ctx->gs_noise[other], sizeof(float) * 4 * cap_new));
      TRY(gather_ahead(g, s, n_p, resident_noise(g, ctx)));
    }
    return gather_ahead(g, s, n_p, resident_states(g, ctx));
  };
  // the all-gather(s), then the rank's slice of the new generation
  const auto apply = [&](const Shard& s, const VotedRank& voted) -> int
  {
    mcl3dl_hip_ctx* ctx = s.ctx;
    const int r = s.r, other = ctx->gs_cur ^ 1;
    size_t olo, ohi;
    shard_bounds(n_out, N, r, &olo, &ohi);
    const size_t n_new = ohi - olo;
    const float *d_all = nullptr, *d_noise_all = nullptr;
    TRY(gather_behind(g, s, voted, n_p, resident_states(g, ctx), &d_all));
    if (with_noise)  // the four noise floats of every particle the same way: a second all-gather, only while noise is installed
      TRY(gather_behind(g, s, voted, n_p, resident_noise(g, ctx), &d_noise_all));
    if (n_new)
    {
      if (drawn)
      {
        TRY(resample_slice_check(ctx, d_all, olo, n_new, ctx->gs_state[other].as<float>()));
        TRY((*drawn)(ctx, r, olo, n_new));
        TRY(resample_slice_launch(ctx, d_all, olo, n_new, ctx->gs_state[other].as<float>()));
      }
      else
        TRY(mcl3dl_hip_resample_apply_slice_device(ctx, d_all, noise13, n_noise, olo, n_new, ctx->gs_state[other].as<float>()));
      if (with_noise)
      {
        hipLaunchKernelGGL(resample_noise_kernel, dim3((static_cast<int>(n_new) + 255) / 256), dim3(256), 0, ctx->stream,
                           d_noise_all, ctx->rs_d_source.as<uint32_t>() + olo, ctx->rs_d_slot.as<uint32_t>() + olo,
                           static_cast<int>(n_new), ctx->gs_noise[other].as<float>());
        HIP_TRY(hipGetLastError());
      }
      // pf.h:207 / 417: every particle of the new generation weighs 1 / n
      TRY(uniform_weights(ctx, n_new, 1.0f / static_cast<float>(n_out)));
    }
    ctx->gs_cur = other;
    TRY(generation_rank_installed(ctx, n_new, false));
    return sync_stream(ctx);
  };
  const int rc = group_voted_call(VotedCall{ g, "resampling", "all-gather" }, n_p, route == ROUTE_RCCL, route != ROUTE_DIRECT,
                                  prepare, apply);
  g->rs_begun = g->rs_planned = false;
  if (rc)
  {
    generation_begin(g);  // the shards may be half way into the new generation
    return rc;
  }
  generation_installed(g, n_out);
  return 0;
}
}  // namespace

int mcl3dl_hip_group_resample_apply(mcl3dl_hip_group* g, const float* noise13, size_t n_noise)
{
  if (!g)
    return -1;
  if (!g->rs_planned)
    return g->fail(-5, "group_resample_apply before group_resample_plan");
  if (n_noise < g->rs_n_dup || (g->rs_n_dup && !noise13))
    return g->fail(-3, "group_resample_apply: %zu duplicated particles need noise, %zu given", g->rs_n_dup, n_noise);
  return group_resample_apply_impl(g, noise13, n_noise, nullptr);
}

namespace
{
// what every rank's resample_plan_device handed back, and whether the ranks agree
struct GroupPlan
{
  float pstep = 0.f, initial_p = 0.f;
  uint32_t state = 0u;
  size_t n_dup = 0;
  int route = 0;
};

// begin + [uniform draw] + plan over the resident particles in one pass over the ranks: every rank needs ALL weights in
// particle order (the prefix recurrence is not associative) — its own buffer on a group of one, else gathered through the host
// ("collective" 1) or by one ncclAllGather of the padded weight shards, the way the states are (host_group_gather.h) — and runs
// mcl3dl_hip_resample_plan_device over them. Leaves the group where group_resample_plan does.
int group_plan_device(mcl3dl_hip_group* g, size_t n_out, int mode, uint32_t state_in, GroupPlan* out)
{
  const size_t n_p = g->n_resident;
  const int N = g->n();
  const GroupRoute route = g->route();
  g->rs_begun = g->rs_planned = false;
  if (route == ROUTE_RCCL)
    TRY(group_comms(g));
  TRY(gather_to_host(g, resident_weights));
  std::vector<GroupPlan> plan(N);
  const auto prepare = [&](const Shard& s) -> int
  {
    mcl3dl_hip_ctx* ctx = s.ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    TRY(rank_holds(ctx, s.n));
    return gather_ahead(g, s, n_p, resident_weights(g, ctx));
  };
  const auto behind = [&](const Shard& s, const VotedRank& voted) -> int
  {
    mcl3dl_hip_ctx* ctx = s.ctx;
    const float* d_w = nullptr;
    TRY(gather_behind(g, s, voted, n_p, resident_weights(g, ctx), &d_w));
    GroupPlan& p = plan[s.r];
    p.state = state_in;
    return mcl3dl_hip_resample_plan_device(ctx, d_w, n_p, n_out, mode, mode == 0 ? &p.state : nullptr, &p.pstep, &p.initial_p,
                                           &p.n_dup, &p.route);
  };
  TRY(group_voted_call(VotedCall{ g, "resampling", "all-gather of the weights" }, n_p, route == ROUTE_RCCL, route != ROUTE_DIRECT,
                       prepare, behind));
  std::vector<size_t> got;  // {duplicated particles, engine state, route} of every rank
  for (const GroupPlan& p : plan)
    got.insert(got.end(), { p.n_dup, static_cast<size_t>(p.state), static_cast<size_t>(p.route) });
  TRY(group_agree(g, "the resampling plan (duplicated particles, engine state, route)", got.data(), 3));
  g->rs_n_out = n_out;
  g->rs_n_dup = plan[0].n_dup;
  g->rs_begun = g->rs_planned = true;
  *out = plan[0];
  return 0;
}
}  // namespace

// Replaces: pf::resizeParticle(n_out) (pf.h:399-436) on the resident particles, in one call — group_resample_begin(n_out),
// _plan(1, ·), _apply without noise, with the prefixes and `pscan += pstep` formed on the devices.
int mcl3dl_hip_group_resize_resident(mcl3dl_hip_group* g, size_t n_out, int* out_route)
{
  if (!g)
    return -1;
  TRY(group_resident(g));
  if (n_out == 0 || n_out > 0x7fffffffu / 16)
    return g->fail(-3, "group_resize_resident: n_out = %zu is outside [1, %u]", n_out, 0x7fffffffu / 16);
  GroupPlan plan;
  TRY(group_plan_device(g, n_out, 1, 0u, &plan));
  TRY(group_resample_apply_impl(g, nullptr, 0, nullptr));
  if (out_route)
    *out_route = plan.route;
  return 0;
}
