// api_particle_bins.inl — included inside the extern "C" block of mcl3dl_hip.hip: the occupied-bin statistic of a particle set
// (particle_bins.h: the definitions; particle_bins_kernels.h: the device pipeline). NOT the reference's behaviour:
// the node shrinks its particles by a fixed factor per scan (src/mcl_3dl.cpp:875-885) and publishes one mean; this is what a
// caller needs to size the set by the posterior (KLD-sampling, Fox 2003) and to read the hypotheses themselves.
namespace
{
// what one run of the pipeline brings home
struct ParticleBinsHome
{
  size_t occupied = 0, occupied_alive = 0, nonfinite = 0, top_n = 0;
  int32_t bin4[4 * PB_MAX_TOP_K] = {};
  double mass[PB_MAX_TOP_K] = {};
  uint32_t count[PB_MAX_TOP_K] = {}, leader[PB_MAX_TOP_K] = {};
};

// the caller's arrays, any of them null
struct ParticleBinsOut
{
  size_t *occupied, *occupied_alive, *nonfinite;
  int32_t* top_bin4;
  double* top_mass;
  uint32_t *top_count, *top_leader;
  size_t* top_n;
  void take(const ParticleBinsHome& h) const
  {
    if (occupied)
      *occupied = h.occupied;
    if (occupied_alive)
      *occupied_alive = h.occupied_alive;
    if (nonfinite)
      *nonfinite = h.nonfinite;
    if (top_n)
      *top_n = h.top_n;
    for (size_t k = 0; k < h.top_n; ++k)
    {
      if (top_bin4)
        memcpy(top_bin4 + 4 * k, h.bin4 + 4 * k, sizeof(int32_t) * 4);
      if (top_mass)
        top_mass[k] = h.mass[k];
      if (top_count)
        top_count[k] = h.count[k];
      if (top_leader)
        top_leader[k] = h.leader[k];
    }
  }
};

// null: the arguments a context and a group check alike are fine; else what is wrong with them
const char* particle_bins_bad_args(const float* bin_xyz, int yaw_bins, int top_k)
{
  if (!bin_xyz || !(bin_xyz[0] > 0.f && bin_xyz[1] > 0.f && bin_xyz[2] > 0.f) || std::isinf(bin_xyz[0]) || std::isinf(bin_xyz[1]) ||
      std::isinf(bin_xyz[2]))
    return "particle_bins: bin_xyz must hold three finite edges > 0";
  if (!pb_yaw_bins_ok(yaw_bins))
    return "particle_bins: yaw_bins must be 1 or 3 ... 64";
  if (top_k < 0 || top_k > PB_MAX_TOP_K)
    return "particle_bins: top_k must be 0 ... 16";
  return nullptr;
}

// the pose grid the finite particles between the corners mm6 span; -3 when its keys do not fit
int particle_bins_grid(mcl3dl_hip_ctx* ctx, const float mm6[6], const float* bin_xyz, int yaw_bins, ParticleBinGrid* grid)
{
  unsigned long long keys = static_cast<unsigned long long>(yaw_bins);
  bool fits = true;
  for (int a = 0; a < 3; ++a)
  {
    grid->inv[a] = 1.0f / bin_xyz[a];
    const float lo = pb_floor_scaled(mm6[a], grid->inv[a]), hi = pb_floor_scaled(mm6[3 + a], grid->inv[a]);
    if (!(std::fabs(lo) < 2147483648.f && std::fabs(hi) < 2147483648.f))
    {
      fits = false;
      break;
    }
    grid->min_b[a] = static_cast<int>(lo);
    const long long div = static_cast<long long>(hi) - static_cast<long long>(lo) + 1;
    if (div < 1 || div > 0x7fffffffLL || keys * static_cast<unsigned long long>(div) > PB_MAX_KEYS)
    {
      fits = false;
      break;
    }
    grid->div[a] = static_cast<uint32_t>(div);
    keys *= static_cast<unsigned long long>(div);
  }
  if (!fits)
    return ctx->fail(-3, "particle_bins: the bins (%g x %g x %g, %d sectors) are too small for the particles' extent "
                         "[%g, %g] x [%g, %g] x [%g, %g]: more than %llu keys",
                     bin_xyz[0], bin_xyz[1], bin_xyz[2], yaw_bins, mm6[0], mm6[3], mm6[1], mm6[4], mm6[2], mm6[5], PB_MAX_KEYS);
  grid->yaw_bins = yaw_bins;
  grid->nonfinite_key = static_cast<uint32_t>(keys);
  return 0;
}

// The pipeline over n rows of `stride` floats (position at 0..2, quaternion xyzw at 3..6) and n weights, all device memory of
// ctx's device. Two synchronisations: the extent (as VoxelGrid's), and the record with the top rows.
int particle_bins_run(mcl3dl_hip_ctx* ctx, const float* d_rows, size_t stride, const float* d_weight, size_t n,
                      const float* bin_xyz, int yaw_bins, int top_k, ParticleBinsHome* home)
{
  *home = ParticleBinsHome();
  HIP_TRY(hipSetDevice(ctx->device));
  const long long nn = static_cast<long long>(n);
  const unsigned nb_mm = minmax_blocks(nn);
  MinMaxOut mm;
  TRY(minmax_out(ctx, nb_mm, &mm));
  hipLaunchKernelGGL(pb_minmax_kernel, dim3(nb_mm), dim3(256), 0, ctx->stream, d_rows, static_cast<long long>(stride), nn, mm);
  HIP_TRY(hipGetLastError());
  float mm6[6];
  unsigned long long n_finite = 0;
  TRY(minmax_to_host(ctx, mm6, &n_finite));
  home->nonfinite = n - static_cast<size_t>(n_finite);
  if (n_finite == 0)
    return 0;
  ParticleBinGrid grid{};
  TRY(particle_bins_grid(ctx, mm6, bin_xyz, yaw_bins, &grid));

  // (key, particle index) -> the stable sort: indices ascend inside a bin, particles without a finite position come last
  TRY(ensure_sort_pairs(ctx, n));
  TRY(ensure(ctx, ctx->pb_table, sizeof(double) * 2 * PB_MAX_YAW_BINS));
  double cs[2 * PB_MAX_YAW_BINS];
  pb_yaw_sector_table(yaw_bins, cs);
  TRY(h2d(ctx, ctx->pb_table.p, cs, sizeof(double) * 2 * static_cast<size_t>(yaw_bins)));
  hipLaunchKernelGGL(pb_key_kernel, dim3(blocks_for(nn)), dim3(256), 0, ctx->stream, d_rows, static_cast<long long>(stride), nn,
                     grid, ctx->pb_table.as<double>(), ctx->cl_key[0].as<uint32_t>(), ctx->cl_val[0].as<uint32_t>());
  HIP_TRY(hipGetLastError());
  TRY(sort_pairs(ctx, nn, bits_for(grid.nonfinite_key)));

  // the segmented reduction over the n_finite sorted pairs in front, then the selection
  const long long nf = static_cast<long long>(n_finite);
  const size_t nb = static_cast<size_t>((nf + PB_BLOCK - 1) / PB_BLOCK);
  TRY(ensure(ctx, ctx->pb_blocks, (sizeof(double) + 4 * sizeof(uint32_t)) * nb));
  TRY(ensure(ctx, ctx->pb_bins, (sizeof(double) + 3 * sizeof(uint32_t)) * static_cast<size_t>(n_finite)));
  TRY(ensure(ctx, ctx->pb_out, sizeof(PbResult) + sizeof(unsigned long long)));
  PbBlockOut part{};
  part.mass = ctx->pb_blocks.as<double>();
  part.wmax = reinterpret_cast<float*>(part.mass + nb);
  part.idx = reinterpret_cast<uint32_t*>(part.wmax + nb);
  part.count = part.idx + nb;
  part.heads = part.count + nb;
  PbBins bins{};
  bins.mass = ctx->pb_bins.as<double>();
  bins.key = reinterpret_cast<uint32_t*>(bins.mass + n_finite);
  bins.count = bins.key + n_finite;
  bins.leader = bins.count + n_finite;
  PbResult* d_result = ctx->pb_out.as<PbResult>();
  bins.n_bins = reinterpret_cast<unsigned long long*>(d_result + 1);
  const uint32_t* key = ctx->cl_key[1].as<uint32_t>();
  const uint32_t* val = ctx->cl_val[1].as<uint32_t>();
  hipLaunchKernelGGL(pb_block_kernel, dim3(static_cast<unsigned>(nb)), dim3(PB_THREADS), 0, ctx->stream, key, val, d_weight, nf, part);
  hipLaunchKernelGGL(pb_bins_kernel, dim3(static_cast<unsigned>(nb)), dim3(PB_THREADS), 0, ctx->stream, key, val, d_weight, nf, part,
                     bins);
  hipLaunchKernelGGL(pb_select_kernel, dim3(1), dim3(PB_SELECT_THREADS), 0, ctx->stream, bins, top_k, d_result);
  HIP_TRY(hipGetLastError());
  PbResult result;
  TRY(d2h(ctx, &result, d_result, sizeof(PbResult)));
  TRY(sync_stream(ctx));
  home->occupied = static_cast<size_t>(result.occupied);
  home->occupied_alive = static_cast<size_t>(result.occupied_alive);
  home->top_n = std::min<size_t>(result.top_n, static_cast<size_t>(top_k));
  for (size_t k = 0; k < home->top_n; ++k)
  {
    pb_key_parts(result.top[k].key, grid, home->bin4 + 4 * k);
    home->mass[k] = result.top[k].mass;
    home->count[k] = result.top[k].count;
    home->leader[k] = result.top[k].leader;
  }
  return 0;
}
}  // namespace

int mcl3dl_hip_yaw_sector_table(int yaw_bins, double* out_cs)
{
  return pb_yaw_sector_table(yaw_bins, out_cs) ? 0 : -3;
}

int mcl3dl_hip_kld_bound(size_t k, double epsilon, double z, size_t* out_n)
{
  return pb_kld_bound(k, epsilon, z, out_n) ? 0 : -3;
}

int mcl3dl_hip_particle_bins_device(mcl3dl_hip_ctx* ctx, const float* d_rows, size_t row_stride, const float* d_weight, size_t n,
                                    const float* bin_xyz, int yaw_bins, int top_k, size_t* out_occupied,
                                    size_t* out_occupied_alive, size_t* out_nonfinite, int32_t* out_top_bin4, double* out_top_mass,
                                    uint32_t* out_top_count, uint32_t* out_top_leader, size_t* out_top_n)
{
  if (!ctx)
    return -1;
  if (!d_rows || !d_weight)
    return ctx->fail(-3, "particle_bins: null rows / weights");
  if (row_stride < 7 || row_stride > 1024)
    return ctx->fail(-3, "particle_bins: row_stride = %zu (7 for pose rows, 13 for state rows)", row_stride);
  if (n == 0 || n > 0x7fffffffu / 16)
    return ctx->fail(-3, "particle_bins: n = %zu is outside [1, %u]", n, 0x7fffffffu / 16);
  if (const char* why = particle_bins_bad_args(bin_xyz, yaw_bins, top_k))
    return ctx->fail(-3, "%s", why);
  ParticleBinsHome home;
  TRY(particle_bins_run(ctx, d_rows, row_stride, d_weight, n, bin_xyz, yaw_bins, top_k, &home));
  ParticleBinsOut{ out_occupied, out_occupied_alive, out_nonfinite, out_top_bin4, out_top_mass, out_top_count, out_top_leader,
                   out_top_n }
      .take(home);
  return 0;
}

// ... over a group's resident particles, leaders as global particle indices. A group of one device that may call its context
// directly reads its shard in place; otherwise states and weights are brought into particle order on every rank the way the
// resampling plan's weights are (group_plan_device), every rank runs the same pipeline, and what comes home must agree.
int mcl3dl_hip_group_particle_bins(mcl3dl_hip_group* g, const float* bin_xyz, int yaw_bins, int top_k, size_t* out_occupied,
                                   size_t* out_occupied_alive, size_t* out_nonfinite, int32_t* out_top_bin4, double* out_top_mass,
                                   uint32_t* out_top_count, uint32_t* out_top_leader, size_t* out_top_n)
{
  if (!g)
    return -1;
  TRY(group_resident(g));
  if (const char* why = particle_bins_bad_args(bin_xyz, yaw_bins, top_k))
    return g->fail(-3, "%s", why);
  const size_t n_p = g->n_resident;
  const int N = g->n();
  const GroupRoute route = g->route();
  if (route == ROUTE_RCCL)
    TRY(group_comms(g));
  TRY(gather_to_host(g, resident_states));
  TRY(gather_to_host(g, resident_weights));
  std::vector<ParticleBinsHome> home(N);
  const auto prepare = [&](const Shard& s) -> int
  {
    mcl3dl_hip_ctx* ctx = s.ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    TRY(rank_holds(ctx, s.n));
    TRY(gather_ahead(g, s, n_p, resident_states(g, ctx)));
    return gather_ahead(g, s, n_p, resident_weights(g, ctx));
  };
  const auto behind = [&](const Shard& s, const VotedRank& voted) -> int
  {
    mcl3dl_hip_ctx* ctx = s.ctx;
    const float *d_states = nullptr, *d_w = nullptr;
    TRY(gather_behind(g, s, voted, n_p, resident_states(g, ctx), &d_states));
    TRY(gather_behind(g, s, voted, n_p, resident_weights(g, ctx), &d_w));
    return particle_bins_run(ctx, d_states, 13, d_w, n_p, bin_xyz, yaw_bins, top_k, &home[s.r]);
  };
  TRY(group_voted_call(VotedCall{ g, "particle_bins", "all-gather of the states and weights" }, n_p, route == ROUTE_RCCL,
                       route != ROUTE_DIRECT, prepare, behind));
  // {occupied, alive, non-finite, top rows, then per row: bin, count, leader, the mass's bits} of every rank
  constexpr size_t WORDS = 4 + 7 * PB_MAX_TOP_K;
  std::vector<uint64_t> got(WORDS * static_cast<size_t>(N), 0);
  for (int r = 0; r < N; ++r)
  {
    uint64_t* w = &got[WORDS * static_cast<size_t>(r)];
    const ParticleBinsHome& h = home[r];
    w[0] = h.occupied;
    w[1] = h.occupied_alive;
    w[2] = h.nonfinite;
    w[3] = h.top_n;
    for (size_t k = 0; k < h.top_n; ++k)
    {
      uint64_t* row = w + 4 + 7 * k;
      for (int a = 0; a < 4; ++a)
        row[a] = static_cast<uint32_t>(h.bin4[4 * k + a]);
      row[4] = h.count[k];
      row[5] = h.leader[k];
      memcpy(&row[6], &h.mass[k], sizeof(double));
    }
  }
  TRY(group_agree(g, "the occupied bins of the resident particles", got.data(), WORDS));
  ParticleBinsOut{ out_occupied, out_occupied_alive, out_nonfinite, out_top_bin4, out_top_mass, out_top_count, out_top_leader,
                   out_top_n }
      .take(home[0]);
  return 0;
}
