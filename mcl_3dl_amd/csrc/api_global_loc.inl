// api_global_loc.inl — included inside the extern "C" block of mcl3dl_hip.hip: global localisation, the reference's
// `global_localization` service (cbGlobalLocalization, src/mcl_3dl.cpp:1039-1099). Device code: global_loc_kernels.h.
//
//   mcl3dl_hip_global_localization_rotations      the div_yaw rotations, formed on the host like the reference forms them
//   mcl3dl_hip_global_localization_points         VoxelGrid of the base map -> "nothing right above" filter -> compaction
//   mcl3dl_hip_global_localization_seed_device    points x div_yaw particles into caller-owned device arrays
//   mcl3dl_hip_group_global_localization          the service on a device group: the seeded particles are resident afterwards
//
// The centroid search does not go through the context's map index (that one covers the map, not the centroid cloud, and
// must come out of this untouched): the centroids get a cell grid of their own, cell edge 1.01 x radius in the dist_weight
// metric, built by host_grid_builders.h:build_transient_cell_grid (the kernels that build the map's cell grid, grid_kernels.h) into
// buffers of this file's own.
namespace
{
// Quat(Vec3(0, 0, yaw)) — setRPY, include/mcl_3dl/quat.h:202-215, every product kept (they decide the signs of the zeros)
Quat gl_quat_from_yaw(float yaw)
{
  const float zero = 0.0f;
  const float t2 = std::cos(zero / 2), t3 = std::sin(zero / 2);
  const float t4 = std::cos(zero / 2), t5 = std::sin(zero / 2);
  const float t0 = std::cos(yaw / 2), t1 = std::sin(yaw / 2);
  Quat q;
  q.x = t0 * t3 * t4 - t1 * t2 * t5;
  q.y = t0 * t2 * t5 + t1 * t3 * t4;
  q.z = t1 * t2 * t4 - t0 * t3 * t5;
  q.w = t0 * t2 * t4 + t1 * t3 * t5;
  return q;
}

bool gl_quat_ok(const float* q4)
{
  return !q4 || (std::isfinite(q4[0]) && std::isfinite(q4[1]) && std::isfinite(q4[2]) && std::isfinite(q4[3]));
}

bool gl_points_current(const mcl3dl_hip_ctx* ctx)
{
  return ctx->gl_valid && ctx->has_map && ctx->gl_stamp == ctx->stamp && ctx->gl_n_base == ctx->n_base &&
         ctx->gl_n_map == ctx->map_xyz.size() / 3;
}

// cell grid over the n_c centroids in ctx->gl_centroids, rescaled by the dist_weight: ctx->gl_sorted / ctx->gl_cells
int gl_build_centroid_grid(mcl3dl_hip_ctx* ctx, size_t n_c, float radius, LikGrid* out, int* reach)
{
  return build_transient_cell_grid(ctx, ctx->gl_centroids.as<float4>(), n_c, ctx->has_weight ? ctx->weight : nullptr, radius, true,
                                   "centroid", ctx->gl_sorted, ctx->gl_cells, out, reach, nullptr);
}
}  // namespace

int mcl3dl_hip_global_localization_rotations(int div_yaw, const float* imu_quat4, float* out_quat4)
{
  if (div_yaw < 1 || !out_quat4 || !gl_quat_ok(imu_quat4))
    return -3;
  const Quat imu = imu_quat4 ? Quat{ imu_quat4[0], imu_quat4[1], imu_quat4[2], imu_quat4[3] } : Quat{ 0.f, 0.f, 0.f, 1.f };
  for (int cnt = 0; cnt < div_yaw; ++cnt)
  {
    // Vec3(0.0, 0.0, 2.0 * M_PI * cnt / dir): a double expression narrowed to Vec3's float
    const float yaw = static_cast<float>(2.0 * M_PI * cnt / div_yaw);
    const Quat q = qnormalized(qmul(gl_quat_from_yaw(yaw), imu));
    out_quat4[4 * cnt + 0] = q.x;
    out_quat4[4 * cnt + 1] = q.y;
    out_quat4[4 * cnt + 2] = q.z;
    out_quat4[4 * cnt + 3] = q.w;
  }
  return 0;
}

int mcl3dl_hip_global_localization_points(mcl3dl_hip_ctx* ctx, double grid, float* out_xyz, size_t capacity, size_t* n_points,
                                          size_t* n_centroids)
{
  if (!ctx)
    return -1;
  if (n_points)
    *n_points = 0;
  if (n_centroids)
    *n_centroids = 0;
  if (!ctx->has_map)
    return ctx->fail(-5, "no map: call mcl3dl_hip_set_map first");
  const float leaf1 = static_cast<float>(grid);  // setLeafSize takes floats
  if (!(grid > 0.0) || !std::isfinite(grid) || !(leaf1 > 0.f) || !std::isfinite(leaf1))
    return ctx->fail(-3, "global localisation grid must be positive and finite (got %g)", grid);
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->gl_valid = false;
  // ---- 1. VoxelGrid over pc_map_: the base map, without the current map update
  TRY(ensure_map_dev(ctx));
  const size_t n_map = ctx->map_xyz.size() / 3;
  const size_t n_base = (ctx->n_base && ctx->n_base <= n_map) ? ctx->n_base : n_map;
  const float leaf[3] = { leaf1, leaf1, leaf1 };
  size_t n_c = 0;
  TRY(voxel_grid_now(ctx, ctx->map_dev.as<float4>(), n_base, leaf, ctx->gl_centroids, &n_c));
  if (n_centroids)
    *n_centroids = n_c;
  if (n_c == 0)
    return ctx->fail(-5, "no standable point: the base map has no finite point");
  if (n_c > 0x7ffffff0u)
    return ctx->fail(-3, "too many centroids (%zu)", n_c);
  // ---- 2. KdTreeFLANN over the centroids, radiusSearch(p2, grid) for every centroid
  LikGrid cg{};
  int reach = 1;
  TRY(gl_build_centroid_grid(ctx, n_c, leaf1, &cg, &reach));
  const long long nc = static_cast<long long>(n_c);
  TRY(ensure(ctx, ctx->gl_flag, sizeof(uint32_t) * (n_c + 2)));
  TRY(ensure(ctx, ctx->gl_pts, sizeof(float4) * n_c));
  const double shift = 0.01 + grid;                       // p2.z += 0.01 + params_.global_localization_grid_
  const float r2 = static_cast<float>(grid * grid);       // pcl::KdTreeFLANN::radiusSearch(p, double radius, ...)
  hipLaunchKernelGGL(gl_blocked_flag_kernel, dim3(blocks_for(nc + 1)), dim3(256), 0, ctx->stream, ctx->gl_centroids.as<float4>(),
                     nc, shift, cg, lik_params(ctx), r2, reach, ctx->gl_flag.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  // ---- 3. remove_if / erase: the survivors in VoxelGrid order
  TRY(device_exclusive_scan(ctx, ctx->gl_flag.as<uint32_t>(), nc + 1));
  uint32_t kept = 0;
  TRY(d2h(ctx, &kept, ctx->gl_flag.as<uint32_t>() + n_c, sizeof(uint32_t)));
  hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(nc)), dim3(256), 0, ctx->stream, ctx->gl_centroids.as<float4>(),
                     ctx->gl_flag.as<uint32_t>(), nc, ctx->gl_pts.as<float4>());
  HIP_TRY(hipGetLastError());
  TRY(sync_stream(ctx));
  if (n_points)
    *n_points = kept;
  if (kept == 0)
    return ctx->fail(-5, "no standable point: all %zu centroids of the %g grid find a centroid within %g of the point %g above "
                         "them (dist_weight %g %g %g)", n_c, grid, grid, shift, ctx->weight[0], ctx->weight[1], ctx->weight[2]);
  ctx->gl_n_points = kept;
  ctx->gl_n_centroids = n_c;
  ctx->gl_stamp = ctx->stamp;
  ctx->gl_n_base = ctx->n_base;
  ctx->gl_n_map = n_map;
  ctx->gl_valid = true;
  if (out_xyz)
  {
    if (capacity < kept)
      return ctx->fail(-3, "capacity %zu < %u points", capacity, kept);
    TRY(download_cloud(ctx, ctx->gl_pts.as<float4>(), kept, out_xyz, nullptr));
  }
  return 0;
}

int mcl3dl_hip_global_localization_seed_device(mcl3dl_hip_ctx* ctx, int div_yaw, const float* imu_quat4, size_t first,
                                               size_t count, float* d_state13, float* d_pose7, float* d_weight)
{
  if (!ctx)
    return -1;
  if (div_yaw < 1)
    return ctx->fail(-3, "div_yaw must be at least 1 (got %d)", div_yaw);
  if (!gl_quat_ok(imu_quat4))
    return ctx->fail(-3, "imu_quat is not finite");
  if (!gl_points_current(ctx))
    return ctx->fail(-5, "no points of the current map: call mcl3dl_hip_global_localization_points first");
  const size_t total = ctx->gl_n_points * static_cast<size_t>(div_yaw);
  if (first > total || count > total - first)
    return ctx->fail(-3, "particles [%zu, %zu + %zu) asked for, %zu points x %d = %zu exist", first, first, count,
                     ctx->gl_n_points, div_yaw, total);
  if (count > 0x7fffffffu / 16)
    return ctx->fail(-3, "too many particles in one call (%zu)", count);
  if (count == 0)
    return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  std::vector<float> rot(4 * static_cast<size_t>(div_yaw));
  if (mcl3dl_hip_global_localization_rotations(div_yaw, imu_quat4, rot.data()) != 0)
    return ctx->fail(-3, "bad rotation arguments");
  TRY(ensure(ctx, ctx->gl_rot, sizeof(float) * rot.size()));
  TRY(h2d(ctx, ctx->gl_rot.p, rot.data(), sizeof(float) * rot.size()));
  // const float prob = 1.0 / static_cast<float>(points->size());
  const float prob = static_cast<float>(1.0 / static_cast<float>(ctx->gl_n_points));
  const unsigned long long dwords = 13ull * count;
  hipLaunchKernelGGL(gl_seed_kernel, dim3(static_cast<unsigned>((dwords + 255) / 256)), dim3(256), 0, ctx->stream,
                     ctx->gl_pts.as<float4>(), ctx->gl_rot.as<float>(), static_cast<unsigned>(div_yaw),
                     static_cast<unsigned long long>(first), static_cast<unsigned long long>(count), prob, d_state13, d_pose7,
                     d_weight);
  HIP_TRY(hipGetLastError());
  return sync_stream(ctx);  // (the rotation table went up from a host vector of this call)
}

int mcl3dl_hip_group_global_localization(mcl3dl_hip_group* g, double grid, int div_yaw, const float* imu_quat4,
                                         size_t max_particles, size_t* n_points, size_t* n_particles)
{
  if (!g)
    return -1;
  if (n_points)
    *n_points = 0;
  if (n_particles)
    *n_particles = 0;
  if (!(grid > 0.0) || !std::isfinite(grid))
    return g->fail(-3, "global localisation grid must be positive and finite (got %g)", grid);
  if (div_yaw < 1)
    return g->fail(-3, "div_yaw must be at least 1 (got %d)", div_yaw);
  if (!gl_quat_ok(imu_quat4))
    return g->fail(-3, "imu_quat is not finite");
  const int N = g->n();
  // ---- steps 1-3 on every rank (the map is replicated; deterministic, so no collective): nothing resident is touched yet
  std::vector<size_t> pts(N, 0);
  TRY(group_run(g, [&](int r) -> int { return mcl3dl_hip_global_localization_points(g->ctx[r], grid, nullptr, 0, &pts[r], nullptr); }));
  TRY(group_agree(g, "the standable points: are their maps the same?", pts.data(), 1));
  if (n_points)
    *n_points = pts[0];
  const size_t n_p = pts[0] * static_cast<size_t>(div_yaw);
  if (n_particles)
    *n_particles = n_p;
  if (max_particles && n_p > max_particles)
    return g->fail(-3, "%zu points x %d = %zu particles needed, max_particles is %zu", pts[0], div_yaw, n_p, max_particles);
  if (n_p > 0x7fffffffu / 16)
    return g->fail(-3, "%zu points x %d = %zu particles needed, more than resident particles can be (%u)", pts[0], div_yaw, n_p,
                   0x7fffffffu / 16);
  // ---- step 4: every rank seeds its own shard; the group is left as mcl3dl_hip_group_upload_state leaves it
  generation_begin(g);
  TRY(group_run_shards(g, n_p,
                       [&](const Shard& s) -> int
                       {
                         mcl3dl_hip_ctx* ctx = s.ctx;
                         TRY(generation_rank_begin(ctx, n_p, N));
                         if (s.n == 0)
                           return 0;
                         ctx->poses_set(0);
                         TRY(ensure(ctx, ctx->pose, sizeof(float) * 7 * s.n));
                         TRY(mcl3dl_hip_global_localization_seed_device(ctx, div_yaw, imu_quat4, s.lo, s.n,
                                                                        ctx->gs_state[0].as<float>(), ctx->pose.as<float>(),
                                                                        ctx->gs_weight.as<float>()));
                         return generation_rank_installed(ctx, s.n, true);  // (the seeding launch wrote the poses)
                       }));
  generation_installed(g, n_p);
  return 0;
}
