// host_grid_builders.h — part of the single translation unit mcl3dl_hip.hip: host drivers of the two linear-time map
// structures, the cell-sorted exact-NN grid (LikGrid) and the DDA occupancy / voxel index (DdaGrid), and of the cell grid over
// a transient cloud. Each structure has a device form (grid_kernels.h: the map goes up once as float4 {x, y, z, label} and
// everything else happens in HBM — a 10 M-point map used to cost seconds of host time and 1.1 GB of run delimiters over PCIe
// at every map stamp and every map update) and a sequential host form (option grid_build_host = 1) that it is checked
// against. The two come out bit-identical because they share their statements: keys and geometry are the functions of
// index_geometry.h, the host forms' sort is its counting_sort, the device forms' is cell_grid_sort below, and each structure
// is installed into the context by one function (install_cell_grid, install_dda_grid).
#pragma once

namespace
{
// The two search radii of RaycastUsingKDTree (raycast_using_kdtree.h:83, :94): double expressions narrowed to the float
// parameter of ChunkedKdtree::radiusSearch.
void kd_ray_radii(const mcl3dl_hip_ctx* ctx, float* grid_min, float* r1, float* r2)
{
  const float mn = std::min({ ctx->map_grid[0], ctx->map_grid[1], ctx->map_grid[2] });
  const float mx = std::max({ ctx->map_grid[0], ctx->map_grid[1], ctx->map_grid[2] });
  *grid_min = mn;
  *r1 = static_cast<float>(std::sqrt(2.0) * mx / 2.0);
  *r2 = static_cast<float>(mn * 2 + std::sqrt(2.0) * mx / 2.0);
}

// Edge of the cell grid's cubes. A context whose likelihood parameters were never set and that casts with the kd-tree caster
// lays the grid out for that caster's first radius (one cell each way per step of a ray); everybody else for match_dist_min.
bool lik_cell_is_beams(const mcl3dl_hip_ctx* ctx)
{
  return !ctx->lik_params_set && ctx->beam_raycast == 1;
}

float lik_cell_edge(const mcl3dl_hip_ctx* ctx)
{
  if (lik_cell_is_beams(ctx))
  {
    float mn, r1, r2;
    kd_ray_radii(ctx, &mn, &r1, &r2);
    return r1 * 1.01f;
  }
  return ctx->match_dist_min * 1.01f;
}

// ---- exact-NN grid ------------------------------------------------------------------------------------------------------
// Replaces ChunkedKdtree::setInputCloud + pcl::KdTreeFLANN::setInputCloud.  The reference's chunking is a memory
// device (20 m chunks with duplicated margins, chunked_kdtree.h:124-216) whose query result equals the global
// nearest neighbour within the radius whenever radius <= max_search_radius; the grid gives that result directly.
void install_cell_grid(LikGrid* lg, const CellGridGeometry& g, const uint32_t* cell_start, const float4* pts)
{
  *lg = LikGrid{ cell_start, pts, g.o[0], g.o[1], g.o[2], g.inv, g.dim[0], g.dim[1], g.dim[2] };
}

// what every build of the map's cell grid leaves in the context besides ctx->lg
void lik_grid_installed(mcl3dl_hip_ctx* ctx, size_t n)
{
  ctx->footprint[0] = sizeof(float4) * n;
  ctx->footprint[1] = sizeof(uint32_t) * (static_cast<size_t>(ctx->lg.nx) * ctx->lg.ny * ctx->lg.nz + 1);
  ctx->lik_dirty = false;
  ctx->lik_cell_from_beam = lik_cell_is_beams(ctx);
  ctx->kd_occ_reach = 0;  // (the kd-tree caster's bitmap is of the previous grid)
}

// Host form: the sequential counting sort the device form is checked against.
int build_lik_grid_host(mcl3dl_hip_ctx* ctx)
{
  const size_t n = ctx->map_xyz.size() / 3;
  const float cell = lik_cell_edge(ctx);
  if (!(cell > 0.f) || !std::isfinite(cell))
    return ctx->fail(-3, "match_dist_min must be positive and finite");
  std::vector<float4> s;
  float mn[3] = { 0, 0, 0 }, mx[3] = { 0, 0, 0 };
  TRY(rescaled_points(ctx, 0, n, s, mn, mx));
  const CellGridGeometry geom = cell_grid_geometry(mn, mx, cell);
  const double total = static_cast<double>(geom.dim[0]) * geom.dim[1] * geom.dim[2];
  if (total > 3.0e9)
    return ctx->fail(-4, "likelihood grid would need %.3g cells (map extent too large for the dense index)", total);
  const size_t ncell = static_cast<size_t>(geom.dim[0]) * geom.dim[1] * geom.dim[2];
  std::vector<uint32_t> key(n), start, order;
  for (size_t i = 0; i < n; ++i)
    key[i] = cell_index(geom, s[i].x, s[i].y, s[i].z);
  counting_sort(key, ncell, start, order);
  std::vector<float4> pts(n);
  for (size_t k = 0; k < n; ++k)
    pts[k] = s[order[k]];
  TRY(ensure(ctx, ctx->lik_pts, sizeof(float4) * n));
  TRY(ensure(ctx, ctx->lik_cells, sizeof(uint32_t) * (ncell + 1)));
  TRY(h2d(ctx, ctx->lik_pts.p, pts.data(), sizeof(float4) * n));
  TRY(h2d(ctx, ctx->lik_cells.p, start.data(), sizeof(uint32_t) * (ncell + 1)));
  TRY(sync_stream(ctx));
  install_cell_grid(&ctx->lg, geom, ctx->lik_cells.as<uint32_t>(), ctx->lik_pts.as<float4>());
  lik_grid_installed(ctx, n);
  return 0;
}

// The counting sort of a cloud by cell on the device: sp = n rescaled points (w = index in the cloud), g their grid; the
// points land cell by cell in `sorted` (ascending index inside a cell: the sort is stable) and the cells + 1 run delimiters
// in `cells`. any: the cloud may hold non-finite points (cell 0). The caller has sized sorted, cells and the sort's work
// arrays (ensure_sort_pairs). Cell keys + histogram -> stable sort -> gather -> exclusive scan.
int cell_grid_sort(mcl3dl_hip_ctx* ctx, const float4* sp, long long n, const CellGridGeometry& g, bool any, float4* sorted,
                   uint32_t* cells)
{
  const size_t ncell = static_cast<size_t>(g.dim[0]) * g.dim[1] * g.dim[2];
  HIP_TRY(hipMemsetAsync(cells, 0, sizeof(uint32_t) * (ncell + 1), ctx->stream));
  hipLaunchKernelGGL(any ? lik_cell_key_kernel<true> : lik_cell_key_kernel<false>, dim3(blocks_for(n)), dim3(256), 0, ctx->stream,
                     sp, n, g, ctx->cl_key[0].as<uint32_t>(), ctx->cl_val[0].as<uint32_t>(), cells);
  TRY(sort_pairs(ctx, n, bits_for(ncell - 1)));
  hipLaunchKernelGGL(grid_gather_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, sp, ctx->cl_val[1].as<uint32_t>(), n,
                     sorted);
  HIP_TRY(hipGetLastError());
  return device_exclusive_scan(ctx, cells, static_cast<long long>(ncell) + 1);
}

// Device form. The grid in use = the grid of the BASE map (cell_grid_sort: linear, but a sort of the whole map) merged with
// the current map update's points (three small kernels, no sort of the map: grid_kernels.h). The base grid is laid out for
// the bounds of base + update of the moment; a later update that stays inside those bounds only merges (0.36 -> ~0.07 ms at
// 1 M points), one that leaves them rebuilds the base for the new bounds.
int build_lik_grid_device(mcl3dl_hip_ctx* ctx)
{
  const size_t n = ctx->map_xyz.size() / 3;
  const size_t n_base = (ctx->n_base && ctx->n_base <= n) ? ctx->n_base : n;
  const size_t n_upd = n - n_base;
  const long long nn = static_cast<long long>(n);
  const float cell = lik_cell_edge(ctx);
  if (!(cell > 0.f) || !std::isfinite(cell))
    return ctx->fail(-3, "match_dist_min must be positive and finite");
  if (n == 0 || n > 0x7fffffffu)
    return ctx->fail(-3, "bad map size for the likelihood grid");
  BuildTimer tm;
  TRY(tm.start(ctx));
  // can the base grid in place take this update? (same base map, same cell edge, update inside the bounds it was laid out for).
  // The update's points — a few thousand — are rescaled on the host (the same float product the device forms) and go up alone:
  // the whole map is neither uploaded nor touched by a kernel unless the base has to be rebuilt.
  bool keep_base = !ctx->lik_base_dirty && ctx->lik_base_n == n_base && ctx->lik_base_geom.inv == 1.0f / cell && ctx->lik_base_pts.p;
  std::vector<float4>& upd_host = ctx->lik_upd_host;
  TRY(rescaled_points(ctx, n_base, n_upd, upd_host, nullptr, nullptr));
  for (const float4& p : upd_host)
  {
    const float v[3] = { p.x, p.y, p.z };
    for (int a = 0; a < 3; ++a)
      keep_base = keep_base && v[a] >= ctx->lik_base_lo[a] && v[a] <= ctx->lik_base_hi[a];
  }
  TempBuf sp;       // rescaled points of the whole map (only when the base is rebuilt)
  TempBuf sp_u;     // rescaled points of the update
  if (n_upd)
  {
    TRY(scratch_alloc(ctx, sp_u, sizeof(float4) * n_upd));
    TRY(h2d(ctx, sp_u.p, upd_host.data(), sizeof(float4) * n_upd));
  }
  if (!keep_base)
  {
    TRY(ensure_map_dev(ctx));
    TRY(scratch_alloc(ctx, sp, sizeof(float4) * n));
    hipLaunchKernelGGL(grid_rescale_kernel, dim3(blocks_for(nn)), dim3(256), 0, ctx->stream, ctx->map_dev.as<float4>(), nn,
                       ctx->weight[0], ctx->weight[1], ctx->weight[2], ctx->has_weight ? 1 : 0, static_cast<float4*>(sp.p));
    float mm[6];
    unsigned long long n_finite = 0;
    TRY(cloud_minmax(ctx, static_cast<const float4*>(sp.p), nn, mm, &n_finite));
    if (n_finite != n)
      return ctx->fail(-3, "%llu map point(s) are not finite", static_cast<unsigned long long>(n) - n_finite);
    const CellGridGeometry geom = cell_grid_geometry(mm, mm + 3, cell);
    const double total = static_cast<double>(geom.dim[0]) * geom.dim[1] * geom.dim[2];
    if (total > 3.0e9)
      return ctx->fail(-4, "likelihood grid would need %.3g cells (map extent too large for the dense index)", total);
    TRY(ensure(ctx, ctx->lik_base_pts, sizeof(float4) * n_base));
    TRY(ensure(ctx, ctx->lik_base_cells, sizeof(uint32_t) * (static_cast<size_t>(total) + 1)));
    TRY(ensure_sort_pairs(ctx, n));
    TRY(cell_grid_sort(ctx, static_cast<const float4*>(sp.p), static_cast<long long>(n_base), geom, false,
                       ctx->lik_base_pts.as<float4>(), ctx->lik_base_cells.as<uint32_t>()));
    ctx->lik_base_geom = geom;
    for (int a = 0; a < 3; ++a)
    {
      ctx->lik_base_lo[a] = mm[a];
      ctx->lik_base_hi[a] = mm[3 + a];
    }
    ctx->lik_base_n = n_base;
    ctx->lik_base_dirty = false;
    ++ctx->lik_grid_rebuilds;
  }
  const CellGridGeometry& g = ctx->lik_base_geom;  // the merged grid is laid out like the base grid
  const size_t ncell = static_cast<size_t>(g.dim[0]) * g.dim[1] * g.dim[2];
  if (n_upd == 0)
    install_cell_grid(&ctx->lg, g, ctx->lik_base_cells.as<uint32_t>(), ctx->lik_base_pts.as<float4>());
  else
  {
    const int nu = static_cast<int>(n_upd);
    TRY(ensure(ctx, ctx->lik_pts, sizeof(float4) * n));
    TRY(ensure(ctx, ctx->lik_cells, sizeof(uint32_t) * (ncell + 1)));
    TRY(ensure_sort_pairs(ctx, n_upd));
    const float4* sp_upd = static_cast<const float4*>(sp_u.p);
    hipLaunchKernelGGL(lik_update_key_kernel, dim3(blocks_for(nu)), dim3(256), 0, ctx->stream, sp_upd, nu, g,
                       ctx->cl_key[0].as<uint32_t>(), ctx->cl_val[0].as<uint32_t>());
    TRY(sort_pairs(ctx, nu, bits_for(ncell - 1)));
    hipLaunchKernelGGL(lik_merge_cells_kernel, dim3(blocks_for(static_cast<long long>(ncell) + 1)), dim3(256), 0, ctx->stream,
                       ctx->lik_base_cells.as<uint32_t>(), static_cast<long long>(ncell) + 1, ctx->cl_key[1].as<uint32_t>(),
                       static_cast<uint32_t>(n_upd), ctx->lik_cells.as<uint32_t>());
    hipLaunchKernelGGL(lik_merge_points_kernel, dim3(blocks_for(nn)), dim3(256), 0, ctx->stream,
                       ctx->lik_base_pts.as<float4>(), static_cast<long long>(n_base), ctx->lik_base_cells.as<uint32_t>(), g,
                       sp_upd, ctx->cl_key[1].as<uint32_t>(), ctx->cl_val[1].as<uint32_t>(), static_cast<uint32_t>(n_upd),
                       ctx->lik_pts.as<float4>());
    HIP_TRY(hipGetLastError());
    install_cell_grid(&ctx->lg, g, ctx->lik_cells.as<uint32_t>(), ctx->lik_pts.as<float4>());
    if (keep_base)
      ++ctx->lik_grid_merges;
  }
  TRY(tm.stop_ms(ctx, &ctx->grid_build_ms[0]));
  lik_grid_installed(ctx, n);
  return 0;
}

// ---- DDA occupancy + voxel index (RaycastUsingDDA::updatePointCloud / setExists, raycast_using_dda.h:162-190,230-235) ----
// AABB by getMinMax3D; dimensions, voxel of a point and its brick bit: index_geometry.h; per voxel the points stay in
// insertion (map) order.
// the ray-test constants of a DdaGrid
void dda_ray_constants(const mcl3dl_hip_ctx* ctx, DdaGrid& g)
{
  g.grid = static_cast<double>(ctx->dda_grid_size);
  g.ray_angle_half = static_cast<double>(ctx->ray_angle_half);
  // RaycastUsingDDA ctor, raycast_using_dda.h:59: map_grid_size_y appears twice (reference quirk, kept)
  const double gx = ctx->map_grid[0], gy = ctx->map_grid[1];
  g.min_dist_thr_sq = gx * gx + gy * gy + gy * gy;
  g.hit_tolerance_f = static_cast<float>(static_cast<double>(ctx->hit_range));
}

// The grid g over the map's n points (bounds mx; g.mn), its arrays in ctx->dda_bits / dda_start / dda_pts / dda_index,
// without an overlay. ov_base and ctx->dda_overlay_ok are the caller's.
void install_dda_grid(mcl3dl_hip_ctx* ctx, const DdaGeom& g, const float mx[3], size_t n)
{
  DdaGrid& d = ctx->dg;
  d.bricks = ctx->dda_bits.as<unsigned long long>();
  d.bnx = g.bdim[0];
  d.bny = g.bdim[1];
  d.bnz = g.bdim[2];
  d.mul24_ok = (g.bdim[0] < (1 << 24) && static_cast<long long>(g.bdim[1]) * g.bdim[2] < (1ll << 24)) ? 1 : 0;
  d.vox_start = ctx->dda_start.as<uint32_t>();
  d.pts = ctx->dda_pts.as<float4>();
  d.pt_index = ctx->dda_index.as<uint32_t>();
  d.min_x = g.mn[0];
  d.min_y = g.mn[1];
  d.min_z = g.mn[2];
  d.max_x = mx[0];
  d.max_y = mx[1];
  d.max_z = mx[2];
  d.nx = g.dim[0];
  d.ny = g.dim[1];
  d.nz = g.dim[2];
  d.ov_n = 0;
  dda_ray_constants(ctx, d);
  ctx->dda_geom = g;
  ctx->footprint[2] = sizeof(unsigned long long) * g.bdim[0] * g.bdim[1] * g.bdim[2];
  ctx->footprint[3] = sizeof(uint32_t) * (g.total + 1);
  ctx->footprint[4] = sizeof(float4) * n + sizeof(uint32_t) * n;
}

// Host form: every point goes into the one array, so a map update then rebuilds.
int build_dda_grid_host(mcl3dl_hip_ctx* ctx)
{
  const size_t n = ctx->map_xyz.size() / 3;
  const double grid = static_cast<double>(ctx->dda_grid_size);
  if (!(grid > 0))
    return ctx->fail(-3, "dda_grid_size must be positive");
  float mn[3] = { 3.4e38f, 3.4e38f, 3.4e38f }, mx[3] = { -3.4e38f, -3.4e38f, -3.4e38f };
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a)
    {
      const float v = ctx->map_xyz[3 * i + a];
      if (v < mn[a])
        mn[a] = v;
      if (v > mx[a])
        mx[a] = v;
    }
  double total_d;
  const DdaGeom g = dda_grid_geometry(mn, mx, grid, &total_d);
  if (total_d >= 2147483647.0)  // the reference keeps point_total in an int (raycast_using_dda.h:176)
    return ctx->fail(-4, "DDA grid would need %.3g voxels (>= 2^31)", total_d);
  const size_t total = g.total;
  std::vector<uint32_t> vox(n), start, index;
  std::vector<unsigned long long> bits(static_cast<size_t>(g.bdim[0]) * g.bdim[1] * g.bdim[2], 0ull);
  for (size_t i = 0; i < n; ++i)
  {
    int c[3];
    for (int a = 0; a < 3; ++a)
      c[a] = dda_voxel_coord(ctx->map_xyz[3 * i + a], mn[a], grid);
    const size_t v = static_cast<size_t>(dda_voxel_index(g, c[0], c[1], c[2]));
    if (v >= total)
      return ctx->fail(-3, "map point %zu falls outside its own DDA grid", i);
    vox[i] = static_cast<uint32_t>(v);
    size_t brick;
    unsigned long long bit;
    dda_brick_of(g, c[0], c[1], c[2], brick, bit);
    bits[brick] |= bit;
  }
  counting_sort(vox, total, start, index);
  std::vector<float4> pts(n);
  for (size_t k = 0; k < n; ++k)
  {
    const size_t i = index[k];
    pts[k] = make_float4(ctx->map_xyz[3 * i], ctx->map_xyz[3 * i + 1], ctx->map_xyz[3 * i + 2], bits_to_float(ctx->map_label[i]));
  }
  TRY(ensure(ctx, ctx->dda_bits, sizeof(unsigned long long) * bits.size()));
  TRY(ensure(ctx, ctx->dda_start, sizeof(uint32_t) * (total + 1)));
  TRY(ensure(ctx, ctx->dda_pts, sizeof(float4) * n));
  TRY(ensure(ctx, ctx->dda_index, sizeof(uint32_t) * n));
  TRY(h2d(ctx, ctx->dda_bits.p, bits.data(), sizeof(unsigned long long) * bits.size()));
  TRY(h2d(ctx, ctx->dda_start.p, start.data(), sizeof(uint32_t) * (total + 1)));
  TRY(h2d(ctx, ctx->dda_pts.p, pts.data(), sizeof(float4) * n));
  TRY(h2d(ctx, ctx->dda_index.p, index.data(), sizeof(uint32_t) * n));
  TRY(sync_stream(ctx));
  install_dda_grid(ctx, g, mx, n);
  ctx->dda_overlay_ok = false;
  ctx->dda_dirty = false;
  return 0;
}

// The map update as an overlay (DdaGrid::ov_*): the previous overlay's bits are withdrawn (a voxel without base points is
// empty again), the new points are keyed, sorted by voxel (stable: update order inside a voxel) and their bits set. A few
// small launches over the update's points — the base arrays are not touched, nothing is read back. upd = the update's
// points on the device {x, y, z, label bits}, all inside the grid's bounds (the caller checked).
int dda_overlay_apply(mcl3dl_hip_ctx* ctx, const float4* upd, size_t n_upd, size_t n_base)
{
  DdaGrid& d = ctx->dg;
  const DdaGeom g = ctx->dda_geom;
  if (d.ov_n > 0)
    hipLaunchKernelGGL(dda_overlay_clear_kernel, dim3(blocks_for(d.ov_n)), dim3(256), 0, ctx->stream, d.ov_key, d.ov_n, g,
                       d.vox_start, ctx->dda_bits.as<unsigned long long>());
  d.ov_n = 0;
  d.ov_base = static_cast<uint32_t>(n_base);
  if (n_upd == 0)
    return 0;
  if (n_upd > 0x7fffffffu)
    return ctx->fail(-3, "map update too large");
  const int n = static_cast<int>(n_upd);
  TRY(ensure(ctx, ctx->dda_ov_key, sizeof(uint32_t) * n_upd));  // (a reallocation waits for the stream: the clear kernel is through)
  TRY(ensure(ctx, ctx->dda_ov_pts, sizeof(float4) * n_upd));
  TRY(ensure(ctx, ctx->dda_ov_idx, sizeof(uint32_t) * n_upd));
  TRY(ensure_sort_pairs(ctx, n_upd));
  hipLaunchKernelGGL(dda_overlay_key_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, upd, n, g,
                     ctx->cl_key[0].as<uint32_t>(), ctx->cl_val[0].as<uint32_t>());
  TRY(sort_pairs(ctx, n, bits_for(g.total - 1)));
  hipLaunchKernelGGL(dda_overlay_set_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, upd, ctx->cl_key[1].as<uint32_t>(),
                     ctx->cl_val[1].as<uint32_t>(), n, g, ctx->dda_ov_key.as<uint32_t>(), ctx->dda_ov_pts.as<float4>(),
                     ctx->dda_ov_idx.as<uint32_t>(), ctx->dda_bits.as<unsigned long long>());
  HIP_TRY(hipGetLastError());
  d.ov_key = ctx->dda_ov_key.as<uint32_t>();
  d.ov_pts = ctx->dda_ov_pts.as<float4>();
  d.ov_idx = ctx->dda_ov_idx.as<uint32_t>();
  d.ov_n = n;
  return 0;
}

// Device form.
int build_dda_grid_device(mcl3dl_hip_ctx* ctx)
{
  const size_t n = ctx->map_xyz.size() / 3;
  const double grid = static_cast<double>(ctx->dda_grid_size);
  if (!(grid > 0))
    return ctx->fail(-3, "dda_grid_size must be positive");
  if (n == 0 || n > 0x7fffffffu)
    return ctx->fail(-3, "bad map size for the DDA grid");
  TRY(ensure_map_dev(ctx));
  BuildTimer tm;
  TRY(tm.start(ctx));
  float mm[6];
  unsigned long long n_finite = 0;
  TRY(cloud_minmax(ctx, ctx->map_dev.as<float4>(), static_cast<long long>(n), mm, &n_finite));  // pcl::getMinMax3D
  if (n_finite != n)
    return ctx->fail(-3, "%llu map point(s) are not finite", static_cast<unsigned long long>(n) - n_finite);
  // A map update that stays inside the base map's bounds (the usual one: it is what the robot sees) does not change the
  // grid's geometry: the arrays are then built from the base map alone and the update rides on top as an overlay, which the
  // next update replaces without a rebuild.
  const size_t n_base = (ctx->n_base && ctx->n_base <= n) ? ctx->n_base : n;
  const size_t n_upd = n - n_base;
  bool overlay = false;
  if (n_upd > 0 && ctx->opt.dda_overlay)
  {
    float mb[6];
    unsigned long long nf = 0;
    TRY(cloud_minmax(ctx, ctx->map_dev.as<float4>(), static_cast<long long>(n_base), mb, &nf));
    overlay = memcmp(mb, mm, sizeof(mm)) == 0;
  }
  const size_t n_csr = overlay ? n_base : n;
  const long long nn = static_cast<long long>(n_csr);
  double total_d;
  const DdaGeom g = dda_grid_geometry(mm, mm + 3, grid, &total_d);
  if (total_d >= 2147483647.0)  // the reference keeps point_total in an int (raycast_using_dda.h:176)
    return ctx->fail(-4, "DDA grid would need %.3g voxels (>= 2^31)", total_d);
  const size_t total = g.total;
  const size_t n_bricks = static_cast<size_t>(g.bdim[0]) * g.bdim[1] * g.bdim[2];
  TRY(ensure(ctx, ctx->dda_bits, sizeof(unsigned long long) * n_bricks));
  TRY(ensure(ctx, ctx->dda_start, sizeof(uint32_t) * (total + 1)));
  TRY(ensure(ctx, ctx->dda_pts, sizeof(float4) * n_csr));
  TRY(ensure(ctx, ctx->dda_index, sizeof(uint32_t) * n_csr));
  TRY(ensure_sort_pairs(ctx, n));
  TRY(ensure(ctx, ctx->cl_err, sizeof(int)));
  HIP_TRY(hipMemsetAsync(ctx->cl_err.p, 0, sizeof(int), ctx->stream));
  HIP_TRY(hipMemsetAsync(ctx->dda_bits.p, 0, sizeof(unsigned long long) * n_bricks, ctx->stream));
  HIP_TRY(hipMemsetAsync(ctx->dda_start.p, 0, sizeof(uint32_t) * (total + 1), ctx->stream));
  hipLaunchKernelGGL(dda_voxel_key_kernel, dim3(blocks_for(nn)), dim3(256), 0, ctx->stream, ctx->map_dev.as<float4>(), nn, g,
                     ctx->cl_key[0].as<uint32_t>(), ctx->cl_val[0].as<uint32_t>(), ctx->dda_start.as<uint32_t>(),
                     ctx->dda_bits.as<unsigned long long>(), ctx->cl_err.as<int>());
  TRY(sort_pairs(ctx, nn, bits_for(total - 1)));
  hipLaunchKernelGGL(dda_gather_kernel, dim3(blocks_for(nn)), dim3(256), 0, ctx->stream, ctx->map_dev.as<float4>(),
                     ctx->cl_val[1].as<uint32_t>(), nn, ctx->dda_pts.as<float4>(), ctx->dda_index.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  TRY(device_exclusive_scan(ctx, ctx->dda_start.as<uint32_t>(), static_cast<long long>(total) + 1));
  int err = 0;
  TRY(d2h(ctx, &err, ctx->cl_err.p, sizeof(int)));
  install_dda_grid(ctx, g, mm + 3, n);  // (a fresh bit array: nothing of an earlier overlay to withdraw)
  ctx->dg.ov_base = static_cast<uint32_t>(n_base);
  if (overlay)
    TRY(dda_overlay_apply(ctx, ctx->map_dev.as<float4>() + n_base, n_upd, n_base));
  double ms = 0.0;
  TRY(tm.stop_ms(ctx, &ms));
  if (err)  // (dda_dirty stays set: what install_dda_grid wrote is replaced by the next build before anything reads it)
    return ctx->fail(-3, "a map point falls outside its own DDA grid");
  ctx->grid_build_ms[1] = ms;
  ctx->dda_overlay_ok = ctx->opt.dda_overlay && (n_upd == 0 || overlay);
  ctx->dda_dirty = false;
  return 0;
}

int build_lik_grid(mcl3dl_hip_ctx* ctx)
{
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = ctx->opt.grid_build_host ? build_lik_grid_host(ctx) : build_lik_grid_device(ctx);
  ctx->grid_build_wall_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int build_dda_grid(mcl3dl_hip_ctx* ctx)
{
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = ctx->opt.grid_build_host ? build_dda_grid_host(ctx) : build_dda_grid_device(ctx);
  ctx->grid_build_wall_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

// ---- a cell grid over a TRANSIENT cloud (global localisation's centroids, the normal sampler's scan) -----------------------
// Not the context's map index: the sorted points and the run delimiters go into buffers the caller names, the map's grid and
// its dirty flags are not touched. Rescale (w = index in the cloud) -> min / max -> cell_grid_geometry -> cell_grid_sort.
constexpr size_t GL_MAX_CELLS = 1u << 28;  // 1 GiB of run delimiters

// cloud: n points on the device. weight3: the dist_weight the search metric rescales by, nullptr = the plain metric.
// radius: the search radius in that metric; the cell edge is 1.01 x radius. require_finite: a non-finite (rescaled) point is
// an error (-3); otherwise such points are sorted into cell 0 of the grid, where no float distance to them passes a `<`,
// and *n_finite says how many points are finite (0: no grid was built, *out is empty). `what` names the cloud in messages.
int build_transient_cell_grid(mcl3dl_hip_ctx* ctx, const float4* cloud, size_t n, const float* weight3, float radius,
                              bool require_finite, const char* what, DevBuf& sorted, DevBuf& cells, LikGrid* out, int* reach,
                              unsigned long long* n_finite_out)
{
  const long long nc = static_cast<long long>(n);
  const float w3[3] = { weight3 ? weight3[0] : 1.f, weight3 ? weight3[1] : 1.f, weight3 ? weight3[2] : 1.f };
  TempBuf sp;
  TRY(scratch_alloc(ctx, sp, sizeof(float4) * n));
  hipLaunchKernelGGL(grid_rescale_kernel, dim3(blocks_for(nc)), dim3(256), 0, ctx->stream, cloud, nc, w3[0], w3[1], w3[2],
                     weight3 ? 1 : 0, static_cast<float4*>(sp.p));
  float mm[6];
  unsigned long long n_finite = 0;
  TRY(cloud_minmax(ctx, static_cast<const float4*>(sp.p), nc, mm, &n_finite));
  if (n_finite_out)
    *n_finite_out = n_finite;
  if (require_finite && n_finite != n)
    return ctx->fail(-3, "%llu rescaled %s(s) are not finite (dist_weight %g %g %g)", static_cast<unsigned long long>(n) - n_finite,
                     what, w3[0], w3[1], w3[2]);
  *out = LikGrid{};
  *reach = 1;
  if (n_finite == 0)
    return 0;
  const float cell = radius * 1.01f;
  if (!(cell > 0.f) || !std::isfinite(cell) || !std::isfinite(1.0f / cell))
    return ctx->fail(-3, "%s grid: %g cannot be a cell edge", what, radius);
  const CellGridGeometry g = cell_grid_geometry(mm, mm + 3, cell);
  const int* dim = g.dim;
  for (int a = 0; a < 3; ++a)
  {
    const double d = std::floor((static_cast<double>(mm[3 + a]) - g.o[a]) * g.inv) + 3;
    if (!(d < 2.0e9))
      return ctx->fail(-3, "the %s cloud spans %.3g cells of %.3g along axis %d (dist_weight %g %g %g)", what, d, cell, a, w3[0],
                       w3[1], w3[2]);
  }
  const double total = static_cast<double>(dim[0]) * dim[1] * dim[2];
  if (total > static_cast<double>(GL_MAX_CELLS))
    return ctx->fail(-3, "the %s index would need %.3g cells of edge %.3g (%d x %d x %d with dist_weight %g %g %g); "
                         "at most %zu are supported", what, total, cell, dim[0], dim[1], dim[2], w3[0], w3[1], w3[2],
                     GL_MAX_CELLS);
  TRY(ensure(ctx, sorted, sizeof(float4) * n));
  TRY(ensure(ctx, cells, sizeof(uint32_t) * (static_cast<size_t>(total) + 1)));
  TRY(ensure_sort_pairs(ctx, n));
  TRY(cell_grid_sort(ctx, static_cast<const float4*>(sp.p), nc, g, !require_finite, sorted.as<float4>(), cells.as<uint32_t>()));
  install_cell_grid(out, g, cells.as<uint32_t>(), sorted.as<float4>());
  // A neighbour is within `radius` of the query along every axis, i.e. within 1 / 1.01 = 0.9901 cells; the two float cell
  // coordinates floorf((s - o) * inv) are each off by at most 2^-23 of their magnitude: with up to 16 384 cells per axis that is
  // 0.004 cells together, so the neighbour's cell is the query's or next to it. Longer axes get one more cell each way.
  *reach = std::max(dim[0], std::max(dim[1], dim[2])) <= 16384 ? 1 : 2;
  return 0;
}
}  // namespace
