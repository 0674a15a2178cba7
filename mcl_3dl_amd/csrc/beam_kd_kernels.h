// beam_kd_kernels.h — beam model with the reference's DEFAULT raycaster (beam/use_raycast_using_dda = false):
// RaycastUsingKDTree marches along the ray in steps of the smallest map grid edge and asks the map's kd-tree for the
// nearest point around every position; here every such search is the exact nearest-within-radius over the cell-sorted
// map (LikGrid, cell_grid.h:cell_grid_nearest — the definition of mcl3dl_hip_radius_search).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "beam_kernels.h"
#include "cell_grid.h"
#include "device_math.h"
#include "map_structs.h"
#pragma clang fp contract(off)

namespace mcl3dl
{
// ---------------------------------------------------------------------------------------------------------
// Beam model: RaycastUsingKDTree (include/mcl_3dl/raycasts/raycast_using_kdtree.h:58-109) +
//             LidarMeasurementModelBeam::getBeamStatus (src/lidar_measurement_model_beam.cpp:157-192)
// ---------------------------------------------------------------------------------------------------------
// The caster's constants (RaycastUsingKDTree ctor, :49-56, from refreshParameters, beam.cpp:69-79) and what the searches need.
struct KdRayParams
{
  float grid_min;         // map_grid_min_
  float hit_tolerance;    // hit_tolerance_ = hit_range
  double two_grid_min;    // map_grid_min_ * 2.0 (:97)
  float r1_sq, r2_sq;     // (float)(r * r) of the two search radii, r widened to double (pcl::KdTreeFLANN::radiusSearch)
  int reach1, reach2;     // cells each way that cover the two radii on the grid in place
  float wx, wy, wz;       // dist_weight (1, 1, 1 when unset): the searches run in the rescaled metric
  int has_weight;
  const float4* map;      // the map in map order {x, y, z, label bits}: label filter and hit_range test use the unscaled point
  // dilated occupancy of the cell grid (kd_occupancy_kernel): bit c = some map point lies within reach1 cells of cell c, i.e.
  // in the cells the first search of a query in c looks at. Most steps of most rays are in free space: one load says so.
  const uint32_t* occ;
};

// One lane per cell, one 64-bit word per wavefront (cells in the grid's linear order, x fastest): the ballot is the word.
__global__ __launch_bounds__(256) void kd_occupancy_kernel(LikGrid g, int reach, unsigned long long n_cells,
                                                            unsigned long long* __restrict__ out)
{
  const unsigned long long c = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
  bool any = false;
  if (c < n_cells)
  {
    const int cx = static_cast<int>(c % static_cast<unsigned>(g.nx));
    const unsigned long long r = c / static_cast<unsigned>(g.nx);
    const int cy = static_cast<int>(r % static_cast<unsigned>(g.ny)), cz = static_cast<int>(r / static_cast<unsigned>(g.ny));
    const CellBlock b = cell_block(g, cx, cy, cz, reach);
    for (int z = b.z0; z <= b.z1; ++z)
      for (int y = b.y0; y <= b.y1; ++y)
      {
        if (any)
          continue;  // (a lane that has found a point loads no more delimiters)
        uint32_t s, e;
        cell_row_run(g, z, y, b.y1, b.x0, b.x1, s, e);
        any = e != s;
      }
  }
  const unsigned long long word = __ballot(any);
  if ((threadIdx.x & 63) == 0 && c < n_cells)
    out[c >> 6] = word;
}

// The searches. cell_grid_nearest (cell_grid.h) defines the result — min d2 below `best` over the cells within `reach` of
// the query's, flann::L2_Simple float order, ties to the lowest map index — and reads one row's run delimiters, then that
// run's points one by one: every load waits for the one before it, and a ray near a wall pays dozens of memory latencies per
// search. The forms below compute the same minimum over the same candidates with the loads batched: the delimiters of
// several rows together, four points per round (a round's indices are clamped to the run: a point looked at twice changes
// neither the minimum nor the tie).
__device__ inline void kd_scan_run(const float4* __restrict__ pts, uint32_t s, uint32_t e, float qx, float qy, float qz,
                                   float& best, int& best_idx)
{
  for (uint32_t k = s; k < e; k += 4)
  {
    const uint32_t last = e - 1;
    const float4 p0 = pts[k], p1 = pts[min(k + 1, last)], p2 = pts[min(k + 2, last)], p3 = pts[min(k + 3, last)];
    nearest_consider(p0, qx, qy, qz, best, best_idx);
    nearest_consider(p1, qx, qy, qz, best, best_idx);
    nearest_consider(p2, qx, qy, qz, best, best_idx);
    nearest_consider(p3, qx, qy, qz, best, best_idx);
  }
}

// one cell each way around an INTERIOR cell (cx, cy, cz): nine rows, their delimiters fetched together
__device__ inline float kd_nearest_27(const LikGrid& g, float qx, float qy, float qz, int cx, int cy, int cz, float best,
                                      int& best_idx)
{
  uint32_t rs[9], re[9];
  cell_rows_27(g, cx, cy, cz, rs, re);
#pragma unroll
  for (int r = 0; r < 9; ++r)
    kd_scan_run(g.pts, rs[r], re[r], qx, qy, qz, best, best_idx);
  return best;
}

// any reach, any query: the rows of a z layer five at a time
__device__ inline float kd_nearest(const LikGrid& g, float qx, float qy, float qz, int reach, float best, int& best_idx)
{
  CellBlock b;
  if (!cell_block_of(g, qx, qy, qz, reach, b))
    return best;
  for (int z = b.z0; z <= b.z1; ++z)
    for (int yb = b.y0; yb <= b.y1; yb += 5)
    {
      uint32_t rs[5], re[5];
#pragma unroll
      for (int j = 0; j < 5; ++j)
        cell_row_run(g, z, yb + j, b.y1, b.x0, b.x1, rs[j], re[j]);
#pragma unroll
      for (int j = 0; j < 5; ++j)
        kd_scan_run(g.pts, rs[j], re[j], qx, qy, qz, best, best_idx);
    }
  return best;
}

// Casts one ray; returns BeamStatus (0 SHORT, 1 HIT, 2 LONG, 3 TOTAL_REFLECTION). *hit = map index of the point the status
// was decided on (-1: LONG).
__device__ inline int cast_ray_kd(const LikGrid& g, const KdRayParams& k, const BeamParams& bp, const Vec3f b, const Vec3f e,
                                  int* hit)
{
  *hit = -1;
  // setRay, :58-66
  const Vec3f diff = vsub(e, b);
  const float nrm = sqrtf(vdot(diff, diff));
  const float len_f = floorf((nrm + k.hit_tolerance) / k.grid_min);
  // a non-finite end point (its norm is infinite or NaN; the reference converts that to int: undefined) and a length no int
  // holds end at once — NaN fails the comparison
  if (!(len_f < 2147483648.0f))
    return 2;
  const int length = static_cast<int>(len_f);
  const Vec3f inc = vscale(Vec3f{ diff.x / nrm, diff.y / nrm, diff.z / nrm }, k.grid_min);
  Vec3f pos = vadd(b, inc);
  // which way the rescaled position moves per axis (it is a monotone float recurrence): > 0 up, < 0 down, 0 not at all
  // (NaN — a zero-length ray — compares false both ways: no early exit, the few steps find nothing)
  const float mx = (k.has_weight && k.wx < 0.f) ? -inc.x : inc.x, my = (k.has_weight && k.wy < 0.f) ? -inc.y : inc.y,
              mz = (k.has_weight && k.wz < 0.f) ? -inc.z : inc.z;
  const float lo = -static_cast<float>(k.reach1);
  const float hx = static_cast<float>(g.nx - 1 + k.reach1), hy = static_cast<float>(g.ny - 1 + k.reach1),
              hz = static_cast<float>(g.nz - 1 + k.reach1);
  // getNextCastResult, :68-109, as two nested loops (the "while-while" form of beam_kernels.h): the inner loop only WALKS —
  // through steps whose occupancy bit says that the search finds nothing — and ends, for a wavefront, when every ray stands at
  // a step that has to search (or has run out); the searches of that step then run once for all 64 rays together instead of
  // once per step for whichever ray happens to be near a surface. The per-ray sequence of operations is unchanged.
  int count = 1;
  int status = 2;
  while (count < length)
  {
    float qx = 0.f, qy = 0.f, qz = 0.f;
    int cx = 0, cy = 0, cz = 0;
    bool search = false, interior = false;
    while (count < length)
    {
      qx = pos.x;
      qy = pos.y;
      qz = pos.z;
      if (k.has_weight)
      {
        qx = qx * k.wx;
        qy = qy * k.wy;
        qz = qz * k.wz;
      }
      // Past the cell grid by more than the search's reach on an axis the ray is moving away on: this search and every later
      // one finds nothing (cell_block_of's own range test, on a coordinate that only moves further out) — LONG
      const Vec3f f = cell_of(g, qx, qy, qz);
      const float fx = f.x, fy = f.y, fz = f.z;
      if ((mx >= 0.f && fx > hx) || (mx <= 0.f && fx < lo) || (my >= 0.f && fy > hy) || (my <= 0.f && fy < lo) ||
          (mz >= 0.f && fz > hz) || (mz <= 0.f && fz < lo))
      {
        count = length;
        break;
      }
      // a query inside the grid: its cell's bit says whether the search can find anything at all (NaN fails the comparisons
      // and goes to the general search, which finds nothing)
      const bool inside = fx >= 0.f && fy >= 0.f && fz >= 0.f && fx <= static_cast<float>(g.nx - 1) &&
                          fy <= static_cast<float>(g.ny - 1) && fz <= static_cast<float>(g.nz - 1);
      search = true;
      interior = false;
      if (inside)
      {
        cx = static_cast<int>(fx);
        cy = static_cast<int>(fy);
        cz = static_cast<int>(fz);
        const size_t c = (static_cast<size_t>(cz) * g.ny + cy) * g.nx + cx;
        search = ((k.occ[c >> 5] >> (c & 31)) & 1u) != 0u;
        interior = k.reach1 == 1 && cx >= 1 && cy >= 1 && cz >= 1 && cx <= g.nx - 2 && cy <= g.ny - 2 && cz <= g.nz - 2;
      }
      if (search)
        break;
      ++count;
      pos = vadd(pos, inc);
    }
    if (!search)
      break;
    int id = -1;
    const float sq0 = interior ? kd_nearest_27(g, qx, qy, qz, cx, cy, cz, k.r1_sq, id) :
                                 kd_nearest(g, qx, qy, qz, k.reach1, k.r1_sq, id);  // :83
    // getBeamStatus, beam.cpp:164-170: a collision with a filtered label is passed over (its sin_angle is never looked at)
    if (id >= 0 && !(__float_as_uint(k.map[id].w) > bp.filter_label_max))
    {
      const float4 m = k.map[id];
      const float d0 = sqrtf(sq0);
      // :91-104: the surface's inclination from a second search two steps back
      const Vec3f prev = vsub(pos, vscale(inc, 2.0f));
      float px = prev.x, py = prev.y, pz = prev.z;
      if (k.has_weight)
      {
        px = px * k.wx;
        py = py * k.wy;
        pz = pz * k.wz;
      }
      int id1 = -1;
      const float sq1 = kd_nearest(g, px, py, pz, k.reach2, k.r2_sq, id1);  // :94
      float sin_ang = 1.0f;
      if (id1 >= 0)
      {
        const float d1 = sqrtf(sq1);
        sin_ang = static_cast<float>(fabs(static_cast<double>(d1 - d0)) / k.two_grid_min);  // :97
      }
      // beam.cpp:170-187
      *hit = id;
      status = 3;
      if (sin_ang > bp.sin_total_ref)
        status = beam_hit_or_short(bp, e, Vec3f{ m.x, m.y, m.z });
      break;
    }
    ++count;
    pos = vadd(pos, inc);
  }
  return status;
}

// One lane per (particle, beam point), rays of a particle next to each other: beam_kernel's frame (beam_kernels.h:beam_body)
// around this caster — the kernels behind it (beam_finalize_kernel or pf::measure's first) do not know which caster ran.
__global__ __launch_bounds__(256) void beam_kd_kernel(const float* __restrict__ pose7, const float4* __restrict__ scan, int n_b,
                                                      const float4* __restrict__ origins, long long n_rays, LikGrid g,
                                                      KdRayParams k, BeamParams bp, unsigned* __restrict__ penalty_count)
{
  const long long ray0 = static_cast<long long>(blockIdx.x) * 256;
  const long long ray = ray0 + threadIdx.x;
  __shared__ unsigned block_count[2];
  if (threadIdx.x < 2)
    block_count[threadIdx.x] = 0u;
  __syncthreads();
  const long long p0 = ray0 / n_b;
  bool penalised = false;
  long long p = p0;
  if (ray < n_rays)
  {
    p = ray / n_b;
    const int i = static_cast<int>(ray - p * n_b);
    const float4 v = scan[i];
    const float* ps = pose7 + 7 * p;
    const Vec3f pos = { ps[0], ps[1], ps[2] };
    const Quat raw = { ps[3], ps[4], ps[5], ps[6] };
    const Vec3f end = beam_ray_end(pos, qnormalized(raw), Vec3f{ v.x, v.y, v.z });
    const float4 og = origins[__float_as_uint(v.w)];
    const Vec3f begin = beam_ray_begin(pos, raw, Vec3f{ og.x, og.y, og.z });
    int hit;
    penalised = beam_penalised(bp, cast_ray_kd(g, k, bp, begin, end, &hit));
  }
  beam_count_penalised(penalised, p, p0, block_count, penalty_count);
}

// LidarMeasurementModelBeam::getBeamStatus for explicit rays with the kd-tree caster (debug-marker path, src/mcl_3dl.cpp:471-478).
__global__ void beam_kd_status_kernel(const float* __restrict__ begin_xyz, const float* __restrict__ end_xyz, int n, LikGrid g,
                                      KdRayParams k, BeamParams bp, int* __restrict__ status, int* __restrict__ hit_index)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  int hit;
  const int s = cast_ray_kd(g, k, bp, Vec3f{ begin_xyz[3 * i], begin_xyz[3 * i + 1], begin_xyz[3 * i + 2] },
                            Vec3f{ end_xyz[3 * i], end_xyz[3 * i + 1], end_xyz[3 * i + 2] }, &hit);
  status[i] = s;
  if (hit_index)
    hit_index[i] = (s == 2) ? -1 : hit;
}

}  // namespace mcl3dl
