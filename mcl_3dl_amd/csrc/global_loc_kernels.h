// global_loc_kernels.h — global localisation (cbGlobalLocalization, src/mcl_3dl.cpp:1039-1099): the "is something right above
// this point?" test over the VoxelGrid centroids of the base map, and the seeding of div_yaw yaw hypotheses per surviving
// point straight into a shard of resident particles. The VoxelGrid itself is cloud_kernels.h's, the compaction its
// compact_kernel, the centroid index the cell-sorted grid of grid_kernels.h built over the centroid cloud (api_global_loc.inl).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_grid.h"
#include "cloud_kernels.h"
#include "device_math.h"
#include "map_structs.h"
#pragma clang fp contract(off)

namespace mcl3dl
{
// One thread per centroid p: p2 = p, p2.z += 0.01 + grid (a double sum, narrowed on the store: src/mcl_3dl.cpp:1066-1067),
// then kdtree->radiusSearch(p2, grid, id, sqdist, 1) over the centroid cloud itself in the dist_weight metric. flag = 1 when
// NOTHING is found (the point stays), 0 when some centroid — possibly p itself — lies within the radius (remove_if drops it).
// `g` is a cell grid over the rescaled centroids; the search and its float arithmetic are cell_grid_nearest's, the function
// match_split and the stand-alone radius search decide with. flag has n + 1 entries (the last one 0: room for the scan's total).
__global__ void gl_blocked_flag_kernel(const float4* __restrict__ centroids, long long n, double shift, LikGrid g,
                                       LikParams prm, float r2, int reach, uint32_t* __restrict__ flag)
{
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i > n)
    return;
  if (i == n)
  {
    flag[i] = 0;
    return;
  }
  const float4 c = centroids[i];
  float qx = c.x, qy = c.y, qz = static_cast<float>(static_cast<double>(c.z) + shift);
  if (prm.has_weight)
  {
    qx = qx * prm.wx;
    qy = qy * prm.wy;
    qz = qz * prm.wz;
  }
  int idx = -1;
  (void)cell_grid_nearest(g, qx, qy, qz, reach, r2, idx);
  flag[i] = idx < 0 ? 1u : 0u;
}

// Particles [first, first + count) of the seeded set, particle i = point i / div_yaw with rotation i % div_yaw
// (src/mcl_3dl.cpp:1076-1095): state13 = { position, rotation, odom_err_integ_lin = 0, odom_err_integ_ang = 0 }, pose7 its
// first seven floats, weight = 1 / points for every particle. A particle's 13 floats are not 16-byte aligned, so the work is
// laid out by output dword of state13: consecutive lanes store consecutive dwords (whole 256-byte lines per wavefront); the
// lanes that hold a pose component store it to pose7 too (seven consecutive dwords out of every thirteen lanes), the lane of
// dword 7 stores the weight. Reads are two small tables (points, div_yaw rotations) hit by dozens of neighbouring lanes each.
// Any of the three outputs may be null; each starts at particle `first`.
__global__ void gl_seed_kernel(const float4* __restrict__ points, const float* __restrict__ rot4, unsigned div_yaw,
                               unsigned long long first, unsigned long long count, float weight,
                               float* __restrict__ state13, float* __restrict__ pose7, float* __restrict__ out_weight)
{
  const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= 13ull * count)
    return;
  const unsigned long long j = t / 13ull;  // particle of this shard
  const unsigned k = static_cast<unsigned>(t - 13ull * j);
  const unsigned long long i = first + j;
  const unsigned long long pt = i / div_yaw;
  const unsigned yaw = static_cast<unsigned>(i - pt * div_yaw);
  float v = 0.0f;
  if (k < 3)
  {
    const float4 p = points[pt];
    v = k == 0 ? p.x : (k == 1 ? p.y : p.z);
  }
  else if (k < 7)
    v = rot4[4u * yaw + (k - 3)];
  if (state13)
    state13[t] = v;
  if (pose7 && k < 7)
    pose7[7ull * j + k] = v;
  if (out_weight && k == 7)
    out_weight[j] = weight;
}
}  // namespace mcl3dl
