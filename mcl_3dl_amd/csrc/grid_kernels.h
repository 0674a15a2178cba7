// grid_kernels.h — device side of the two linear-time map structures: the cell-sorted exact-NN grid (LikGrid: radius
// search, matched / unmatched, lik_index = 0, the K-bar statistics) and the DDA occupancy + voxel index (DdaGrid). Both
// are counting sorts of the map by a cell id: key per point -> stable radix sort of (key, map index) -> gather; the run
// delimiters come from a histogram (one atomic per point) and an exclusive scan. Same keys, same order inside a cell
// (ascending map index) as a sequential counting sort on the host: the structures are bit-identical to what
// host_grid_builders.h:build_*_grid_host lays out, and the keys are the same functions there and here (index_geometry.h:
// cell_index, dda_voxel_coord / dda_voxel_index, dda_brick_of / dda_brick_bit). tests/test_gpu_grid_builders.py and
// tests/test_gpu_map_path.py compare results under both forms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_geometry.h"
#include "map_structs.h"
#pragma clang fp contract(off)

namespace mcl3dl
{
// PointRepresentation::vectorize (one float product per coordinate when a dist_weight is set); w = map index
__global__ void grid_rescale_kernel(const float4* __restrict__ map, long long n, float wx, float wy, float wz, int has_weight,
                                    float4* __restrict__ out)
{
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float4 p = map[i];
  out[i] = make_float4(has_weight ? p.x * wx : p.x, has_weight ? p.y * wy : p.y, has_weight ? p.z * wz : p.z,
                       __uint_as_float(static_cast<uint32_t>(i)));
}

// cell of every rescaled point (index_geometry.h:cell_index) + the cells' histogram. ANY: the cloud may hold non-finite
// points (a scan, build_transient_cell_grid), which go to cell 0 by decree (cell_index_any)
template <bool ANY>
__global__ void lik_cell_key_kernel(const float4* __restrict__ sp, long long n, CellGridGeometry g, uint32_t* __restrict__ key,
                                    uint32_t* __restrict__ val, uint32_t* __restrict__ count)
{
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float4 p = sp[i];
  const uint32_t k = ANY ? cell_index_any(g, p.x, p.y, p.z) : cell_index(g, p.x, p.y, p.z);
  key[i] = k;
  val[i] = static_cast<uint32_t>(i);
  atomicAdd(&count[k], 1u);
}

// ---- the cell grid after a map update: merge of the BASE map's grid with the update's points (round 5) -------------------
// pc_map2 = pc_map + pc_update (src/mcl_3dl.cpp:150): the update's points have the highest map indices, so inside a cell they
// follow the base points — the merged, cell-sorted array is the base array with every cell's run shifted by the number of
// update points in the cells before it, and the update's points (sorted by cell, stable) appended to their cells' runs.
// ukey = the update's cell keys, ascending (n_u of them). No histogram, no sort of the map: one binary search per cell / point.
__device__ inline uint32_t lower_bound_u32(const uint32_t* __restrict__ a, uint32_t n, uint32_t v)
{
  uint32_t lo = 0, hi = n;
  while (lo < hi)
  {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ void lik_update_key_kernel(const float4* __restrict__ sp_upd, int n_u, CellGridGeometry g, uint32_t* __restrict__ key,
                                      uint32_t* __restrict__ val)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_u)
    return;
  const float4 p = sp_upd[i];
  key[i] = cell_index(g, p.x, p.y, p.z);
  val[i] = static_cast<uint32_t>(i);
}

// (measured and not kept: one search per run of eight consecutive cells / points followed by a linear walk of the keys —
// 0.138 ms instead of 0.112 at C2: the strided runs cost more in uncoalesced accesses than the searches they save)
__global__ void lik_merge_cells_kernel(const uint32_t* __restrict__ base_start, long long n_cell_plus_1,
                                       const uint32_t* __restrict__ ukey, uint32_t n_u, uint32_t* __restrict__ out_start)
{
  const long long c = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c < n_cell_plus_1)
    out_start[c] = base_start[c] + lower_bound_u32(ukey, n_u, static_cast<uint32_t>(c));
}

__global__ void lik_merge_points_kernel(const float4* __restrict__ base_pts, long long n_base,
                                        const uint32_t* __restrict__ base_start, CellGridGeometry g,
                                        const float4* __restrict__ sp_upd, const uint32_t* __restrict__ ukey,
                                        const uint32_t* __restrict__ uval, uint32_t n_u, float4* __restrict__ out_pts)
{
  const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t < n_base)
  {
    const float4 p = base_pts[t];
    out_pts[t + lower_bound_u32(ukey, n_u, cell_index(g, p.x, p.y, p.z))] = p;
  }
  else if (t < n_base + n_u)
  {
    const uint32_t j = static_cast<uint32_t>(t - n_base);
    out_pts[static_cast<size_t>(base_start[ukey[j] + 1u]) + j] = sp_upd[uval[j]];
  }
}

__global__ void grid_gather_kernel(const float4* __restrict__ src, const uint32_t* __restrict__ val, long long n,
                                   float4* __restrict__ dst)
{
  const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k < n)
    dst[k] = src[val[k]];
}

// voxel of every map point (index_geometry.h: dda_voxel_coord, dda_voxel_index) + the voxels' histogram + setExists -> the
// voxel's bit in its 4x4x4 brick word (dda_brick_of)
__global__ void dda_voxel_key_kernel(const float4* __restrict__ map, long long n, DdaGeom g, uint32_t* __restrict__ key,
                                     uint32_t* __restrict__ val, uint32_t* __restrict__ count,
                                     unsigned long long* __restrict__ bricks, int* __restrict__ err)
{
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float4 p = map[i];
  const int c0 = dda_voxel_coord(p.x, g.mn[0], g.grid), c1 = dda_voxel_coord(p.y, g.mn[1], g.grid),
            c2 = dda_voxel_coord(p.z, g.mn[2], g.grid);
  const size_t v = static_cast<size_t>(dda_voxel_index(g, c0, c1, c2));
  val[i] = static_cast<uint32_t>(i);
  if (v >= g.total)
  {
    key[i] = 0xffffffffu;  // "map point falls outside its own DDA grid"
    atomicMax(err, 1);
    return;
  }
  key[i] = static_cast<uint32_t>(v);
  atomicAdd(&count[v], 1u);
  size_t brick;
  unsigned long long bit;
  dda_brick_of(g, c0, c1, c2, brick, bit);
  atomicOr(&bricks[brick], bit);
}

// points in voxel order (insertion = map order inside a voxel: the sort is stable) + their original map index
__global__ void dda_gather_kernel(const float4* __restrict__ map, const uint32_t* __restrict__ val, long long n,
                                  float4* __restrict__ pts, uint32_t* __restrict__ index)
{
  const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  const uint32_t i = val[k];
  pts[k] = map[i];
  index[k] = i;
}

// ---- the DDA overlay of a map update (DdaGrid::ov_*) ---------------------------------------------------------------------
// voxel keys of the update's points (all inside the grid: the host checked them against the grid's bounds)
__global__ void dda_overlay_key_kernel(const float4* __restrict__ upd, int n, DdaGeom g, uint32_t* __restrict__ key,
                                       uint32_t* __restrict__ val)
{
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n)
    return;
  const float4 p = upd[i];
  key[i] = static_cast<uint32_t>(dda_voxel_index(g, dda_voxel_coord(p.x, g.mn[0], g.grid), dda_voxel_coord(p.y, g.mn[1], g.grid),
                                                  dda_voxel_coord(p.z, g.mn[2], g.grid)));
  val[i] = static_cast<uint32_t>(i);
}

// the previous overlay goes: a voxel that holds no base point is empty again
__global__ void dda_overlay_clear_kernel(const uint32_t* __restrict__ old_key, int n, DdaGeom g,
                                         const uint32_t* __restrict__ vox_start, unsigned long long* __restrict__ bricks)
{
  const int k = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= n)
    return;
  const uint32_t v = old_key[k];
  if (vox_start[v + 1] != vox_start[v])
    return;
  size_t brick;
  unsigned long long bit;
  dda_brick_bit(g, v, brick, bit);
  atomicAnd(&bricks[brick], ~bit);
}

// the sorted overlay arrays + the occupancy bits of the new update
__global__ void dda_overlay_set_kernel(const float4* __restrict__ upd, const uint32_t* __restrict__ skey,
                                       const uint32_t* __restrict__ sval, int n, DdaGeom g, uint32_t* __restrict__ ov_key,
                                       float4* __restrict__ ov_pts, uint32_t* __restrict__ ov_idx,
                                       unsigned long long* __restrict__ bricks)
{
  const int k = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= n)
    return;
  const uint32_t v = skey[k], i = sval[k];
  ov_key[k] = v;
  ov_pts[k] = upd[i];
  ov_idx[k] = i;
  size_t brick;
  unsigned long long bit;
  dda_brick_bit(g, v, brick, bit);
  atomicOr(&bricks[brick], bit);
}

}  // namespace mcl3dl
