// cell_grid.h — the walk over the cell-sorted map (LikGrid, map_structs.h: run delimiters in cell_start, one contiguous run of
// pts per (z, y) row), stated once for every kernel that runs it: the cell of a query, the block of cells within a reach, a
// row's run, the nine rows around an interior cell, flann::L2_Simple's distance with the tie rule, and cell_grid_nearest — the
// definition of mcl3dl_hip_radius_search. Callers that batch their loads (likelihood_kernels.h:nearest_d2, beam_kd_kernels.h,
// sampler_kernels.h) keep the batching and take everything else from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "map_structs.h"
#pragma clang fp contract(off)

namespace mcl3dl
{
// flann::L2_Simple<float>: ((0 + dx*dx) + dy*dy) + dz*dz, float, no contraction
__device__ inline float d2_simple(float qx, float qy, float qz, float px, float py, float pz)
{
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  float d2 = dx * dx;
  d2 = d2 + dy * dy;
  d2 = d2 + dz * dz;
  return d2;
}

// cell of a query, as floats: (q - o) * inv is the float expression the builders bin the map points with (index_geometry.h)
__device__ inline Vec3f cell_of(const LikGrid& g, float qx, float qy, float qz)
{
  return { floorf((qx - g.ox) * g.inv_cell), floorf((qy - g.oy) * g.inv_cell), floorf((qz - g.oz) * g.inv_cell) };
}

struct CellBlock
{
  int x0, x1, y0, y1, z0, z1;
};

// the cells within `reach` of cell (cx, cy, cz), clamped to the grid
__device__ inline CellBlock cell_block(const LikGrid& g, int cx, int cy, int cz, int reach)
{
  return { max(cx - reach, 0), min(cx + reach, g.nx - 1), max(cy - reach, 0),
           min(cy + reach, g.ny - 1), max(cz - reach, 0), min(cz + reach, g.nz - 1) };
}

// the cells within `reach` of the query's; false = nothing to search: a query further than `reach` cells outside the grid, or a
// NaN coordinate (the comparisons fail)
__device__ inline bool cell_block_of(const LikGrid& g, float qx, float qy, float qz, int reach, CellBlock& b)
{
  const Vec3f f = cell_of(g, qx, qy, qz);
  if (!(f.x >= -static_cast<float>(reach) && f.y >= -static_cast<float>(reach) && f.z >= -static_cast<float>(reach) &&
        f.x <= static_cast<float>(g.nx - 1 + reach) && f.y <= static_cast<float>(g.ny - 1 + reach) &&
        f.z <= static_cast<float>(g.nz - 1 + reach)))
    return false;
  b = cell_block(g, static_cast<int>(f.x), static_cast<int>(f.y), static_cast<int>(f.z), reach);
  return b.x0 <= b.x1;
}

// run delimiters of the cells [x0, x1] of row (z, y); a row past y1 is an empty run (for callers that fetch a fixed number of
// rows together)
__device__ inline void cell_row_run(const LikGrid& g, int z, int y, int y1, int x0, int x1, uint32_t& s, uint32_t& e)
{
  const bool in = y <= y1;
  const size_t row = (static_cast<size_t>(z) * g.ny + (in ? y : y1)) * g.nx;
  s = g.cell_start[row + x0];
  e = in ? g.cell_start[row + x1 + 1] : s;
}

// one cell each way around an INTERIOR cell (cx, cy, cz): the delimiters of its nine rows, fetched together
__device__ inline void cell_rows_27(const LikGrid& g, int cx, int cy, int cz, uint32_t (&rs)[9], uint32_t (&re)[9])
{
#pragma unroll
  for (int r = 0; r < 9; ++r)
  {
    const int dz = r / 3 - 1, dy = r % 3 - 1;
    const size_t row = (static_cast<size_t>(cz + dz) * g.ny + (cy + dy)) * g.nx + cx;
    rs[r] = g.cell_start[row - 1];
    re[r] = g.cell_start[row + 2];
  }
}

// one candidate of a nearest-point search: p replaces the best so far when it is nearer, or as near with a lower map index
__device__ inline void nearest_consider(const float4 p, float qx, float qy, float qz, float& best, int& best_idx)
{
  const float d2 = d2_simple(qx, qy, qz, p.x, p.y, p.z);
  const int idx = static_cast<int>(__float_as_uint(p.w));
  if (d2 < best || (d2 == best && best_idx >= 0 && idx < best_idx))
  {
    best = d2;
    best_idx = idx;
  }
}

// ChunkedKdtree::radiusSearch(p, radius, id, sqdist, 1) (include/mcl_3dl/chunked_kdtree.h:217-237) for ANY radius: the nearest
// map point to the (already rescaled) query among the cells within `reach` of its own: min d2 below `best` (initialised by the
// caller with (float)(radius * radius)), ties to the lowest map index; best_idx stays as it is when there is none.
__device__ inline float cell_grid_nearest(const LikGrid& g, float qx, float qy, float qz, int reach, float best,
                                          int& best_idx)
{
  CellBlock b;
  if (!cell_block_of(g, qx, qy, qz, reach, b))
    return best;
  for (int z = b.z0; z <= b.z1; ++z)
    for (int y = b.y0; y <= b.y1; ++y)
    {
      uint32_t s, e;
      cell_row_run(g, z, y, b.y1, b.x0, b.x1, s, e);
      for (uint32_t k = s; k < e; ++k)
        nearest_consider(g.pts[k], qx, qy, qz, best, best_idx);
    }
  return best;
}
}  // namespace mcl3dl
