// index_geometry.h — the pure arithmetic of the map structures' geometry, free of HIP so that a plain C++ program can include
// it (tests/cpp/voxel_slack_check.cpp and tests/cpp/grid_keys_check.cpp run it on the host): the candidate-voxel grid
// (map_compiler.h, host_map_compilers.h) — edges, their float reciprocals, the slack `grow` of V+, reach, origin, voxel and
// brick counts — and, stated once for the kernels of grid_kernels.h and the host forms of host_grid_builders.h alike, the
// map's cell grid (origin, edge, dimensions, cell of a point), the DDA grid (dimensions, voxel of a point, brick word and
// bit) and the stable counting sort both host forms lay their arrays out with.
//
// The slack. A query q gets, per axis, the voxel
//     v = floor(t),  t = fl(fl(q - o) * inv_e),  inv_e = fl(1 / e)           (float; o, e floats)
// and the candidate proof needs q inside V+ = [o + v e - grow, o + (v + 1) e + grow]. With u = 2^-24 (half an ulp, relative):
//     fl(q - o) = (q - o)(1 + d1),  inv_e = (1 / e)(1 + d2),  the product's rounding (1 + d3),  |d1|, |d2|, |d3| <= u
// (d1 is relative to the DIFFERENCE whatever the magnitudes of q and o are: a float subtraction is correctly rounded), so
//     t = ((q - o) / e)(1 + th),  |th| <= (1 + u)^3 - 1 < 3.0000004 u,
// and v <= t < v + 1 puts (q - o) / e inside [v, v + 1] widened by (v + 1) |th| / (1 - |th|) voxels on either side: q lies
// inside V+ when grow >= 3.0000008 u (v + 1) e. v + 1 is at most the axis' voxel count n, and n e is the length L of the grid
// along the axis; the compiler's own fp64 faces o + v e carry another 2^-52 (|o| + L). Hence, from the longest axis,
//     derived = 3.25 * 2^-24 * L_max + 2^-50 * (max |coordinate| + L_max)      (3.25: 8 % of headroom over 3.0000008)
//     grow    = max(1e-3 * e_min, derived)
// The first term wins while L_max < 5 162 e_min (a map of 516 m at e = 0.1 m): every shorter grid keeps the slack it always had.
// A coordinate x past 2 048 m whose float spacing exceeds 1e-3 e is inside the bound: its spacing is at most 2 u x, under two
// thirds of the slack derived for a grid long enough to reach it.
// Limit: grow <= e_min / 16 (CAND_GROW_MAX_FRACTION), i.e. L_max <= 322 000 e_min (32 km at e = 0.1 m): beyond, the build is
// refused. At a sixteenth of a voxel V+ is an eighth wider than V per axis and its candidate sets are still those of a voxel
// an eighth larger; the float t itself then has a spacing of a thirty-second of a voxel (t < 2^19), past which `floor(t)`
// stops naming a voxel in any useful sense.
//
// The map's cell grid (nearest_d2's 27-cell scan): cell = fl(1.01f r), c = floor(fl(fl(s - o) * inv)). Two coordinates a, b
// closer than r along an axis get t_a - t_b = ((a - b) / cell)(1 + d2) + (rounding of the two differences and the two
// products) with |a - b| / cell <= 1 / 1.0099999 (1 + 2u) < 0.9901005 and roundings of at most 2 u t each: the two cells
// differ by at most one while 0.9901005 + 4.0000005 u n < 1, n < 41 519 cells per axis. LIK_SCAN_MAX_CELLS = 40 000 (8 km at
// r = 0.2 m); the 27-cell scan is refused on a longer grid (radius_search scans a cell more each way and is not).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define MCL3DL_GEOM_HD __host__ __device__
#else
#define MCL3DL_GEOM_HD
#endif

namespace mcl3dl
{
struct CompileParams
{
  float ox, oy, oz, inv_ex, inv_ey, inv_ez;
  double ex, ey, ez;  // voxel edges (rescaled coordinates). Every step of the candidate proof is per axis (boxes V, V+), so a
                      // voxel may be a box: dist_weight stretches the map along an axis and thins its points out there in the
                      // metric — an edge stretched likewise keeps the candidates per voxel and divides the voxel count
  double grow;    // V+ = V grown by this on every side
  double r2_hi;   // (r*(1+1e-5))^2
  double margin;  // domination margin m
  int rx, ry, rz;  // voxels to visit around a point's own voxel, per axis
  int nvx, nvy, nvz, nbx, nby, nbz;
  int n_points;
};

// voxel (or cell) coordinate of q along one axis: THE float expression — voxel_of (map_compiler.h), rec_locate and
// nearest_d2 (likelihood_kernels.h, with their own floor instruction), the host builders. No contraction is possible in it.
MCL3DL_GEOM_HD inline float grid_coord(float q, float o, float inv_edge)
{
  return floorf((q - o) * inv_edge);
}

constexpr double CAND_GROW_MIN_FRACTION = 1e-3;         // of the shortest edge: the slack of every grid below ~5 000 voxels
constexpr double CAND_GROW_MAX_FRACTION = 1.0 / 16.0;   // of the shortest edge: beyond, no index is built
constexpr double CAND_GROW_PER_LENGTH = 3.25 / 16777216.0;
constexpr double CAND_MAX_TABLE = 2.0e9;                // entries of the dense brick table

enum CandGeomStatus
{
  CAND_GEOM_OK = 0,
  CAND_GEOM_BAD_EDGE = 1,   // an edge that is not a positive finite float
  CAND_GEOM_SLACK = 2,      // the derived slack exceeds CAND_GROW_MAX_FRACTION of the shortest edge (*detail = slack / e_min)
  CAND_GEOM_TABLE = 3,      // the dense brick table would exceed CAND_MAX_TABLE entries (*detail = entries)
};

// Slack a grid of length `length` (longest axis) whose coordinates stay below `max_abs` in magnitude needs (header comment).
inline double cand_derived_grow(double length, double max_abs)
{
  return CAND_GROW_PER_LENGTH * length + (max_abs + length) / 1125899906842624.0;
}

// Geometry of the candidate-voxel grid for a point set with the bounds mn .. mx (rescaled coordinates), search radius r,
// voxel edge voxel_ratio * r * stretch[axis], origin phase `phase` (option cand_phase). n_points is left 0.
inline CandGeomStatus cand_grid_geometry(double r, double voxel_ratio, const double stretch[3], double phase, const float mn[3],
                                         const float mx[3], CompileParams* out, long long* n_table_out, double* detail)
{
  float e_f[3];
  for (int a = 0; a < 3; ++a)
  {
    e_f[a] = static_cast<float>(r * voxel_ratio * stretch[a]);
    if (!(e_f[a] > 0.f) || !std::isfinite(e_f[a]))
      return CAND_GEOM_BAD_EDGE;
  }
  CompileParams cp{};
  cp.ex = static_cast<double>(e_f[0]);
  cp.ey = static_cast<double>(e_f[1]);
  cp.ez = static_cast<double>(e_f[2]);
  cp.inv_ex = 1.0f / e_f[0];
  cp.inv_ey = 1.0f / e_f[1];
  cp.inv_ez = 1.0f / e_f[2];
  const double ed[3] = { cp.ex, cp.ey, cp.ez };
  const double e_min = fmin(cp.ex, fmin(cp.ey, cp.ez));
  const double r_hi = r * (1.0 + 1e-5);
  cp.r2_hi = r_hi * r_hi;
  cp.margin = 1e-5 * r * r;
  // the slack, from an upper bound of the grid's length: the bounds, the widest reach any admissible slack gives, the
  // origin's margin and phase (the length itself depends on the reach, which depends on the slack)
  double length = 0.0, max_abs = 0.0;
  for (int a = 0; a < 3; ++a)
  {
    const double reach_hi = floor((r_hi + 2.0 * CAND_GROW_MAX_FRACTION * e_min) / ed[a]) + 1.0;
    const double l = (static_cast<double>(mx[a]) - static_cast<double>(mn[a])) + (2.0 * reach_hi + 6.0) * ed[a];
    length = fmax(length, l);
    max_abs = fmax(max_abs, fmax(fabs(static_cast<double>(mn[a])), fabs(static_cast<double>(mx[a]))));
  }
  const double derived = cand_derived_grow(length, max_abs);
  if (!(derived <= CAND_GROW_MAX_FRACTION * e_min))
  {
    if (detail)
      *detail = derived / e_min;
    return CAND_GEOM_SLACK;
  }
  cp.grow = fmax(CAND_GROW_MIN_FRACTION * e_min, derived);
  // a point lies up to `grow` outside its own voxel and V+ reaches `grow` beyond V: a voxel whose V+ comes within r_hi of the
  // point is at most ceil((r_hi + 2 grow) / e) <= floor((r_hi + 2 grow) / e) + 1 voxels from the point's own
  int reach[3];
  for (int a = 0; a < 3; ++a)
    reach[a] = static_cast<int>(floor((r_hi + 2.0 * cp.grow) / ed[a])) + 1;
  cp.rx = reach[0];
  cp.ry = reach[1];
  cp.rz = reach[2];
  float o[3];
  int nv[3], nb[3];
  double n_table_d = 1;
  for (int a = 0; a < 3; ++a)
  {
    // Phase: maps that come out of a voxel filter sit on a lattice; with the origin ON that lattice every voxel face
    // coincides with a Voronoi face of the map and each voxel keeps 3 candidates per axis instead of the 2 a generic
    // position needs. Half a voxel of phase puts lattice maps in the generic position; arbitrary maps do not care.
    o[a] = mn[a] - static_cast<float>((reach[a] + 1 + phase) * ed[a]);
    const double nv_d = floor((static_cast<double>(mx[a]) - o[a]) / ed[a]) + reach[a] + 2;
    if (!(nv_d < 2.0e9))
    {
      if (detail)
        *detail = nv_d;
      return CAND_GEOM_TABLE;
    }
    nv[a] = static_cast<int>(nv_d);
    nb[a] = (nv[a] + 7) / 8;
    n_table_d *= nb[a];
  }
  if (n_table_d > CAND_MAX_TABLE)
  {
    if (detail)
      *detail = n_table_d;
    return CAND_GEOM_TABLE;
  }
  cp.ox = o[0];
  cp.oy = o[1];
  cp.oz = o[2];
  cp.nvx = nv[0];
  cp.nvy = nv[1];
  cp.nvz = nv[2];
  cp.nbx = nb[0];
  cp.nby = nb[1];
  cp.nbz = nb[2];
  *out = cp;
  *n_table_out = static_cast<long long>(n_table_d);
  return CAND_GEOM_OK;
}

// ---- the map's cell grid (LikGrid): cubes of `cell`, two cells of margin below the bounds, one above ------------------------
struct CellGridGeometry
{
  float o[3];
  float inv;
  int dim[3];
};

constexpr int LIK_SCAN_MAX_CELLS = 40000;  // per axis: up to here two coordinates within the radius lie in adjacent cells

// (an axis of 2^31 cells and more counts as INT_MAX cells: every caller refuses such a grid by its cell count)
MCL3DL_GEOM_HD inline CellGridGeometry cell_grid_geometry(const float mn[3], const float mx[3], float cell)
{
  CellGridGeometry g;
  g.inv = 1.0f / cell;
  for (int a = 0; a < 3; ++a)
  {
    g.o[a] = mn[a] - 2.0f * cell;
    const float c = grid_coord(mx[a], g.o[a], g.inv);
    g.dim[a] = c < 2147483520.0f ? static_cast<int>(c) + 3 : 2147483647;
  }
  return g;
}

MCL3DL_GEOM_HD inline int clamp_coord(int c, int n)
{
  const int lo = c > 0 ? c : 0;  // max, then min: one instruction each on the device
  return lo < n - 1 ? lo : n - 1;
}

// Cell of a rescaled, finite point: grid_coord per axis, clamped into the grid, x-fastest index. Every builder's key — the
// base, update and merge kernels of grid_kernels.h and the host form — is this function. The queries' cell stays a statement
// of its own, cell_grid.h:cell_of: the walk needs the three unclamped floats (a query may lie outside the grid), not an index.
MCL3DL_GEOM_HD inline uint32_t cell_index(const CellGridGeometry& g, float sx, float sy, float sz)
{
  const int cx = clamp_coord(static_cast<int>(grid_coord(sx, g.o[0], g.inv)), g.dim[0]);
  const int cy = clamp_coord(static_cast<int>(grid_coord(sy, g.o[1], g.inv)), g.dim[1]);
  const int cz = clamp_coord(static_cast<int>(grid_coord(sz, g.o[2], g.inv)), g.dim[2]);
  return static_cast<uint32_t>((static_cast<size_t>(cz) * g.dim[1] + cy) * g.dim[0] + cx);
}

// ... of a point that may be non-finite (a scan: a clip keeps NaN): cell 0 by decree instead of a float-to-int conversion of
// NaN or infinity; no float distance to such a point passes a `<`. Finite points: the same cell.
MCL3DL_GEOM_HD inline uint32_t cell_index_any(const CellGridGeometry& g, float sx, float sy, float sz)
{
  return (std::isfinite(sx) && std::isfinite(sy) && std::isfinite(sz)) ? cell_index(g, sx, sy, sz) : 0u;
}

inline bool lik_scan_provable(const int dim[3])
{
  return dim[0] <= LIK_SCAN_MAX_CELLS && dim[1] <= LIK_SCAN_MAX_CELLS && dim[2] <= LIK_SCAN_MAX_CELLS;
}

// ---- the DDA grid (DdaGrid): RaycastUsingDDA::updatePointCloud / toIndex / getArrayIndex / setExists ------------------------
// (raycast_using_dda.h:162-190, 205-210, 225-228) with the occupancy kept as one 64-bit word per 4 x 4 x 4 brick of voxels
struct DdaGeom
{
  float mn[3];
  double grid;
  int dim[3], bdim[3];       // voxels and bricks per axis
  unsigned long long total;  // voxels (0 when the grid is refused: 2^31 and more)
};

// map_size = (size_t)((max - min) / grid) + 1 per axis: float difference, double division. *total_d = the voxel count as a
// double: the reference keeps point_total in an int (raycast_using_dda.h:176), the caller refuses >= 2^31.
MCL3DL_GEOM_HD inline DdaGeom dda_grid_geometry(const float mn[3], const float mx[3], double grid, double* total_d)
{
  DdaGeom g;
  g.grid = grid;
  *total_d = 1;
  for (int a = 0; a < 3; ++a)
  {
    g.mn[a] = mn[a];
    g.dim[a] = static_cast<int>(static_cast<size_t>((mx[a] - mn[a]) / grid) + 1);
    g.bdim[a] = (g.dim[a] + 3) / 4;
    *total_d *= g.dim[a];
  }
  g.total = *total_d < 2147483647.0 ? static_cast<unsigned long long>(*total_d) : 0ull;
  return g;
}

// toIndex along one axis: float difference, double division, truncation toward zero. The builders' statement; the casting
// kernels keep the other one, beam_kernels.h:to_index, over the DdaGrid they are handed: that file's bytes are what the
// committed profiler counters are matched to, and it is not edited for a shared spelling.
MCL3DL_GEOM_HD inline int dda_voxel_coord(float p, float mn, double grid)
{
  return static_cast<int>(static_cast<double>(p - mn) / grid);
}

// getArrayIndex: x-fastest, in int arithmetic as the reference's
MCL3DL_GEOM_HD inline int dda_voxel_index(const DdaGeom& g, int c0, int c1, int c2)
{
  return c0 + c1 * g.dim[0] + c2 * (g.dim[0] * g.dim[1]);
}

// setExists: the occupancy word of the voxel's brick and the voxel's bit in it
MCL3DL_GEOM_HD inline void dda_brick_of(const DdaGeom& g, int c0, int c1, int c2, size_t& brick, unsigned long long& bit)
{
  brick = (static_cast<size_t>(c2 >> 2) * g.bdim[1] + (c1 >> 2)) * g.bdim[0] + (c0 >> 2);
  bit = 1ull << (((c2 & 3) << 4) | ((c1 & 3) << 2) | (c0 & 3));
}

// the same from a voxel index (dda_voxel_index inverted)
MCL3DL_GEOM_HD inline void dda_brick_bit(const DdaGeom& g, uint32_t v, size_t& brick, unsigned long long& bit)
{
  const int plane = g.dim[0] * g.dim[1];
  const int c2 = static_cast<int>(v) / plane, rem = static_cast<int>(v) - c2 * plane;
  const int c1 = rem / g.dim[0];
  dda_brick_of(g, rem - c1 * g.dim[0], c1, c2, brick, bit);
}

// ---- the host forms' stable counting sort: key[i] < n_keys -> start (n_keys + 1 run delimiters) and order (the element
// indices run by run, ascending inside a run — what the device's stable radix sort of (key, index) leaves) ------------------
inline void counting_sort(const std::vector<uint32_t>& key, size_t n_keys, std::vector<uint32_t>& start, std::vector<uint32_t>& order)
{
  start.assign(n_keys + 1, 0);
  for (const uint32_t k : key)
    ++start[k + 1];
  for (size_t k = 0; k < n_keys; ++k)
    start[k + 1] += start[k];
  std::vector<uint32_t> fill(start.begin(), start.end() - 1);
  order.resize(key.size());
  for (size_t i = 0; i < key.size(); ++i)
    order[fill[key[i]]++] = static_cast<uint32_t>(i);
}
}  // namespace mcl3dl
