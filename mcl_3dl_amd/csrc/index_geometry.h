// index_geometry.h — the pure arithmetic of the two likelihood indices' geometry, free of HIP so that a plain C++ program can
// include it (tests/cpp/voxel_slack_check.cpp sweeps it): the candidate-voxel grid (map_compiler.h, host_map_compilers.h) —
// edges, their float reciprocals, the slack `grow` of V+, reach, origin, voxel and brick counts — the map's cell grid
// (build_lik_grid_host and its device twin) — origin, edge, dimensions — and the one float expression by which every kernel
// and every host builder assigns a coordinate its voxel or cell.
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
#include <cstdint>

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

inline CellGridGeometry cell_grid_geometry(const float mn[3], const float mx[3], float cell)
{
  CellGridGeometry g;
  g.inv = 1.0f / cell;
  for (int a = 0; a < 3; ++a)
  {
    g.o[a] = mn[a] - 2.0f * cell;
    g.dim[a] = static_cast<int>(grid_coord(mx[a], g.o[a], g.inv)) + 3;
  }
  return g;
}

inline bool lik_scan_provable(const int dim[3])
{
  return dim[0] <= LIK_SCAN_MAX_CELLS && dim[1] <= LIK_SCAN_MAX_CELLS && dim[2] <= LIK_SCAN_MAX_CELLS;
}
}  // namespace mcl3dl
