// voxel_slack_check.cpp — stand-alone sweep of mcl_3dl_amd/csrc/index_geometry.h (no HIP, no GPU): does every float
// coordinate lie inside the grown box V+ of the voxel the float expression floor((q - o) * inv_e) gives it, on every grid the
// header lays out — and does the 27-cell scan's premise hold on the cell grid: two coordinates closer than the radius along
// an axis get cells that differ by at most one.
//
// Geometries: match_dist_min 0.05, 0.1, 0.2, 0.3, 0.5; voxel ratio 0.125, 0.5, 2; cubes and voxels stretched x 5 along z;
// bounds starting at -0.35, -17.123, 999.65; 20 m, 500 m, 1.1 km, 2.2 km, 5 km long along x or along z (3 m and 2 m across).
// Faces: all up to index 4 096, every face within 32 of a power of two of the index, of the coordinate, and of the distance
// from the origin, and 20 000 seeded random faces beyond. At each face: the float nearest to it and the 8 floats on either side.
// A geometry the header refuses counts as refused (the engine builds no index there).
//
//   voxel_slack_check                the header's slack and limits: must pass
//   voxel_slack_check --fixed-slack  the same grids with the slack fixed at 1e-3 of the shortest edge and no limit on the cell
//                                    grid (what the engine did before the slack was derived): must FAIL — prints the first
//                                    failing face per radius
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "index_geometry.h"

using namespace mcl3dl;

namespace
{
constexpr int SIDE = 8;  // floats on either side of the float nearest to a face

void add_window(std::set<long long>& faces, double centre, long long n)
{
  if (!(centre > -64.0 && centre < static_cast<double>(n) + 64.0))
    return;
  const long long c = static_cast<long long>(std::floor(centre));
  for (long long k = c - 32; k <= c + 33; ++k)
    if (k >= 1 && k <= n - 1)
      faces.insert(k);
}

// the faces of one axis: origin o, edge e (fp64 of a float), n voxels or cells
std::vector<long long> face_set(double o, double e, long long n, uint32_t seed)
{
  std::set<long long> faces;
  for (long long k = 1; k <= std::min<long long>(4096, n - 1); ++k)
    faces.insert(k);
  for (int j = 12; j < 31; ++j)
    add_window(faces, std::ldexp(1.0, j), n);  // index
  for (int j = -4; j < 20; ++j)
  {
    const double x = std::ldexp(1.0, j);
    add_window(faces, (x - o) / e, n);   // coordinate
    add_window(faces, (-x - o) / e, n);
    add_window(faces, x / e, n);         // distance from the origin
  }
  if (n - 1 > 4096)
  {
    std::mt19937_64 rng(seed);
    std::uniform_int_distribution<long long> pick(4097, n - 1);
    for (int i = 0; i < 20000; ++i)
      faces.insert(pick(rng));
  }
  return std::vector<long long>(faces.begin(), faces.end());
}

struct Failure
{
  bool any = false;
  double r = 0, ratio = 0, stretch = 0, origin = 0, extent = 0, outside = 0;
  int axis = 0;
  long long face = 0;
  float q = 0;
  int voxel = 0;
};

// one axis of a candidate grid; returns the number of floats outside the V+ of their voxel
long long sweep_axis(float o_f, double e, float inv_e, int nv, double grow, uint32_t seed, Failure* first, long long* tested)
{
  const double o = static_cast<double>(o_f);
  long long bad = 0;
  for (const long long k : face_set(o, e, nv, seed))
  {
    float q = static_cast<float>(o + static_cast<double>(k) * e);
    for (int s = 0; s < SIDE; ++s)
      q = std::nextafterf(q, -INFINITY);
    for (int s = 0; s < 2 * SIDE + 1; ++s, q = std::nextafterf(q, INFINITY))
    {
      const float t = grid_coord(q, o_f, inv_e);
      if (!(t >= 0.0f && t < static_cast<float>(nv)))
        continue;  // outside the grid: the kernel finds no voxel
      const int v = static_cast<int>(t);
      const double lo = o + v * e - grow, hi = o + (v + 1) * e + grow;  // box_dist2's faces (map_compiler.h)
      const double x = static_cast<double>(q);
      ++*tested;
      if (x >= lo && x <= hi)
        continue;
      ++bad;
      if (!first->any)
      {
        first->any = true;
        first->face = k;
        first->q = q;
        first->voxel = v;
        first->outside = x < lo ? lo - x : x - hi;
      }
    }
  }
  return bad;
}

// the 27-cell scan's premise on one axis of a cell grid: |a - b| < r (fp64)  =>  |cell(a) - cell(b)| <= 1
long long sweep_cells(float o_f, float inv, int dim, double r, uint32_t seed, Failure* first, long long* tested)
{
  const double o = static_cast<double>(o_f), cell = 1.0 / static_cast<double>(inv);
  long long bad = 0;
  for (const long long k : face_set(o, cell, dim, seed))
  {
    float a = static_cast<float>(o + static_cast<double>(k) * cell);
    for (int s = 0; s < SIDE; ++s)
      a = std::nextafterf(a, -INFINITY);
    for (int s = 0; s < 2 * SIDE + 1; ++s, a = std::nextafterf(a, INFINITY))
    {
      const float ca = grid_coord(a, o_f, inv);
      // the farthest floats still closer than r, above and below
      for (int dir = -1; dir <= 1; dir += 2)
      {
        float b = static_cast<float>(static_cast<double>(a) + dir * r);
        while (!(std::fabs(static_cast<double>(b) - static_cast<double>(a)) < r))
          b = std::nextafterf(b, dir > 0 ? -INFINITY : INFINITY);
        for (int s2 = 0; s2 < 3; ++s2, b = std::nextafterf(b, dir > 0 ? -INFINITY : INFINITY))
        {
          const float cb = grid_coord(b, o_f, inv);
          ++*tested;
          if (std::fabs(cb - ca) <= 1.0f)
            continue;
          ++bad;
          if (!first->any)
          {
            first->any = true;
            first->face = k;
            first->q = a;
            first->voxel = static_cast<int>(ca);
            first->outside = static_cast<double>(b);
          }
        }
      }
    }
  }
  return bad;
}
}  // namespace

int main(int argc, char** argv)
{
  const bool fixed_slack = argc > 1 && strcmp(argv[1], "--fixed-slack") == 0;
  const float radii[] = { 0.05f, 0.1f, 0.2f, 0.3f, 0.5f };
  const double ratios[] = { 0.125, 0.5, 2.0 };
  const double stretches[] = { 1.0, 5.0 };
  const double origins[] = { -0.35, -17.123, 999.65 };
  const double extents[] = { 20.0, 500.0, 1100.0, 2200.0, 5000.0 };
  long long geometries = 0, refused = 0, failing = 0, tested = 0, cell_grids = 0, cell_refused = 0, cell_failing = 0;
  bool ok = true;
  for (const float r_f : radii)
  {
    const double r = static_cast<double>(r_f);  // the engine keeps match_dist_min as a float
    Failure first_r, first_cells_r;
    std::set<double> failing_extents;
    for (const double extent : extents)
      for (const double origin : origins)
        for (int long_axis = 0; long_axis <= 2; long_axis += 2)
        {
          float mn[3], mx[3];
          const double across[3] = { 3.0, 2.0, 2.5 };
          for (int a = 0; a < 3; ++a)
          {
            mn[a] = static_cast<float>(origin);
            mx[a] = static_cast<float>(origin + (a == long_axis ? extent : across[a]));
          }
          const uint32_t seed = static_cast<uint32_t>(geometries * 7919 + 17);
          for (const double ratio : ratios)
            for (const double sz : stretches)
            {
              const double stretch[3] = { 1.0, 1.0, sz };
              CompileParams cp{};
              long long n_table = 0;
              double detail = 0;
              ++geometries;
              const CandGeomStatus st = cand_grid_geometry(r, ratio, stretch, 0.5, mn, mx, &cp, &n_table, &detail);
              if (st == CAND_GEOM_SLACK || st == CAND_GEOM_TABLE)
              {
                ++refused;
                continue;
              }
              if (st != CAND_GEOM_OK)
              {
                printf("FAIL: r %g ratio %g stretch %g origin %g extent %g: status %d\n", r, ratio, sz, origin, extent, st);
                ok = false;
                continue;
              }
              const double e_min = std::fmin(cp.ex, std::fmin(cp.ey, cp.ez));
              if (fixed_slack)
                cp.grow = CAND_GROW_MIN_FRACTION * e_min;
              const float o[3] = { cp.ox, cp.oy, cp.oz }, inv[3] = { cp.inv_ex, cp.inv_ey, cp.inv_ez };
              const double ed[3] = { cp.ex, cp.ey, cp.ez };
              const int nv[3] = { cp.nvx, cp.nvy, cp.nvz }, reach[3] = { cp.rx, cp.ry, cp.rz };
              if (!fixed_slack)
              {
                // what the slack was derived from covers the grid that came out, the reach covers the slack, the slack is
                // within its stated fractions of the shortest edge
                double max_abs = 0.0;
                for (int a = 0; a < 3; ++a)
                  max_abs = std::fmax(max_abs, std::fmax(std::fabs(static_cast<double>(o[a])), std::fabs(o[a] + nv[a] * ed[a])));
                for (int a = 0; a < 3; ++a)
                {
                  const bool covered = cp.grow >= cand_derived_grow(nv[a] * ed[a], 0.0) &&
                                       cp.grow >= CAND_GROW_PER_LENGTH * nv[a] * ed[a] + max_abs / 4503599627370496.0;
                  const bool reaches = reach[a] >= std::ceil((r * (1.0 + 1e-5) + 2.0 * cp.grow) / ed[a]);
                  const bool bounded = cp.grow >= CAND_GROW_MIN_FRACTION * e_min && cp.grow <= CAND_GROW_MAX_FRACTION * e_min;
                  const bool inside = static_cast<double>(mn[a]) - o[a] >= (reach[a] + 1) * ed[a] * (1.0 - 1e-6) &&
                                      o[a] + nv[a] * ed[a] - static_cast<double>(mx[a]) >= (reach[a] + 1) * ed[a] * (1.0 - 1e-6);
                  if (!(covered && reaches && bounded && inside))
                  {
                    printf("FAIL: r %g ratio %g stretch %g origin %g extent %g axis %d: grow %.6g voxels %d reach %d (covered %d "
                           "reaches %d bounded %d inside %d)\n", r, ratio, sz, origin, extent, a, cp.grow, nv[a], reach[a], covered,
                           reaches, bounded, inside);
                    ok = false;
                  }
                }
                // a grid of today's sizes keeps the slack it always had
                if (extent <= 20.0 && cp.grow != 1e-3 * e_min)
                {
                  printf("FAIL: r %g ratio %g stretch %g extent %g: grow %.17g is not 1e-3 of the shortest edge\n", r, ratio, sz, extent,
                         cp.grow);
                  ok = false;
                }
              }
              Failure first;
              long long bad = 0;
              for (int a = 0; a < 3; ++a)
              {
                Failure f;
                bad += sweep_axis(o[a], ed[a], inv[a], nv[a], cp.grow, seed + a, &f, &tested);
                if (f.any && !first.any)
                {
                  first = f;
                  first.axis = a;
                }
              }
              if (bad)
              {
                ++failing;
                failing_extents.insert(extent);
                first.r = r;
                first.ratio = ratio;
                first.stretch = sz;
                first.origin = origin;
                first.extent = extent;
                if (!first_r.any || first.face < first_r.face)
                  first_r = first;
                if (!fixed_slack)
                  printf("FAIL: r %g ratio %g stretch %g origin %g extent %g axis %d: %lld floats outside V+, first at face %lld: "
                         "q = %.9g -> voxel %d, %.3g outside (grow %.3g)\n", r, ratio, sz, origin, extent, first.axis, bad, first.face,
                         first.q, first.voxel, first.outside, cp.grow);
              }
            }
          // the cell grid of the same bounds
          const float cell = r_f * 1.01f;
          const CellGridGeometry g = cell_grid_geometry(mn, mx, cell);
          ++cell_grids;
          if (!fixed_slack && !lik_scan_provable(g.dim))
          {
            ++cell_refused;
            continue;
          }
          Failure fc;
          long long bad_cells = 0;
          for (int a = 0; a < 3; ++a)
            bad_cells += sweep_cells(g.o[a], g.inv, g.dim[a], r, seed + 3 + a, &fc, &tested);
          if (bad_cells)
          {
            ++cell_failing;
            fc.r = r;
            fc.origin = origin;
            fc.extent = extent;
            if (!first_cells_r.any || fc.face < first_cells_r.face)
              first_cells_r = fc;
            if (!fixed_slack)
              printf("FAIL: cell grid r %g origin %g extent %g: %lld pairs closer than r more than one cell apart, first at cell "
                     "%lld: %.9g and %.9g\n", r, origin, extent, bad_cells, fc.face, fc.q, static_cast<float>(fc.outside));
          }
        }
    if (first_r.any)
      printf("r %g: first float outside the V+ of its voxel at face %lld (ratio %g, stretch %g, bounds from %g, %g m long, axis %d): "
             "q = %.9g -> voxel %d, %.3g outside\n", r, first_r.face, first_r.ratio, first_r.stretch, first_r.origin, first_r.extent,
             first_r.axis, first_r.q, first_r.voxel, first_r.outside);
    else
      printf("r %g: every float inside the V+ of its voxel\n", r);
    if (!failing_extents.empty())
    {
      printf("r %g: grids with floats outside V+ are", r);
      for (const double x : failing_extents)
        printf(" %g", x);
      printf(" m long\n");
    }
    if (first_cells_r.any)
      printf("r %g: cell grid: first pair closer than r and more than one cell apart at cell %lld (bounds from %g, %g m long): %.9g "
             "and %.9g\n", r, first_cells_r.face, first_cells_r.origin, first_cells_r.extent, first_cells_r.q,
             static_cast<float>(first_cells_r.outside));
    else
      printf("r %g: cell grid: every pair closer than r within one cell\n", r);
  }
  printf("candidate grids: %lld, refused %lld, failing %lld; cell grids: %lld, refused %lld, failing %lld; %lld floats tested\n",
         geometries, refused, failing, cell_grids, cell_refused, cell_failing, tested);
  if (failing || cell_failing)
    ok = false;
  // the sweep is not vacuous: most grids are laid out, those of today's sizes all of them
  if (!fixed_slack && (refused * 4 > geometries || cell_refused * 4 > cell_grids))
  {
    printf("FAIL: too many geometries refused\n");
    ok = false;
  }
  printf(ok ? "all checks passed\n" : "CHECKS FAILED\n");
  return ok ? 0 : 1;
}
