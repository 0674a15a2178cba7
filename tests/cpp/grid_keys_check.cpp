// grid_keys_check — what mcl_3dl_amd/csrc/index_geometry.h gives the builders of the two map grids, compiled for the host
// (tests/test_grid_keys_cpu.py holds the output against a numpy restatement of the reference's expressions): the cell grid's
// geometry and every point's cell, the DDA grid's geometry and every point's voxel, brick word and bit, the run starts and
// the order of the host forms' counting sort, and dda_brick_of / dda_brick_bit on every voxel of the grid.
//
//   grid_keys_check IN OUT
// IN : uint32 n, any (2: the cell grid's geometry alone), with_dda; float cell; double dda_grid; n x 3 float raw points; n x 3 float rescaled points
// OUT: uint64 words (floats and doubles as their bits) —
//   cell grid: o[3], inv, dim[3], cell[n], start[cells + 1], order[n]
//   with_dda : dim[3], bdim[3], total (double), voxel[n], brick[n], bit[n], start[total + 1], order[n], then per voxel of the
//              grid, x fastest: index, brick and bit by dda_brick_of, brick and bit by dda_brick_bit
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "index_geometry.h"

using namespace mcl3dl;

namespace
{
std::vector<uint64_t> out;

void put(uint64_t v)
{
  out.push_back(v);
}

void put_f(float f)
{
  uint32_t u;
  memcpy(&u, &f, sizeof(u));
  put(u);
}

void put_d(double d)
{
  uint64_t u;
  memcpy(&u, &d, sizeof(u));
  put(u);
}

// bounds of the finite points (what the device's min / max kernel hands the builders)
void bounds(const std::vector<float>& p, float mn[3], float mx[3])
{
  bool first = true;
  for (size_t i = 0; i < p.size() / 3; ++i)
  {
    if (!(std::isfinite(p[3 * i]) && std::isfinite(p[3 * i + 1]) && std::isfinite(p[3 * i + 2])))
      continue;
    for (int a = 0; a < 3; ++a)
    {
      if (first || p[3 * i + a] < mn[a])
        mn[a] = p[3 * i + a];
      if (first || p[3 * i + a] > mx[a])
        mx[a] = p[3 * i + a];
    }
    first = false;
  }
}

int write_out(const char* path)
{
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(out.data(), sizeof(uint64_t), out.size(), f) != out.size())
    return 2;
  fclose(f);
  return 0;
}

void put_sorted(const std::vector<uint32_t>& key, size_t n_keys)
{
  std::vector<uint32_t> start, order;
  counting_sort(key, n_keys, start, order);
  for (const uint32_t s : start)
    put(s);
  for (const uint32_t o : order)
    put(o);
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc != 3)
    return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f)
    return 2;
  uint32_t head[3];
  float cell;
  double grid;
  if (fread(head, sizeof(uint32_t), 3, f) != 3 || fread(&cell, sizeof(cell), 1, f) != 1 || fread(&grid, sizeof(grid), 1, f) != 1)
    return 2;
  const size_t n = head[0];
  const bool any = head[1] == 1, with_dda = head[2] != 0;
  std::vector<float> raw(3 * n), s(3 * n);
  if (fread(raw.data(), sizeof(float), 3 * n, f) != 3 * n || fread(s.data(), sizeof(float), 3 * n, f) != 3 * n)
    return 2;
  fclose(f);

  float mn[3] = { 0, 0, 0 }, mx[3] = { 0, 0, 0 };
  bounds(s, mn, mx);
  const CellGridGeometry cg = cell_grid_geometry(mn, mx, cell);
  for (int a = 0; a < 3; ++a)
    put_f(cg.o[a]);
  put_f(cg.inv);
  for (int a = 0; a < 3; ++a)
    put(static_cast<uint64_t>(cg.dim[a]));
  const double cells_d = static_cast<double>(cg.dim[0]) * cg.dim[1] * cg.dim[2];
  if (head[1] == 2)  // geometry only: a grid no builder would allocate
    return write_out(argv[2]);
  if (!(cells_d < 1.0e7))
    return 3;
  std::vector<uint32_t> key(n);
  for (size_t i = 0; i < n; ++i)
  {
    key[i] = any ? cell_index_any(cg, s[3 * i], s[3 * i + 1], s[3 * i + 2]) : cell_index(cg, s[3 * i], s[3 * i + 1], s[3 * i + 2]);
    put(key[i]);
  }
  put_sorted(key, static_cast<size_t>(cells_d));

  if (with_dda)
  {
    bounds(raw, mn, mx);
    double total_d = 0;
    const DdaGeom dg = dda_grid_geometry(mn, mx, grid, &total_d);
    for (int a = 0; a < 3; ++a)
      put(static_cast<uint64_t>(dg.dim[a]));
    for (int a = 0; a < 3; ++a)
      put(static_cast<uint64_t>(dg.bdim[a]));
    put_d(total_d);
    if (!(total_d < 1.0e7) || dg.total != static_cast<unsigned long long>(total_d))
      return 3;
    std::vector<uint64_t> brick(n), bit(n);
    for (size_t i = 0; i < n; ++i)
    {
      const int c0 = dda_voxel_coord(raw[3 * i], dg.mn[0], dg.grid), c1 = dda_voxel_coord(raw[3 * i + 1], dg.mn[1], dg.grid),
                c2 = dda_voxel_coord(raw[3 * i + 2], dg.mn[2], dg.grid);
      const int v = dda_voxel_index(dg, c0, c1, c2);
      if (v < 0 || static_cast<unsigned long long>(v) >= dg.total)
        return 4;
      key[i] = static_cast<uint32_t>(v);
      size_t b;
      unsigned long long m;
      dda_brick_of(dg, c0, c1, c2, b, m);
      brick[i] = b;
      bit[i] = m;
    }
    for (size_t i = 0; i < n; ++i)
      put(key[i]);
    for (size_t i = 0; i < n; ++i)
      put(brick[i]);
    for (size_t i = 0; i < n; ++i)
      put(bit[i]);
    put_sorted(key, static_cast<size_t>(dg.total));
    for (int c2 = 0; c2 < dg.dim[2]; ++c2)
      for (int c1 = 0; c1 < dg.dim[1]; ++c1)
        for (int c0 = 0; c0 < dg.dim[0]; ++c0)
        {
          const int v = dda_voxel_index(dg, c0, c1, c2);
          size_t b0, b1;
          unsigned long long m0, m1;
          dda_brick_of(dg, c0, c1, c2, b0, m0);
          dda_brick_bit(dg, static_cast<uint32_t>(v), b1, m1);
          put(static_cast<uint64_t>(v));
          put(b0);
          put(m0);
          put(b1);
          put(m1);
        }
  }
  return write_out(argv[2]);
}
