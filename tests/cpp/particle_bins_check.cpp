// particle_bins_check.cpp — TEST INFRASTRUCTURE: the scalar functions of mcl_3dl_amd/csrc/particle_bins.h compiled for the host
// with g++ (the device compiles the same statements), run over states a test hands in; tests/test_particle_bins_cpu.py holds
// the output against tests/particle_bins_ref.py bit for bit.
//
//   in : int32 n, yaw_bins | float32 bin[3] | int32 min_b[3] | uint32 div[3] | float64 cs[2 yaw_bins] | float32 rows[n][7]
//   out: per row int32 {finite, i0, i1, i2, sector} and uint32 key, then float64 own_table[2 yaw_bins] (pb_yaw_sector_table)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "particle_bins.h"

using namespace mcl3dl;

template <typename T>
static bool read_n(FILE* f, T* p, size_t n)
{
  return n == 0 || fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv)
{
  if (argc != 3)
    return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in)
    return 3;
  int32_t head[2];
  float bin[3];
  int32_t min_b[3];
  uint32_t div[3];
  if (!read_n(in, head, 2) || !read_n(in, bin, 3) || !read_n(in, min_b, 3) || !read_n(in, div, 3))
    return 4;
  const int n = head[0], yaw_bins = head[1];
  if (n < 0 || !pb_yaw_bins_ok(yaw_bins))
    return 5;
  std::vector<double> cs(2 * static_cast<size_t>(yaw_bins));
  std::vector<float> rows(7 * static_cast<size_t>(n));
  if (!read_n(in, cs.data(), cs.size()) || !read_n(in, rows.data(), rows.size()))
    return 6;
  fclose(in);

  ParticleBinGrid g{};
  for (int a = 0; a < 3; ++a)
  {
    g.inv[a] = 1.0f / bin[a];
    g.min_b[a] = min_b[a];
    g.div[a] = div[a];
  }
  g.yaw_bins = yaw_bins;
  g.nonfinite_key = div[0] * div[1] * div[2] * static_cast<uint32_t>(yaw_bins);

  FILE* out = fopen(argv[2], "wb");
  if (!out)
    return 7;
  for (int i = 0; i < n; ++i)
  {
    const float* r = &rows[7 * static_cast<size_t>(i)];
    int32_t rec[5] = { 0, 0, 0, 0, 0 };
    uint32_t key = g.nonfinite_key;
    float t0, t1;
    pb_yaw_terms(r[3], r[4], r[5], r[6], &t0, &t1);
    rec[4] = pb_yaw_sector(t0, t1, cs.data(), yaw_bins);
    if (pb_finite3(r[0], r[1], r[2]))
    {
      rec[0] = 1;
      for (int a = 0; a < 3; ++a)
        rec[1 + a] = pb_axis_bin(r[a], g.inv[a], g.min_b[a]);
      key = pb_key(r, r + 3, g, cs.data());
    }
    fwrite(rec, sizeof(int32_t), 5, out);
    fwrite(&key, sizeof(uint32_t), 1, out);
  }
  std::vector<double> own(cs.size());
  if (!pb_yaw_sector_table(yaw_bins, own.data()))
    return 8;
  fwrite(own.data(), sizeof(double), own.size(), out);
  fclose(out);
  return 0;
}
