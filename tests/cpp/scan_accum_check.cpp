// scan_accum_check.cpp — accum_affine_apply of mcl_3dl_amd/csrc/scan_accum.h compiled for the host (the expression the push and
// the to-base kernels run), so that tests/test_scan_accum_cpu.py can hold tests/scan_accum_ref.py against it bit for bit.
//
//   scan_accum_check IN OUT
//     IN : uint32 n_mats, uint32 n_pts, n_mats x 12 floats (rows of the 3x4 [R | t]), n_pts x 3 floats
//     OUT: n_mats x n_pts x 3 floats
//   build: g++ -O2 -std=c++17 -ffp-contract=off -I mcl_3dl_amd/csrc
#include <cstdint>
#include <cstdio>
#include <vector>

#include "scan_accum.h"

int main(int argc, char** argv)
{
  if (argc != 3)
  {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in)
    return 2;
  uint32_t head[2] = { 0, 0 };
  if (fread(head, sizeof(uint32_t), 2, in) != 2)
    return 3;
  std::vector<float> mats(12 * static_cast<size_t>(head[0])), pts(3 * static_cast<size_t>(head[1]));
  if (fread(mats.data(), sizeof(float), mats.size(), in) != mats.size() || fread(pts.data(), sizeof(float), pts.size(), in) != pts.size())
    return 3;
  fclose(in);
  FILE* out = fopen(argv[2], "wb");
  if (!out)
    return 2;
  std::vector<float> res(pts.size());
  for (uint32_t k = 0; k < head[0]; ++k)
  {
    for (uint32_t i = 0; i < head[1]; ++i)
    {
      const mcl3dl::AccumPoint p = mcl3dl::accum_affine_apply(&mats[12 * static_cast<size_t>(k)], pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
      res[3 * i] = p.x;
      res[3 * i + 1] = p.y;
      res[3 * i + 2] = p.z;
    }
    if (fwrite(res.data(), sizeof(float), res.size(), out) != res.size())
      return 4;
  }
  return fclose(out) == 0 ? 0 : 4;
}
