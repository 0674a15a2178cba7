// scan_keys_check.cpp — the scan ordering's keys of mcl_3dl_amd/csrc/cloud_keys.h compiled for the host (the functions the sort
// kernels and api_core.inl:order_scan both call), so that tests/test_cloud_ref_cpu.py can hold tests/cloud_ref.py against them
// bit for bit.
//
//   scan_keys_check IN OUT
//     IN : uint32 n_lik, uint32 n_beam, uint32 n_o, n_lik x 3 floats, n_beam x 3 floats, n_beam uint32 origin ids (< n_o),
//          n_o x 3 floats
//     OUT: uint32 dropped bits, n_lik uint32 Morton keys (corners: min / max over the finite points, +-FLT_MAX when there is
//          none), n_beam uint32 range keys
//   build: g++ -O2 -std=c++17 -ffp-contract=off -I mcl_3dl_amd/csrc
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cloud_keys.h"

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
  uint32_t head[3] = { 0, 0, 0 };
  if (fread(head, sizeof(uint32_t), 3, in) != 3)
    return 3;
  const size_t n_lik = head[0], n_beam = head[1], n_o = head[2];
  std::vector<float> lik(3 * n_lik), beam(3 * n_beam), origins(3 * n_o);
  std::vector<uint32_t> og(n_beam);
  if (fread(lik.data(), sizeof(float), lik.size(), in) != lik.size() || fread(beam.data(), sizeof(float), beam.size(), in) != beam.size() ||
      fread(og.data(), sizeof(uint32_t), og.size(), in) != og.size() ||
      fread(origins.data(), sizeof(float), origins.size(), in) != origins.size())
    return 3;
  fclose(in);
  float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
  for (size_t i = 0; i < n_lik; ++i)
  {
    const float* q = &lik[3 * i];
    if (!(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2])))
      continue;
    for (int a = 0; a < 3; ++a)
    {
      mn[a] = q[a] < mn[a] ? q[a] : mn[a];
      mx[a] = q[a] > mx[a] ? q[a] : mx[a];
    }
  }
  std::vector<uint32_t> res(1 + n_lik + n_beam);
  const uint32_t drop = mcl3dl::morton_drop_bits(mn, mx);
  res[0] = drop;
  for (size_t i = 0; i < n_lik; ++i)
    res[1 + i] = mcl3dl::morton_key(lik[3 * i], lik[3 * i + 1], lik[3 * i + 2], mn) >> drop;
  for (size_t i = 0; i < n_beam; ++i)
  {
    if (og[i] >= n_o)
      return 3;
    const float* o = &origins[3 * og[i]];
    res[1 + n_lik + i] = mcl3dl::range_key(beam[3 * i], beam[3 * i + 1], beam[3 * i + 2], o[0], o[1], o[2]);
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out)
    return 2;
  if (fwrite(res.data(), sizeof(uint32_t), res.size(), out) != res.size())
    return 4;
  return fclose(out) == 0 ? 0 : 4;
}
