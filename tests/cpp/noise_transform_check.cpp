// noise_transform_check.cpp — mcl_3dl_amd/csrc/noise_transform.h on its own (the header the library compiles, with g++), and the
// standard library's side of the stream claim behind mcl3dl_hip_group_init_drawn_multivariate.
//
//   noise_transform_check transform <cov.bin> <out.bin>
//        cov.bin: 36 doubles, row-major. Prints "rc=<0|-3> clamped=<eigenvalues set to 0> msg=<the reason, when rejected>" and, with
//        rc = 0, writes 36 floats (T, row-major) and the 6 eigenvalues.
//   noise_transform_check particles <state> <n> <out.bin>
//        MultivariateNoiseGenerator::operator()'s draws (multivariate_noise_generator.h:84-88): per particle ONE
//        std::normal_distribution<float>(0, 1), called six times, on one std::default_random_engine that starts at <state>. Prints
//        "state=<engine state behind>" and writes the 6 n floats.
// g++ -O2 -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <sstream>
#include <vector>

#include "../../mcl_3dl_amd/csrc/noise_transform.h"

namespace
{
bool write_floats(const char* path, const std::vector<float>& v)
{
  FILE* f = fopen(path, "wb");
  if (!f)
    return false;
  const bool ok = fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc == 4 && !strcmp(argv[1], "transform"))
  {
    double cov[36];
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(cov, sizeof(double), 36, f) != 36)
      return 3;
    fclose(f);
    std::vector<float> out(42, 0.0f);
    char msg[192] = "";
    int clamped = 0;
    const int rc = mcl3dl::noise_transform6(cov, out.data(), out.data() + 36, &clamped, msg, sizeof(msg));
    printf("rc=%d clamped=%d msg=%s\n", rc, clamped, msg);
    if (rc == 0 && !write_floats(argv[3], out))
      return 3;
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "particles"))
  {
    const unsigned long state = strtoul(argv[2], nullptr, 10);
    const size_t n = strtoull(argv[3], nullptr, 10);
    if (state < 1ul || state > 2147483646ul)
      return 2;
    std::default_random_engine engine;
    {
      std::stringstream ss;
      ss << state;
      ss >> engine;
    }
    std::vector<float> values(6 * n);
    for (size_t i = 0; i < n; ++i)
    {
      std::normal_distribution<float> nd(0.0, 1.0);
      for (size_t j = 0; j < 6; ++j)
        values[6 * i + j] = nd(engine);
    }
    std::stringstream ss;
    ss << engine;
    unsigned long behind = 0;
    ss >> behind;
    printf("state=%lu\n", behind);
    return write_floats(argv[4], values) ? 0 : 3;
  }
  fprintf(stderr, "usage: %s transform <cov.bin> <out.bin> | particles <state> <n> <out.bin>\n", argv[0]);
  return 2;
}
