// particle_bins.h — the occupied-bin statistic of a particle set, stated ONCE as scalar functions that compile
// for the device (particle_bins_kernels.h) and for the host (api_particle_bins.inl; tests/cpp/particle_bins_check.cpp compiles
// them with g++ and holds them against tests/particle_bins_ref.py). Nothing of this is the reference's: it has no pose grid.
//
//   position bin   pcl::VoxelGrid's own expression (cloud_keys.h:voxel_leaf_key) with the bin edge in place of the leaf:
//                  inv = 1.0f / bin, i = int(floorf(p * inv) - float(min_b)), min_b = int(floorf(min_p * inv))
//   yaw sector     t0 / t1 as Quat::getRPY forms them (float products, the tails in double, rounded to float), and NO atan2:
//                  the first j with c_j t1 - s_j t0 >= 0 and c_{j+1} t1 - s_{j+1} t0 < 0 over the table (c_j, s_j) = (cos, sin)
//                  (2 pi j / yaw_bins) — products and difference in double, unfused; 0 when no j qualifies
//   key            ((i2 div1 + i1) div0 + i0) yaw_bins + sector, below 2^32 - 1
//   KLD bound      Fox's bound as AMCL's pf_resample_limit writes it
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PARTICLE_BINS_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define PARTICLE_BINS_HD
#endif

namespace mcl3dl
{
constexpr int PB_MAX_YAW_BINS = 64;
constexpr int PB_MAX_TOP_K = 16;
constexpr unsigned long long PB_MAX_KEYS = 0xfffffffeull;  // cells x yaw_bins; the key above them all is the non-finite one

PARTICLE_BINS_HD inline bool pb_yaw_bins_ok(int yaw_bins)
{
  return yaw_bins == 1 || (yaw_bins >= 3 && yaw_bins <= PB_MAX_YAW_BINS);
}

PARTICLE_BINS_HD inline bool pb_finite3(float x, float y, float z)
{
  // (x - x is 0 for a finite x and NaN otherwise: the same test on both sides of the boundary)
  return (x - x) == 0.f && (y - y) == 0.f && (z - z) == 0.f;
}

// floor(p * inv) as the float VoxelGrid converts to int: min_b / max_b of the extent
PARTICLE_BINS_HD inline float pb_floor_scaled(float p, float inv)
{
  return floorf(p * inv);
}

// bin index along one axis, relative to min_b
PARTICLE_BINS_HD inline int pb_axis_bin(float p, float inv, int min_b)
{
  return static_cast<int>(floorf(p * inv) - static_cast<float>(min_b));
}

// Quat::getRPY's t0 and t1 (include/mcl_3dl/quat.h:193-195) of the quaternion {x, y, z, w}
PARTICLE_BINS_HD inline void pb_yaw_terms(float x, float y, float z, float w, float* t0, float* t1)
{
  const float ysq = y * y;
  const float zz = z * z;
  const float s0 = ysq + zz;
  const float xy = x * y;
  const float wz = w * z;
  const float s1 = xy + wz;
  *t0 = static_cast<float>(-2.0 * static_cast<double>(s0) + 1.0);
  *t1 = static_cast<float>(+2.0 * static_cast<double>(s1));
}

// the sector of a heading (t0, t1) over the table cs = {c_0, s_0, c_1, s_1, ...} of yaw_bins entries
PARTICLE_BINS_HD inline int pb_yaw_sector(float t0, float t1, const double* cs, int yaw_bins)
{
  if (yaw_bins <= 1)
    return 0;
  const double a = static_cast<double>(t1), b = static_cast<double>(t0);
  const double pc0 = cs[0] * a, ps0 = cs[1] * b;
  double side = pc0 - ps0;
  for (int j = 0; j < yaw_bins; ++j)
  {
    const int jn = j + 1 == yaw_bins ? 0 : j + 1;
    const double pc = cs[2 * jn] * a, ps = cs[2 * jn + 1] * b;
    const double next = pc - ps;
    if (side >= 0.0 && next < 0.0)
      return j;
    side = next;
  }
  return 0;
}

struct ParticleBinGrid
{
  float inv[3];    // 1.0f / bin
  int min_b[3];    // int(floorf(min_p * inv))
  uint32_t div[3];  // max_b - min_b + 1
  int yaw_bins;
  uint32_t nonfinite_key;  // div0 div1 div2 yaw_bins: above every bin's key
};

// the key of a particle with a finite position: pos {x, y, z}, rot {x, y, z, w}
PARTICLE_BINS_HD inline uint32_t pb_key(const float* pos, const float* rot, const ParticleBinGrid& g, const double* cs)
{
  const uint32_t i0 = static_cast<uint32_t>(pb_axis_bin(pos[0], g.inv[0], g.min_b[0]));
  const uint32_t i1 = static_cast<uint32_t>(pb_axis_bin(pos[1], g.inv[1], g.min_b[1]));
  const uint32_t i2 = static_cast<uint32_t>(pb_axis_bin(pos[2], g.inv[2], g.min_b[2]));
  float t0, t1;
  pb_yaw_terms(rot[0], rot[1], rot[2], rot[3], &t0, &t1);
  const uint32_t sector = static_cast<uint32_t>(pb_yaw_sector(t0, t1, cs, g.yaw_bins));
  return ((i2 * g.div[1] + i1) * g.div[0] + i0) * static_cast<uint32_t>(g.yaw_bins) + sector;
}

// key -> {absolute ix, iy, iz, sector}
inline void pb_key_parts(uint32_t key, const ParticleBinGrid& g, int32_t* bin4)
{
  const uint32_t yb = static_cast<uint32_t>(g.yaw_bins);
  const uint32_t cell = key / yb;
  bin4[3] = static_cast<int32_t>(key % yb);
  bin4[0] = static_cast<int32_t>(cell % g.div[0]) + g.min_b[0];
  bin4[1] = static_cast<int32_t>((cell / g.div[0]) % g.div[1]) + g.min_b[1];
  bin4[2] = static_cast<int32_t>(cell / g.div[0] / g.div[1]) + g.min_b[2];
}

// ---- host only ------------------------------------------------------------------------------------------------------------
// (c_j, s_j) = (cos, sin)(2 pi j / yaw_bins); the multiples of a quarter turn are exact, so that an axis-aligned heading sits ON
// its sector's boundary and not an ulp of pi beside it. false: yaw_bins is neither 1 nor 3 ... 64.
inline bool pb_yaw_sector_table(int yaw_bins, double* out_cs)
{
  if (!pb_yaw_bins_ok(yaw_bins) || !out_cs)
    return false;
  static const double quarter[4][2] = { { 1.0, 0.0 }, { 0.0, 1.0 }, { -1.0, 0.0 }, { 0.0, -1.0 } };
  for (int j = 0; j < yaw_bins; ++j)
  {
    if ((4 * j) % yaw_bins == 0)
    {
      out_cs[2 * j] = quarter[4 * j / yaw_bins][0];
      out_cs[2 * j + 1] = quarter[4 * j / yaw_bins][1];
      continue;
    }
    const double angle = 2.0 * M_PI * static_cast<double>(j) / static_cast<double>(yaw_bins);
    out_cs[2 * j] = cos(angle);
    out_cs[2 * j + 1] = sin(angle);
  }
  return true;
}

// Fox's KLD bound (Fox 2003) as AMCL's pf_resample_limit writes it, term by term in double: the particles that keep the
// K-L distance to the true posterior below epsilon with the probability whose upper normal quantile is z, when k bins are
// occupied. k <= 1 -> 1; a bound below 1 (a z far in the lower tail) is 1 as well. false: epsilon outside (0, 1], a non-finite
// z, or a bound that does not fit 2^62.
inline bool pb_kld_bound(size_t k, double epsilon, double z, size_t* out_n)
{
  if (!(epsilon > 0.0 && epsilon <= 1.0) || !(z - z == 0.0) || !out_n)
    return false;
  if (k <= 1)
  {
    *out_n = 1;
    return true;
  }
  const double km1 = static_cast<double>(k - 1);
  const double b = 2.0 / (9.0 * km1);
  const double x = 1.0 - b + sqrt(b) * z;
  const double n = ceil(km1 / (2.0 * epsilon) * x * x * x);
  if (!(n < 4611686018427387904.0))  // 2^62 (a NaN fails too)
    return false;
  *out_n = n < 1.0 ? 1 : static_cast<size_t>(n);
  return true;
}
}  // namespace mcl3dl
