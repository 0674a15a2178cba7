// cloud_keys.h — the sort keys of the cloud path: pcl::VoxelGrid's leaf index (device only), and the Morton key and the range
// key of the scan ordering. The two scan keys are stated ONCE, as scalar functions that compile for the device (the fused
// key-and-sort kernels of sort_kernels.h, scan_stage_kernel) and for the host (api_core.inl:order_scan);
// tests/cpp/scan_keys_check.cpp compiles them with g++ and holds them against tests/cloud_ref.py.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLOUD_KEYS_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define CLOUD_KEYS_HD
#endif

namespace mcl3dl
{
#if defined(__HIPCC__)
__device__ inline bool finite3(const float4 p)
{
  return isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
}

// ---- pcl::VoxelGrid ---------------------------------------------------------------------------------------------------
struct VoxelGridParams
{
  float inv_leaf[3];       // Eigen::Array4f::Ones() / leaf_size
  int min_b[3];            // floor(min_p * inv_leaf)
  int mul[3];              // divb_mul_: 1, div_b[0], div_b[0] * div_b[1]
  uint32_t nonfinite_key;  // key of a point with a non-finite coordinate: above every leaf index (sorted last, dropped)
};

// leaf index of a point — the expression of voxel_grid.hpp: ijk = int(floor(p * inv_leaf) - float(min_b)),
// idx = ijk . divb_mul
__device__ inline uint32_t voxel_leaf_key(const float4 p, const VoxelGridParams& vp)
{
  if (!finite3(p))
    return vp.nonfinite_key;
  const int i0 = static_cast<int>(floorf(p.x * vp.inv_leaf[0]) - static_cast<float>(vp.min_b[0]));
  const int i1 = static_cast<int>(floorf(p.y * vp.inv_leaf[1]) - static_cast<float>(vp.min_b[1]));
  const int i2 = static_cast<int>(floorf(p.z * vp.inv_leaf[2]) - static_cast<float>(vp.min_b[2]));
  return static_cast<uint32_t>(i0 * vp.mul[0] + i1 * vp.mul[1] + i2 * vp.mul[2]);
}

#endif  // __HIPCC__

// ---- scan ordering ----------------------------------------------------------------------------------------------------
CLOUD_KEYS_HD inline uint32_t spread10(uint32_t v)
{
  // 10 bits -> every third bit
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// 0.25 m cell of a coordinate `d` metres above the cloud's minimum corner, clamped to 10 bits (a NaN lands in cell 0)
CLOUD_KEYS_HD inline uint32_t morton_cell(float d)
{
  const float f = d * 4.0f;
  return (f >= 0.f) ? (f < 1023.f ? static_cast<uint32_t>(f) : 1023u) : 0u;
}

// Morton key of a likelihood scan point: 0.25 m cells from the cloud's minimum corner, 10 bits per axis, of which the
// MCL3DL_MORTON_BITS most significant bits the cloud's extent can set are kept (the extent: the corners of the cloud's finite
// points). The order only decides which evaluations share a work-group. 16 bits = two radix passes (four launches
// behind the key-making one) instead of the three a 22-bit key costs or the four of the full 30-bit key: cells of 1 m for a
// cloud up to 32 m across (2 m up to 64 m, ...). Measured at C2 (round-4 sessions s2 / s4, drivers in the git history: profiles/r04b_time8d_C2_m16.json,
// r04d_time8d_C2_m16.json against the 22-bit build in the same session): likelihood kernel +0.5 % (0.2305 -> 0.2326 ms
// device-resident step), host-buffer update -2.5 % (0.2918 -> 0.2843 ms: two launches fewer in front of the likelihood
// kernel, where every dependent launch costs 3-4 us); with 8 bits (one pass) the kernel loses 13 %. Round 3 measured 16 / 22 /
// 30 bits at C2 / C5 / the map of centroids within 1 % of each other (round-3 session s22, git history).
#ifndef MCL3DL_MORTON_BITS
#define MCL3DL_MORTON_BITS 16   // (A/B builds: 22 / 8 — csrc/Makefile:variants-morton)
#endif
// the low bits dropped from the 30-bit key of a cloud between the corners mn and mx
CLOUD_KEYS_HD inline uint32_t morton_drop_bits(const float mn[3], const float mx[3])
{
  uint32_t cells = 0;
  for (int a = 0; a < 3; ++a)
  {
    const uint32_t c = morton_cell(mx[a] - mn[a]);
    cells = c > cells ? c : cells;
  }
  const uint32_t bits = cells ? 32u - static_cast<uint32_t>(__builtin_clz(cells)) : 0u;
  return 3u * bits > MCL3DL_MORTON_BITS ? 3u * bits - MCL3DL_MORTON_BITS : 0u;
}

// the whole 30-bit key of a point: the sort key is morton_key(...) >> morton_drop_bits(...)
CLOUD_KEYS_HD inline uint32_t morton_key(float x, float y, float z, const float mn[3])
{
  return spread10(morton_cell(x - mn[0])) | (spread10(morton_cell(y - mn[1])) << 1) | (spread10(morton_cell(z - mn[2])) << 2);
}

// squared range of a beam point from its scan origin, as float bits: non-negative floats order like unsigned ints, the sum of
// squares is never -0, and a NaN range (a NaN or an inf - inf coordinate difference) has bits above +inf's: behind every other
CLOUD_KEYS_HD inline uint32_t range_key(float x, float y, float z, float ox, float oy, float oz)
{
  const float dx = x - ox, dy = y - oy, dz = z - oz;
  const float r2 = dx * dx + dy * dy + dz * dz;
  uint32_t u;
  memcpy(&u, &r2, sizeof(u));
  return u;
}

#if defined(__HIPCC__)
// ... of float4 points on the device (mm6 = the cloud's {min x, y, z, max x, y, z}, device memory)
__device__ inline uint32_t morton_key_drop(const float* __restrict__ mm6)
{
  return morton_drop_bits(mm6, mm6 + 3);
}

__device__ inline uint32_t morton_scan_key(const float4 p, const float* __restrict__ mm6)
{
  return morton_key(p.x, p.y, p.z, mm6) >> morton_key_drop(mm6);
}

__device__ inline uint32_t range_scan_key(const float4 p, const float4* __restrict__ origins, uint32_t n_o, int* __restrict__ error)
{
  uint32_t og = __float_as_uint(p.w);
  if (og >= n_o)
  {
    *error = 2;
    og = 0;
  }
  const float4 o = origins[og];
  return range_key(p.x, p.y, p.z, o.x, o.y, o.z);
}
#endif  // __HIPCC__
}  // namespace mcl3dl
