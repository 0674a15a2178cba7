// scan_accum.h — the head of MCL3dlNode::measure() on the device: accumCloud (src/mcl_3dl.cpp:274-302: sensor -> odom,
// label = index of the accumulated cloud, append to pc_local_accum_) and the transform of the whole accumulation
// odom -> base_link at the last stamp (:319-336), in front of the VoxelGrid of cloud_kernels.h.
//
//   scan_accum_push_kernel            xyz array          -> transform, stamp the label, one float4 per point behind the
//   scan_accum_push_pc2_kernel        PointCloud2 bytes  -> points the accumulation already holds
//   scan_accum_to_raw_minmax_kernel   accumulation -> the scan path's raw cloud, with the min / max / finite count VoxelGrid needs
//
// Both transforms are ONE expression per output row, in float32, every product and sum rounded on its own (no fused
// multiply-add), and they are never composed: the points sit in the odom frame as floats between them, as pc_local_accum_
// does. The reference takes this arithmetic from tf2_sensor_msgs / PCL over an Eigen that is neither vendored nor pinned:
// parity here is against this restatement. accum_affine_apply compiles for the host too:
// tests/cpp/scan_accum_check.cpp holds it against tests/scan_accum_ref.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "cloud_kernels.h"  // load_u32_unaligned, MinMaxOut / block_minmax_finish
#define SCAN_ACCUM_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define SCAN_ACCUM_HD
#endif

namespace mcl3dl
{
struct AccumPoint
{
  float x, y, z;
};

// m: the rows of the 3x4 [R | t]. out[r] = ((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3] — the order PCL >= 1.10's
// Transformer::se3 spells out; within gamma_4 (|m0 x| + |m1 y| + |m2 z| + |t|) of the real-number result, as any association is
SCAN_ACCUM_HD inline AccumPoint accum_affine_apply(const float m[12], float x, float y, float z)
{
  AccumPoint o;
  o.x = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
  o.y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
  o.z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
  return o;
}

#if defined(__HIPCC__)
// a kernel argument: the matrix travels with the launch. on == 0: no transform, the coordinates' bits are copied
struct AccumAffine
{
  float m[12];
  int on;
};

__device__ inline float4 accum_point(const AccumAffine& a, float x, float y, float z, uint32_t label_bits)
{
  if (!a.on)
    return make_float4(x, y, z, __uint_as_float(label_bits));
  const AccumPoint p = accum_affine_apply(a.m, x, y, z);
  return make_float4(p.x, p.y, p.z, __uint_as_float(label_bits));
}

// `out` points at the first free slot of the accumulation (n more points fit behind it: the host grew the buffer)
__global__ __launch_bounds__(256) void scan_accum_push_kernel(const float* __restrict__ xyz, long long n, AccumAffine a,
                                                              uint32_t label, float4* __restrict__ out)
{
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * 256)
    out[i] = accum_point(a, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], label);
}

// the same from little-endian PointCloud2 rows (the byte loads of cloud_decode_kernel); the message's own label field is not
// read: accumCloud overwrites it
__global__ __launch_bounds__(256) void scan_accum_push_pc2_kernel(const uint8_t* __restrict__ data, long long n, uint32_t point_step,
                                                                  int off_x, int off_y, int off_z, AccumAffine a, uint32_t label,
                                                                  float4* __restrict__ out)
{
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * 256)
  {
    const uint8_t* p = data + static_cast<size_t>(i) * point_step;
    out[i] = accum_point(a, __uint_as_float(load_u32_unaligned(p + off_x)), __uint_as_float(load_u32_unaligned(p + off_y)),
                         __uint_as_float(load_u32_unaligned(p + off_z)), label);
  }
}

// accumulation (odom frame) -> raw cloud of the scan path (base_link), labels kept, + its min / max / finite count (one launch;
// the launch shape of cloud_pack_minmax_kernel)
__global__ __launch_bounds__(256) void scan_accum_to_raw_minmax_kernel(const float4* __restrict__ accum, long long n, AccumAffine a,
                                                                       float4* __restrict__ out, MinMaxOut mm)
{
  float mn[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, mx[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
  unsigned cnt = 0;
  for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * 256)
  {
    const float4 p = accum[i];
    const float4 q = accum_point(a, p.x, p.y, p.z, __float_as_uint(p.w));
    out[i] = q;
    minmax_accumulate(q, mn, mx, cnt);
  }
  block_minmax_finish(mn, mx, cnt, mm);
}
#endif  // __HIPCC__

}  // namespace mcl3dl
