// sampler_kernels.h — PointCloudSamplerWithNormal (include/mcl_3dl/point_cloud_random_samplers/
// point_cloud_sampler_with_normal.h:130-158): the surface normal of every point of a scan from its neighbours within
// normal_search_range, and the sampling weight the reference derives from it. pcl::NormalEstimation is not pinned by the
// reference, so the definition is this project's own: neighbour decisions in the float expression of
// mcl3dl_hip_radius_search, moments in fp64 about the query, a cyclic Jacobi solve in fp64. The neighbour search runs over a cell
// grid of the scan itself (host_grid_builders.h:build_transient_cell_grid, plain metric).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_grid.h"
#include "grid_kernels.h"
#include "map_structs.h"
#pragma clang fp contract(off)

namespace mcl3dl
{
// One Jacobi rotation of the symmetric 3x3 matrix in the (p, q) plane: app, aqq the two diagonal entries, apq the entry it
// annihilates, arp, arq the entries that couple p and q to the third index; (v?p, v?q) the two columns of the eigenvector
// matrix. Everything is a named scalar: an indexed 3x3 array would live in scratch memory.
__device__ inline void sn_jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                        double& v1p, double& v1q, double& v2p, double& v2q)
{
  if (apq == 0.0)
    return;
  const double theta = (aqq - app) / (2.0 * apq);
  // the smaller root of t^2 + 2 theta t - 1 = 0; a theta whose square overflows gives t = 0 (apq is negligible)
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0;
  v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1;
  v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2;
  v2q = s * a2 + c * b2;
}

constexpr int SN_JACOBI_SWEEPS = 8;  // cyclic Jacobi converges quadratically: a 3x3 is at rounding level after 4-5 sweeps

// Unit eigenvector of the smallest eigenvalue of the symmetric matrix { a00 a01 a02; a01 a11 a12; a02 a12 a22 }.
__device__ inline void sn_smallest_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22, double& nx,
                                               double& ny, double& nz)
{
  // eigenvectors do not change with a scale: entries of order one keep theta * theta away from overflow and underflow
  const double big = fmax(fmax(fmax(fabs(a00), fabs(a11)), fmax(fabs(a22), fabs(a01))), fmax(fabs(a02), fabs(a12)));
  if (big > 0.0 && isfinite(big))
  {
    const double sc = 1.0 / big;
    a00 *= sc;
    a01 *= sc;
    a02 *= sc;
    a11 *= sc;
    a12 *= sc;
    a22 *= sc;
  }
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < SN_JACOBI_SWEEPS; ++sweep)
  {
    sn_jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), third index 2
    sn_jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), third index 1
    sn_jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), third index 0
  }
  // (selects on the values: a choice between the columns written as branches is turned into an indexed load from scratch)
  const bool c1 = a11 < a00;
  const double lam = c1 ? a11 : a00;
  const bool c2 = a22 < lam;
  const double ex = c2 ? v02 : (c1 ? v01 : v00);
  const double ey = c2 ? v12 : (c1 ? v11 : v10);
  const double ez = c2 ? v22 : (c1 ? v21 : v20);
  const double inv = 1.0 / sqrt((ex * ex + ey * ey) + ez * ez);
  nx = ex * inv;
  ny = ey * inv;
  nz = ez * inv;
}

struct SnParams
{
  float r2;              // (float)(r * r): d2 < r2 makes a neighbour
  int reach;             // cells each way the neighbours can be in (build_transient_cell_grid)
  double fx, fy, fz;     // fpc_local, widened from float
  double max_weight_m1;  // max_weight - 1
};

// sum of q and of q q^T over the neighbours, q = neighbour - query in fp64, and their number
struct SnMoments
{
  double sx, sy, sz, sxx, sxy, sxz, syy, syz, szz;
  uint32_t cnt;
};

// the points [s, e) of the cell-sorted cloud against the query
__device__ inline void sn_accumulate_run(const float4* __restrict__ pts, uint32_t s, uint32_t e, const float4 q, float r2,
                                         SnMoments& m)
{
  const double qx = static_cast<double>(q.x), qy = static_cast<double>(q.y), qz = static_cast<double>(q.z);
  for (uint32_t i = s; i < e; ++i)
  {
    const float4 p = pts[i];
    // (neighbour minus query, where the searches subtract the other way round: the squares are the same floats)
    if (d2_simple(p.x, p.y, p.z, q.x, q.y, q.z) < r2)
    {
      // q_j = (double)p_j - (double)p_i: exact
      const double ux = static_cast<double>(p.x) - qx, uy = static_cast<double>(p.y) - qy, uz = static_cast<double>(p.z) - qz;
      m.sx += ux;
      m.sy += uy;
      m.sz += uz;
      m.sxx += ux * ux;
      m.sxy += ux * uy;
      m.sxz += ux * uz;
      m.syy += uy * uy;
      m.syz += uy * uz;
      m.szz += uz * uz;
      ++m.cnt;
    }
  }
}

// One lane per point, taken in CELL-SORTED order k (the lanes of a wavefront sit in the same few cells and walk the same
// runs); the results are scattered to the point's place in the cloud, g.pts[k].w. A non-finite point finds nobody (every
// distance to it fails the `<`), and nobody finds it. out_normal may be null. *n_without counts the points without a normal.
__global__ void __launch_bounds__(256) sampler_normal_weight_kernel(LikGrid g, long long n, SnParams prm, double* __restrict__ out_weight,
                                                                  float* __restrict__ out_normal,
                                                                  uint32_t* __restrict__ n_without)
{
  const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool live = k < n;
  bool without = false;
  if (live)
  {
    const float4 q = g.pts[k];
    const uint32_t self = __float_as_uint(q.w);
    SnMoments m{};
    if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z))
    {
      // the cell the grid's key kernel put this point into (the same expression), and the block of cells around it
      // (clamped like the key kernel's, in front of the block's own clamping)
      const Vec3f f = cell_of(g, q.x, q.y, q.z);
      const CellBlock b = cell_block(g, min(max(static_cast<int>(f.x), 0), g.nx - 1), min(max(static_cast<int>(f.y), 0), g.ny - 1),
                                     min(max(static_cast<int>(f.z), 0), g.nz - 1), prm.reach);
      for (int z = b.z0; z <= b.z1; ++z)
        for (int yb = b.y0; yb <= b.y1; yb += 5)
        {
          // the run delimiters of up to five rows of this layer together (reach 1: three rows, reach 2: five), then their points
          uint32_t s0, e0, s1, e1, s2, e2, s3, e3, s4, e4;
          cell_row_run(g, z, yb, b.y1, b.x0, b.x1, s0, e0);
          cell_row_run(g, z, yb + 1, b.y1, b.x0, b.x1, s1, e1);
          cell_row_run(g, z, yb + 2, b.y1, b.x0, b.x1, s2, e2);
          cell_row_run(g, z, yb + 3, b.y1, b.x0, b.x1, s3, e3);
          cell_row_run(g, z, yb + 4, b.y1, b.x0, b.x1, s4, e4);
          sn_accumulate_run(g.pts, s0, e0, q, prm.r2, m);
          sn_accumulate_run(g.pts, s1, e1, q, prm.r2, m);
          sn_accumulate_run(g.pts, s2, e2, q, prm.r2, m);
          sn_accumulate_run(g.pts, s3, e3, q, prm.r2, m);
          sn_accumulate_run(g.pts, s4, e4, q, prm.r2, m);
        }
    }
    double w = 1.0;
    float nxf = __uint_as_float(0x7fc00000u), nyf = nxf, nzf = nxf;
    without = m.cnt < 3u;
    if (!without)
    {
      const double kk = static_cast<double>(m.cnt);
      const double mx = m.sx / kk, my = m.sy / kk, mz = m.sz / kk;
      double nx, ny, nz;
      sn_smallest_eigenvector(m.sxx / kk - mx * mx, m.sxy / kk - mx * my, m.sxz / kk - mx * mz, m.syy / kk - my * my,
                              m.syz / kk - my * mz, m.szz / kk - mz * mz, nx, ny, nz);
      // :146-155: |n . fpc_local| clamped to 1, weight = 1 + (max_weight - 1) (pi/2 - acos) / (pi/2)
      double c = fabs((nx * prm.fx + ny * prm.fy) + nz * prm.fz);
      if (c > 1.0)
        c = 1.0;
      const double angle = acos(c);
      w = 1.0 + prm.max_weight_m1 * ((M_PI / 2 - angle) / (M_PI / 2));
      nxf = static_cast<float>(nx);
      nyf = static_cast<float>(ny);
      nzf = static_cast<float>(nz);
    }
    if (self < static_cast<unsigned long long>(n))
    {
      out_weight[self] = w;
      if (out_normal)
      {
        out_normal[3 * static_cast<size_t>(self) + 0] = nxf;
        out_normal[3 * static_cast<size_t>(self) + 1] = nyf;
        out_normal[3 * static_cast<size_t>(self) + 2] = nzf;
      }
    }
  }
  // one atomic per wavefront
  const unsigned long long votes = __ballot(live && without);
  if (votes && (threadIdx.x & 63) == static_cast<unsigned>(__ffsll(static_cast<long long>(votes)) - 1))
    atomicAdd(n_without, static_cast<uint32_t>(__popcll(votes)));
}
}  // namespace mcl3dl
