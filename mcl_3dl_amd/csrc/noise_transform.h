// noise_transform.h — MultivariateNoiseGenerator::setCovariance (multivariate_noise_generator.h:63-77) for six dimensions, on the
// host: norm_transform_ = V diag(sqrt(lambda)) of the covariance's eigen-decomposition, the matrix
// mcl3dl_hip_group_init_drawn_multivariate multiplies every particle's six normal values with. Plain C++ (no HIP type appears
// here): tests/cpp/noise_transform_check.cpp compiles it with g++.
//
// THE DEFINITION IS THIS PROJECT'S OWN, as the normals of DESIGN.md 3.5.1 are. The reference hands the matrix to
// Eigen::SelfAdjointEigenSolver<Matrix<float>>, whose eigenvectors differ between Eigen releases and, within a repeated eigenvalue
// (rviz's default covariance has two), are any orthonormal basis of the eigenspace. No release's eigenvectors are reproduced here:
// particles drawn with this T have the reference's DISTRIBUTION (T T^T = the float-cast covariance), not the reference's bits. A
// caller who wants the reference's particles value for value computes Eigen's own
// eigenvectors() * eigenvalues().cwiseSqrt().asDiagonal() and hands that to the device call — which is why the device call takes
// the transform and not the covariance.
//
//   1. the 36 doubles are cast to float (the reference's Matrix<float> stores them so) and only the lower triangle is read
//      (SelfAdjointEigenSolver's rule): c(i, j) = c(j, i) = (float)cov36[6 i + j], i >= j. All 36 must be finite as floats.
//   2. cyclic Jacobi in fp64, pairs (p, q) in row order, the rotation that zeroes a(p, q) by the smaller root
//      t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / (2 a_pq); sweeps until every off-diagonal element is
//      exactly 0, 30 at the most.
//   3. eigenvalues ascending (Eigen's order), equal ones in the order of their columns.
//   4. each eigenvector's sign is chosen so that its component of largest magnitude is positive (the lowest index on a tie).
//   5. T[i][k] = (float)(V[i][k] sqrt(lambda_k)), formed in double and rounded once; row-major.
//
// NEGATIVE EIGENVALUES. The reference takes sqrt of a negative eigenvalue and fills the particle set with NaN. Rounding the entries
// to float moves each eigenvalue of a positive semi-definite input by at most |E|_F <= 2^-24 |C|_F (Weyl); twice that covers the
// fp64 Jacobi's own residual. So an eigenvalue in [-2^-23 |C|_F, 0) is set to 0, and anything more negative is rejected with -3 and
// a message that names the eigenvalue.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdio>

namespace mcl3dl
{
constexpr int NOISE_TRANSFORM_SWEEPS = 30;

// 0, or -3 with the reason in msg (msg_cap bytes; may be null). eigenvalues6 (may be null) takes the six eigenvalues behind the
// clamp, ascending, as floats; *n_clamped (may be null) how many of them the clamp set to 0.
inline int noise_transform6(const double* cov36, float* transform36, float* eigenvalues6, int* n_clamped, char* msg, size_t msg_cap)
{
  const auto fail = [&](const char* fmt, auto... args)
  {
    if (msg && msg_cap)
      snprintf(msg, msg_cap, fmt, args...);
    return -3;
  };
  if (!cov36)
    return fail("%s", "null cov36");
  if (!transform36)
    return fail("%s", "null transform36");
  double a[6][6], v[6][6];
  double frob2 = 0.0;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)
    {
      if (!std::isfinite(static_cast<float>(cov36[6 * i + j])))
        return fail("cov36[%d] is not finite as a float", 6 * i + j);
      v[i][j] = i == j ? 1.0 : 0.0;
      if (i >= j)
        a[i][j] = a[j][i] = static_cast<double>(static_cast<float>(cov36[6 * i + j]));
    }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)
      frob2 += a[i][j] * a[i][j];
  for (int sweep = 0; sweep < NOISE_TRANSFORM_SWEEPS; ++sweep)
  {
    bool diagonal = true;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q)
        diagonal = diagonal && a[p][q] == 0.0;
    if (diagonal)
      break;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q)
      {
        if (a[p][q] == 0.0)
          continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        a[p][p] -= t * a[p][q];
        a[q][q] += t * a[p][q];
        a[p][q] = a[q][p] = 0.0;
        for (int r = 0; r < 6; ++r)
        {
          if (r == p || r == q)
            continue;
          const double rp = a[r][p], rq = a[r][q];
          a[r][p] = a[p][r] = c * rp - s * rq;
          a[r][q] = a[q][r] = s * rp + c * rq;
        }
        for (int k = 0; k < 6; ++k)
        {
          const double vp = v[k][p], vq = v[k][q];
          v[k][p] = c * vp - s * vq;
          v[k][q] = s * vp + c * vq;
        }
      }
  }
  // ascending, equal eigenvalues in column order (an insertion sort: stable)
  int order[6] = { 0, 1, 2, 3, 4, 5 };
  for (int i = 1; i < 6; ++i)
    for (int j = i; j > 0 && a[order[j]][order[j]] < a[order[j - 1]][order[j - 1]]; --j)
    {
      const int o = order[j];
      order[j] = order[j - 1];
      order[j - 1] = o;
    }
  const double clamp_below = -std::ldexp(std::sqrt(frob2), -23);
  int clamped = 0;
  double root[6];
  for (int k = 0; k < 6; ++k)
  {
    double lambda = a[order[k]][order[k]];
    if (!(lambda >= 0.0))
    {
      if (!(lambda >= clamp_below))
        return fail("eigenvalue %d of the covariance is %g, below -2^-23 |C|_F = %g: not positive semi-definite", k, lambda,
                    clamp_below);
      lambda = 0.0;
      ++clamped;
    }
    root[k] = std::sqrt(lambda);
    if (eigenvalues6)
      eigenvalues6[k] = static_cast<float>(lambda);
  }
  for (int k = 0; k < 6; ++k)
  {
    const int col = order[k];
    int big = 0;
    for (int i = 1; i < 6; ++i)
      if (std::fabs(v[i][col]) > std::fabs(v[big][col]))
        big = i;
    const double sign = v[big][col] < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 6; ++i)
      transform36[6 * i + k] = static_cast<float>(sign * v[i][col] * root[k]);
  }
  if (n_clamped)
    *n_clamped = clamped;
  return 0;
}
}  // namespace mcl3dl
