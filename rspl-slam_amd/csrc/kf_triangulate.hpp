// Map::TriangulateMappoint (src/map.cc:292-339) for one map point, fp64, as ONE routine compiled for the
// host and for the device: kf_triangulate_kernel runs it one lane per point, rspl_map_insert_keyframe
// without a keyframe builder and the CPU tests run the host instantiation of the same source.
//
//   bearings  b_k = R_k ((x - cx) fx_inv, (y - cy) fy_inv, 1)  (Camera::BackProjectMono, camera.cc:150-155:
//             the inverse focal lengths are products), centres c_k = t_k, in observer order; an observer
//             with obs_pose < 0 (its frame is not in the map, or -- see below -- its keypoint index is
//             out of range) is skipped; fewer than 2 valid observers -> kTriFew
//   system    AxtAx = n I - sum_k b_k b_k^T / |b_k|^2,  Axtbx = sum_k c_k - sum_k b_k (b_k . c_k) / |b_k|^2
//   solve     column-pivoted Householder QR of the 3x3 as Eigen::ColPivHouseholderQR does it: pivot by the
//             largest remaining column norm (the first on a tie), rank = #{ |R_ii| > 1e-5 max |R_ii| },
//             rank < 3 -> kTriRank, otherwise Q^T rhs, back substitution, the permutation undone.
//
// Deviation from the reference: Frame::GetKeypointPosition accepts idx == cols (frame.cc:215, `>`) and
// would read past the feature matrix.  The callers of this routine treat a keypoint index >= the frame's
// keypoint count as an invalid observer (obs_pose = -1), which is skipped.
//
// Everything is compiled with contraction off and stays in registers: every array index is a constant
// after unrolling, column swaps are selects.  Division and square root are IEEE on both sides, so the host
// and the device instantiation agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rspl {
namespace kf {

constexpr int kTriFew = 0, kTriOk = 1, kTriRank = 2;  // RSPL_KF_TRI_*
constexpr double kRankLossTolerance = 1e-5;           // map.cc:331

namespace tri_detail {

__host__ __device__ __forceinline__ void swap2(double& a, double& b) {
  const double t = a;
  a = b;
  b = t;
}

// columns p and q of A (constant p, q) and the permutation entries
template <int P, int Q>
__host__ __device__ __forceinline__ void swap_cols(double (&A)[3][3], int (&perm)[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) swap2(A[r][P], A[r][Q]);
  const int t = perm[P];
  perm[P] = perm[Q];
  perm[Q] = t;
}

// Householder step K of the QR: reflect column K's rows K.. onto e_K, apply it to the columns right of K
// and to the right-hand side.  Returns beta = R_KK.  (Eigen's makeHouseholder: a tail below the smallest
// normal number is no reflection.)
template <int K>
__host__ __device__ __forceinline__ double householder(double (&A)[3][3], double (&y)[3]) {
#pragma clang fp contract(off)
  const double c0 = A[K][K];
  double tail2 = 0.0;
#pragma unroll
  for (int r = K + 1; r < 3; r++) tail2 = tail2 + A[r][K] * A[r][K];
  if (!(tail2 > 2.2250738585072014e-308)) return c0;
  double beta = sqrt(c0 * c0 + tail2);
  if (c0 >= 0.0) beta = -beta;
  const double den = c0 - beta, tau = (beta - c0) / beta;
  double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int r = K + 1; r < 3; r++) v[r] = A[r][K] / den;
#pragma unroll
  for (int c = K + 1; c < 3; c++) {
    double s = A[K][c];
#pragma unroll
    for (int r = K + 1; r < 3; r++) s = s + v[r] * A[r][c];
    const double ts = tau * s;
    A[K][c] = A[K][c] - ts;
#pragma unroll
    for (int r = K + 1; r < 3; r++) A[r][c] = A[r][c] - v[r] * ts;
  }
  double s = y[K];
#pragma unroll
  for (int r = K + 1; r < 3; r++) s = s + v[r] * y[r];
  const double ts = tau * s;
  y[K] = y[K] - ts;
#pragma unroll
  for (int r = K + 1; r < 3; r++) y[r] = y[r] - v[r] * ts;
  return beta;
}

}  // namespace tri_detail

// A x = rhs by the pivoted QR.  Returns the rank decision (kTriOk / kTriRank); *ratio (nullable) receives
// min |R_ii| / max |R_ii|, the quantity the threshold is applied to.
__host__ __device__ __forceinline__ int solve3_colpiv(double (&A)[3][3], double (&y)[3], double (&x)[3],
                                                      double* ratio) {
#pragma clang fp contract(off)
  using namespace tri_detail;
  int perm[3] = {0, 1, 2};
  // step 0: the largest of the three column norms
  {
    const double n0 = sqrt(A[0][0] * A[0][0] + A[1][0] * A[1][0] + A[2][0] * A[2][0]);
    const double n1 = sqrt(A[0][1] * A[0][1] + A[1][1] * A[1][1] + A[2][1] * A[2][1]);
    const double n2 = sqrt(A[0][2] * A[0][2] + A[1][2] * A[1][2] + A[2][2] * A[2][2]);
    if (n1 > n0 && !(n2 > n1)) swap_cols<0, 1>(A, perm);
    else if (n2 > n0 && n2 > n1) swap_cols<0, 2>(A, perm);
  }
  const double r0 = householder<0>(A, y);
  // step 1: the larger of the two remaining columns' norms below row 0
  {
    const double n1 = sqrt(A[1][1] * A[1][1] + A[2][1] * A[2][1]);
    const double n2 = sqrt(A[1][2] * A[1][2] + A[2][2] * A[2][2]);
    if (n2 > n1) swap_cols<1, 2>(A, perm);
  }
  const double r1 = householder<1>(A, y);
  const double r2 = A[2][2];
  const double a0 = fabs(r0), a1 = fabs(r1), a2 = fabs(r2);
  const double mx = a0 > a1 ? (a0 > a2 ? a0 : a2) : (a1 > a2 ? a1 : a2);
  const double mn = a0 < a1 ? (a0 < a2 ? a0 : a2) : (a1 < a2 ? a1 : a2);
  if (ratio) *ratio = mx > 0.0 ? mn / mx : 0.0;
  const double thr = mx * kRankLossTolerance;
  const int rank = (a0 > thr) + (a1 > thr) + (a2 > thr);
  x[0] = x[1] = x[2] = 0.0;
  if (rank < 3) return kTriRank;
  const double z2 = y[2] / r2;
  const double z1 = (y[1] - A[1][2] * z2) / r1;
  const double z0 = (y[0] - A[0][1] * z1 - A[0][2] * z2) / r0;
#pragma unroll
  for (int j = 0; j < 3; j++) x[j] = perm[0] == j ? z0 : (perm[1] == j ? z1 : z2);
  return kTriOk;
}

// One map point: poses Twc [.][16] row-major, its n_obs observers (pose index or -1, pixel x y).
// cam = fx fy cx cy.  p receives the position (zeros unless kTriOk).
__host__ __device__ __forceinline__ int triangulate_point(const double* Twc, const int32_t* obs_pose,
                                                          const double* obs_xy, int n_obs, const double* cam,
                                                          double* p, double* ratio) {
#pragma clang fp contract(off)
  const double fx_inv = 1.0 / cam[0], fy_inv = 1.0 / cam[1], cx = cam[2], cy = cam[3];
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, sc[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
  int n = 0;
  for (int k = 0; k < n_obs; k++) {
    const int f = obs_pose[k];
    if (f < 0) continue;
    const double* T = Twc + 16 * (size_t)f;
    const double u = (obs_xy[2 * k] - cx) * fx_inv, v = (obs_xy[2 * k + 1] - cy) * fy_inv;
    double b[3], c[3], d[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      b[r] = T[4 * r] * u + T[4 * r + 1] * v + T[4 * r + 2] * 1.0;
      c[r] = T[4 * r + 3];
    }
    const double inv = 1.0 / (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    const double bc = b[0] * c[0] + b[1] * c[1] + b[2] * c[2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      d[r] = b[r] * inv;
      sc[r] = sc[r] + c[r];
      sb[r] = sb[r] + d[r] * bc;
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int q = 0; q < 3; q++) S[r][q] = S[r][q] + d[r] * b[q];
    n++;
  }
  p[0] = p[1] = p[2] = 0.0;
  if (ratio) *ratio = 0.0;
  if (n < 2) return kTriFew;
  double A[3][3], y[3], x[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int q = 0; q < 3; q++) A[r][q] = (r == q ? (double)n : 0.0) - S[r][q];
    y[r] = sc[r] - sb[r];
  }
  const int rc = solve3_colpiv(A, y, x, ratio);
  p[0] = x[0]; p[1] = x[1]; p[2] = x[2];
  return rc;
}

}  // namespace kf
}  // namespace rspl
