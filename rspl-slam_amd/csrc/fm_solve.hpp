// cv::findFundamentalMat(FM_RANSAC)'s per-hypothesis arithmetic (OpenCV 4.2 fundam.cpp: run7Point,
// FMEstimatorCallback::checkSubset / computeError) as ONE source compiled for the host and for the device:
// fm_hyp_kernel runs it one lane per hypothesis, rspl_fm_debug_seven_point / rspl_fm_debug_subsets and the CPU
// tests run the host instantiation.
//
//   collinear    haveCollinearPoints: the subset's LAST point against every pair of earlier ones,
//                |dx2 dy1 - dy2 dx1| <= FLT_EPSILON (|dx1| + |dy1| + |dx2| + |dy2|)
//   seven_point  rows (x1 x0, x1 y0, x1, y1 x0, y1 y0, y1, x0, y0, 1); the two-dimensional null space by
//                Gauss-Jordan elimination with complete pivoting (OpenCV takes the last two right singular
//                vectors; the models do not depend on the basis once F33 = 1); det(l G + H) = 0 with
//                G = f1 - f2, H = f2; cv::solveCubic; F = (l G + H) / s with s = l G33 + H33 when
//                |s| > DBL_EPSILON; a model with a non-finite entry is dropped
//   error        max(d1^2 s1, d2^2 s2) rounded to float
//
// The 7x9 matrix and the two null vectors are indexed by run-time pivots, so they live in a caller-provided
// workspace addressed with a stride: the host passes a local array (stride 1), the kernel a lane's column of
// an LDS tile (stride 64: lane l owns word l of every row of 64, conflict-free) -- nothing here indexes a
// register array dynamically, so nothing goes to scratch.  Contraction is off on both sides.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace rspl {
namespace fm {

constexpr int kModelPoints = 7;
constexpr int kWork = 63 + 18;  // doubles of workspace per solve: the 7x9 matrix | f1 | f2

#define RSPL_FM_HD __host__ __device__ __forceinline__

// haveCollinearPoints(m, 7) on p[7][2]
RSPL_FM_HD bool collinear7(const double* p) {
#pragma clang fp contract(off)
  const double xi = p[12], yi = p[13];
  bool hit = false;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const double dx1 = p[2 * j] - xi, dy1 = p[2 * j + 1] - yi;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      if (k < j) {
        const double dx2 = p[2 * k] - xi, dy2 = p[2 * k + 1] - yi;
        hit |= fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
      }
    }
  }
  return hit;
}

// FMEstimatorCallback::checkSubset
RSPL_FM_HD bool check_subset(const double* p0, const double* p1) { return !collinear7(p0) && !collinear7(p1); }

// FMEstimatorCallback::computeError for one correspondence
RSPL_FM_HD float sampson_max(const double* F, double x0, double y0, double x1, double y1) {
#pragma clang fp contract(off)
  double a = F[0] * x0 + F[1] * y0 + F[2];
  double b = F[3] * x0 + F[4] * y0 + F[5];
  double c = F[6] * x0 + F[7] * y0 + F[8];
  const double s2 = 1. / (a * a + b * b);
  const double d2 = x1 * a + y1 * b + c;
  a = F[0] * x1 + F[3] * y1 + F[6];
  b = F[1] * x1 + F[4] * y1 + F[7];
  c = F[2] * x1 + F[5] * y1 + F[8];
  const double s1 = 1. / (a * a + b * b);
  const double d1 = x0 * a + y0 * b + c;
  const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
  return (float)(e1 > e2 ? e1 : e2);  // std::max(d1 d1 s1, d2 d2 s2)
}

namespace detail {

RSPL_FM_HD double det3(double a0, double a1, double a2, double b0, double b1, double b2, double c0, double c1,
                       double c2) {  // columns a, b, c
#pragma clang fp contract(off)
  return a0 * (b1 * c2 - b2 * c1) - b0 * (a1 * c2 - a2 * c1) + c0 * (a1 * b2 - a2 * b1);
}

// cv::solveCubic for c0 x^3 + c1 x^2 + c2 x + c3; returns the root count (0 .. 3)
RSPL_FM_HD int solve_cubic(double a0, double a1, double a2, double a3, double& x0, double& x1, double& x2) {
#pragma clang fp contract(off)
  x0 = x1 = x2 = 0.;
  if (a0 == 0) {
    if (a1 == 0) {
      if (a2 == 0) return 0;
      x0 = -a3 / a2;
      return 1;
    }
    double d = a2 * a2 - 4 * a1 * a3;
    if (!(d >= 0)) return 0;
    d = sqrt(d);
    const double q1 = (-a2 + d) * 0.5, q2 = (a2 + d) * -0.5;
    if (fabs(q1) > fabs(q2)) {
      x0 = q1 / a1;
      x1 = a3 / q1;
    } else {
      x0 = q2 / a1;
      x1 = a3 / q2;
    }
    return d > 0 ? 2 : 1;
  }
  a0 = 1. / a0;
  a1 *= a0;
  a2 *= a0;
  a3 *= a0;
  const double Q = (a1 * a1 - 3 * a2) * (1. / 9);
  const double R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1. / 54);
  const double Qcubed = Q * Q * Q;
  double d = Qcubed - R * R;
  if (d > 0) {
    const double theta = acos(R / sqrt(Qcubed));
    const double t0 = -2 * sqrt(Q), t1 = theta * (1. / 3), t2 = a1 * (1. / 3);
    x0 = t0 * cos(t1) - t2;
    x1 = t0 * cos(t1 + (2. * 3.14159265358979323846 / 3)) - t2;
    x2 = t0 * cos(t1 + (4. * 3.14159265358979323846 / 3)) - t2;
    return 3;
  }
  if (d == 0) {
    if (R >= 0) {
      x0 = -2 * pow(R, 1. / 3) - a1 / 3;
      x1 = pow(R, 1. / 3) - a1 / 3;
    } else {
      x0 = 2 * pow(-R, 1. / 3) - a1 / 3;
      x1 = -pow(-R, 1. / 3) - a1 / 3;
    }
    if (x0 == x1) {
      x1 = 0.;
      return 1;
    }
    return 2;
  }
  if (!(d < 0)) return 0;  // NaN coefficients
  d = sqrt(-d);
  double e = pow(d + fabs(R), 1. / 3);
  if (R > 0) e = -e;
  x0 = (e + Q / e) - a1 * (1. / 3);
  return 1;
}

// entry i of the column permutation packed four bits each
RSPL_FM_HD int nib(uint64_t p, int i) { return (int)((p >> (4 * i)) & 15u); }

}  // namespace detail

// run7Point on p0[7][2], p1[7][2] (float-rounded pixels).  w: kWork doubles of workspace, element i at
// w[i * S].  F[3][9] (memory, not a register array: slot n is a run-time index): the models, n (the
// return value) of them valid.
template <int S>
RSPL_FM_HD int seven_point(const double* p0, const double* p1, double* w, double* F) {
#pragma clang fp contract(off)
  using namespace detail;
#define A_(r, c) w[((r) * 9 + (c)) * S]
#pragma unroll
  for (int i = 0; i < 7; i++) {
    const double x0 = p0[2 * i], y0 = p0[2 * i + 1], x1 = p1[2 * i], y1 = p1[2 * i + 1];
    A_(i, 0) = x1 * x0; A_(i, 1) = x1 * y0; A_(i, 2) = x1;
    A_(i, 3) = y1 * x0; A_(i, 4) = y1 * y0; A_(i, 5) = y1;
    A_(i, 6) = x0;      A_(i, 7) = y0;      A_(i, 8) = 1.;
  }
  // Gauss-Jordan, complete pivoting: rows and columns are swapped in place, perm[c] = the unknown column c holds
  uint64_t perm = 0x876543210ull;
  for (int k = 0; k < 7; k++) {
    double best = -1.;
    int pr = k, pc = k;
    for (int r = k; r < 7; r++)
      for (int c = k; c < 9; c++) {
        const double v = fabs(A_(r, c));
        if (v > best) {  // the first maximum; a NaN never wins
          best = v;
          pr = r;
          pc = c;
        }
      }
    if (!(best > 0.) || !(best <= DBL_MAX)) return 0;  // rank below 7, or a non-finite entry: no model
    if (pr != k)
      for (int c = 0; c < 9; c++) {
        const double t = A_(k, c);
        A_(k, c) = A_(pr, c);
        A_(pr, c) = t;
      }
    if (pc != k) {
      for (int r = 0; r < 7; r++) {
        const double t = A_(r, k);
        A_(r, k) = A_(r, pc);
        A_(r, pc) = t;
      }
      const uint64_t a = (uint64_t)nib(perm, k), b = (uint64_t)nib(perm, pc);
      perm &= ~((15ull << (4 * k)) | (15ull << (4 * pc)));
      perm |= (b << (4 * k)) | (a << (4 * pc));
    }
    const double inv = 1. / A_(k, k);
    for (int c = k; c < 9; c++) A_(k, c) = A_(k, c) * inv;
    for (int r = 0; r < 7; r++) {
      if (r == k) continue;
      const double fac = A_(r, k);
      for (int c = k; c < 9; c++) A_(r, c) = A_(r, c) - fac * A_(k, c);
    }
  }
  // the null vectors of the free columns 7 and 8, each scaled to unit length
  double* f = w + 63 * S;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    double* fj = f + 9 * j * S;
    double n2 = 1.;
    for (int i = 0; i < 7; i++) {
      const double v = -A_(i, 7 + j);
      fj[nib(perm, i) * S] = v;
      n2 = n2 + v * v;
    }
    fj[nib(perm, 7 + j) * S] = 1.;
    fj[nib(perm, 8 - j) * S] = 0.;
    const double sc = 1. / sqrt(n2);
    for (int i = 0; i < 9; i++) fj[i * S] = fj[i * S] * sc;
  }
#undef A_
  double G[9], H[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    H[i] = f[(9 + i) * S];
    G[i] = f[i * S] - H[i];
  }
  // det(l G + H): the columns of the 3x3 (row-major G, H) mixed
#define COL(M, k) M[k], M[3 + k], M[6 + k]
  const double c0 = det3(COL(G, 0), COL(G, 1), COL(G, 2));
  const double c1 = det3(COL(H, 0), COL(G, 1), COL(G, 2)) + det3(COL(G, 0), COL(H, 1), COL(G, 2)) +
                    det3(COL(G, 0), COL(G, 1), COL(H, 2));
  const double c2 = det3(COL(G, 0), COL(H, 1), COL(H, 2)) + det3(COL(H, 0), COL(G, 1), COL(H, 2)) +
                    det3(COL(H, 0), COL(H, 1), COL(G, 2));
  const double c3 = det3(COL(H, 0), COL(H, 1), COL(H, 2));
#undef COL
  double r[3];
  const int nr = solve_cubic(c0, c1, c2, c3, r[0], r[1], r[2]);
  int n = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (k < nr) {
      double lambda = r[k], mu = 1.;
      const double s = G[8] * r[k] + H[8];
      double M[9];
      if (fabs(s) > DBL_EPSILON) {
        mu = 1. / s;
        lambda = lambda * mu;
        M[8] = 1.;
      } else {
        M[8] = 0.;
      }
      bool fin = true;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        M[i] = G[i] * lambda + H[i] * mu;
        fin = fin && fabs(M[i]) <= DBL_MAX;
      }
      if (fin) {
#pragma unroll
        for (int i = 0; i < 9; i++) F[9 * n + i] = M[i];
        n++;
      }
    }
  }
  return n;
}

}  // namespace fm
}  // namespace rspl
