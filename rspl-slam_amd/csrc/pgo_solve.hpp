// Pose-graph optimisation (loop closure): the residual, Jacobian and update arithmetic of one
// edge as ONE source compiled for the host and for the device, and the tile geometry both sides share.
// pgo_kernels.hip runs it one thread per edge, rspl_pgo_debug_host and the CPU tests run the host instantiation.
//
//   pose       T_wc as a unit quaternion (x y z w) and a position
//   edge       Z = T_wi^-1 T_wj measured; with d = R_i^T (p_j - p_i):
//                e_t = d - t_Z,   e_R = Log(R_Z^T R_i^T R_j)
//              the log through the quaternion with w >= 0: 2 atan2(|v|, w) v / |v|, stable up to pi
//   update     p <- p + dp,  R <- R Exp(dphi)
//   Jacobians  de_t/ddp_i = -R_i^T   de_t/ddphi_i = [d]x   de_t/ddp_j = R_i^T
//              de_R/ddphi_j = Jr^-1(e_R)   de_R/ddphi_i = -Jr^-1(e_R) R_j^T R_i
//              Jr^-1(phi) = I + 1/2 [phi]x + c [phi]x^2, c = 1/theta^2 - (1 + cos theta) / (2 theta sin theta),
//              1/12 below theta = 1e-5
//   cost       w_t |e_t|^2 + w_r |e_R|^2;  H = sum J^T W J,  g = sum J^T W e  (b = -g)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace rspl {
namespace pgo {

constexpr int kPoseDim = 6;                   // (dp, dphi)
constexpr int kTilePoses = 16;                // free poses per tile
constexpr int kTile = kTilePoses * kPoseDim;  // 96: a tile is kTile x kTile doubles, row-major
constexpr int kTileElems = kTile * kTile;
constexpr int kMaxPoses = 4096;
constexpr int kMaxRejections = 10;
constexpr double kResolvable = 1e-12;  // a predicted decrease of at most this share of F ends the call: see rspl.h

#define RSPL_PGO_HD __host__ __device__ __forceinline__

// a * b, Hamilton product, x y z w
RSPL_PGO_HD void qmul(const double* a, const double* b, double* o) {
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  const double z = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}

// the conjugate of a times b
RSPL_PGO_HD void qcmul(const double* a, const double* b, double* o) {
  const double c[4] = {-a[0], -a[1], -a[2], a[3]};
  qmul(c, b, o);
}

RSPL_PGO_HD void qnormalize(const double* q, double* o) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  o[0] = q[0] / n; o[1] = q[1] / n; o[2] = q[2] / n; o[3] = q[3] / n;
}

// row-major rotation of a unit quaternion
RSPL_PGO_HD void qmat(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}

// Log of a unit quaternion, the branch with w >= 0
RSPL_PGO_HD void qlog(const double* q, double* phi) {
  const double s = q[3] < 0 ? -1.0 : 1.0;
  const double x = s * q[0], y = s * q[1], z = s * q[2], w = s * q[3];
  const double n = sqrt(x * x + y * y + z * z);
  const double k = n < 1e-8 ? 2.0 / w : 2.0 * atan2(n, w) / n;
  phi[0] = k * x; phi[1] = k * y; phi[2] = k * z;
}

// Exp as a quaternion
RSPL_PGO_HD void qexp(const double* phi, double* q) {
  const double t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  const double t = sqrt(t2);
  double k, w;
  if (t < 1e-5) {
    k = 0.5 - t2 / 48.0;
    w = 1.0 - t2 / 8.0;
  } else {
    k = sin(0.5 * t) / t;
    w = cos(0.5 * t);
  }
  q[0] = k * phi[0]; q[1] = k * phi[1]; q[2] = k * phi[2]; q[3] = w;
}

// Jr^-1(phi), row-major
RSPL_PGO_HD void jr_inv(const double* phi, double* J) {
  const double x = phi[0], y = phi[1], z = phi[2];
  const double t2 = x * x + y * y + z * z, t = sqrt(t2);
  const double c = t < 1e-5 ? 1.0 / 12.0 : 1.0 / t2 - (1.0 + cos(t)) / (2.0 * t * sin(t));
  // [phi]x^2 = phi phi^T - theta^2 I
  J[0] = 1 + c * (x * x - t2); J[1] = -0.5 * z + c * x * y;  J[2] = 0.5 * y + c * x * z;
  J[3] = 0.5 * z + c * x * y;  J[4] = 1 + c * (y * y - t2); J[5] = -0.5 * x + c * y * z;
  J[6] = -0.5 * y + c * x * z; J[7] = 0.5 * x + c * y * z;  J[8] = 1 + c * (z * z - t2);
}

// the update of one pose by d = (dp, dphi); the quaternion is normalised again
RSPL_PGO_HD void pose_update(const double* q, const double* p, const double* d, double* qo, double* po) {
  double dq[4], t[4];
  qexp(d + 3, dq);
  qmul(q, dq, t);
  qnormalize(t, qo);
  po[0] = p[0] + d[0]; po[1] = p[1] + d[1]; po[2] = p[2] + d[2];
}

struct EdgeGeometry {
  double Ri[9], d[3], e[6];
  double qij[4];  // R_i^T R_j
};

// the residual of one edge and what the Jacobians reuse
RSPL_PGO_HD void edge_residual(const double* qi, const double* pi, const double* qj, const double* pj, const double* qz,
                               const double* pz, EdgeGeometry& g) {
  qmat(qi, g.Ri);
  const double dx = pj[0] - pi[0], dy = pj[1] - pi[1], dz = pj[2] - pi[2];
  for (int c = 0; c < 3; c++) {
    g.d[c] = g.Ri[c] * dx + g.Ri[3 + c] * dy + g.Ri[6 + c] * dz;  // R_i^T (p_j - p_i)
    g.e[c] = g.d[c] - pz[c];
  }
  double qe[4];
  qcmul(qi, qj, g.qij);
  qcmul(qz, g.qij, qe);
  qnormalize(qe, qe);
  qlog(qe, g.e + 3);
}

RSPL_PGO_HD double edge_cost(const double* e, double wt, double wr) {
  return wt * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + wr * (e[3] * e[3] + e[4] * e[4] + e[5] * e[5]);
}

// One edge's share of the normal equations: Hii, Hij, Hjj row-major 6 x 6 (Hij: rows of i, columns of j),
// gi = Ji^T W e, gj = Jj^T W e.  The Jacobians' zero blocks are not multiplied.
//   Ji = [ -Ri^T  [d]x ]   Jj = [ Ri^T  0 ]
//        [  0     -B   ]        [ 0     A ]     A = Jr^-1(e_R), B = A R_j^T R_i
RSPL_PGO_HD void edge_blocks(const EdgeGeometry& g, double wt, double wr, double* Hii, double* Hij, double* Hjj,
                             double* gi, double* gj) {
  double A[9], Rji[9], B[9], Rij[9];
  jr_inv(g.e + 3, A);
  qmat(g.qij, Rij);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Rji[3 * r + c] = Rij[3 * c + r];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) B[3 * r + c] = A[3 * r] * Rji[c] + A[3 * r + 1] * Rji[3 + c] + A[3 * r + 2] * Rji[6 + c];
  const double dx[9] = {0, -g.d[2], g.d[1], g.d[2], 0, -g.d[0], -g.d[1], g.d[0], 0};
  double Ji[36], Jj[36];
  for (int k = 0; k < 36; k++) Ji[k] = Jj[k] = 0;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      const double rt = g.Ri[3 * c + r];  // Ri^T
      Ji[6 * r + c] = -rt;
      Ji[6 * r + 3 + c] = dx[3 * r + c];
      Ji[6 * (3 + r) + 3 + c] = -B[3 * r + c];
      Jj[6 * r + c] = rt;
      Jj[6 * (3 + r) + 3 + c] = A[3 * r + c];
    }
  for (int a = 0; a < 6; a++) {
    double si = 0, sj = 0;
    for (int r = 0; r < 6; r++) {
      const double w = r < 3 ? wt : wr;
      si += Ji[6 * r + a] * (w * g.e[r]);
      sj += Jj[6 * r + a] * (w * g.e[r]);
    }
    gi[a] = si;
    gj[a] = sj;
    for (int c = 0; c < 6; c++) {
      double ii = 0, ij = 0, jj = 0;
      for (int r = 0; r < 6; r++) {
        const double w = r < 3 ? wt : wr;
        ii += Ji[6 * r + a] * (w * Ji[6 * r + c]);
        ij += Ji[6 * r + a] * (w * Jj[6 * r + c]);
        jj += Jj[6 * r + a] * (w * Jj[6 * r + c]);
      }
      Hii[6 * a + c] = ii;
      Hij[6 * a + c] = ij;
      Hjj[6 * a + c] = jj;
    }
  }
}

// which 6 x 6 block of an edge a table entry adds: packed as edge * 4 + kind
enum BlockKind { kBlockII = 0, kBlockJJ = 1, kBlockIJ = 2, kBlockIJT = 3 };

RSPL_PGO_HD double block_entry(const double* eblk, int packed, int a, int c) {
  const double* e = eblk + (size_t)(packed >> 2) * 108;  // Hii | Hij | Hjj
  const int kind = packed & 3;
  return kind == kBlockII ? e[6 * a + c] : kind == kBlockJJ ? e[72 + 6 * a + c] : kind == kBlockIJ ? e[36 + 6 * a + c]
                                                                                                   : e[36 + 6 * c + a];
}

// packed lower triangle of a kTile x kTile tile
RSPL_PGO_HD int tri(int r, int c) { return r * (r + 1) / 2 + c; }
constexpr int kTriElems = kTile * (kTile + 1) / 2;

}  // namespace pgo
}  // namespace rspl
