// Local BA, device code shared by the kernels that linearise: per-edge Jacobians and weighted
// normal-equation contributions of point edges (landmark groups) and line edges (line workgroups), the
// small landmark-block inverses, the candidate pose, the outlier test and the block reduction.
// linearize_kernel and setup_kernel (ba_first.hip) and update_errors_kernel (ba_trial.hip) run the
// same lin_point_landmarks / point_edge_core / lin_lines; pair_chunk_kernel (ba_schur.hip) forms a
// point edge's pose block again with point_pose_block.  Everything here is __device__ __forceinline__.
#pragma once
#include "ba_device.hpp"
#include "wave_reduce.hpp"

namespace rspl {
namespace ba {

__device__ __forceinline__ double edge_weight_of(const Problem& P, const Active& A, const double* er, int t) {
  double w = einfo(t);
  if (A.robust) {
    double chi2 = 0;
    for (int k = 0; k < edim(t); k++) chi2 += er[k] * er[k];
    chi2 *= einfo(t);
    double r0, r1;
    huber(chi2, pick4(P.delta, t), r0, r1);
    w *= r1;  // robustInformation = rho'(chi2) * Omega
  }
  return w;
}

// point edges: analytic Jacobians (g2o types_sba, EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::linearizeOplus).
// Mono edges carry a zero third row, so every index below is a compile-time constant (register resident, no
// scratch).
__device__ __forceinline__ void point_jac_R(int t, const double (&R)[9], const double* tt, const double* cam,
                                            const double* Xg, double (&Jp)[3][6], double (&Jl)[3][3]) {
  const double fx = cam[0], fy = cam[1], bf = cam[4];
  double Xc[3];
  mat3_vec(R, Xg, Xc);
#pragma unroll
  for (int k = 0; k < 3; k++) Xc[k] += tt[k];
  const double x = Xc[0], y = Xc[1], z = Xc[2], iz = 1.0 / z, iz2 = iz * iz;
  const bool st = t == 1;
  const double D[3][3] = {{fx * iz, 0, -fx * x * iz2},
                          {0, fy * iz, -fy * y * iz2},
                          {st ? fx * iz : 0.0, 0, st ? -fx * x * iz2 + bf * iz2 : 0.0}};
  const double SX[9] = {0, -z, y, z, 0, -x, -y, x, 0};
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double s = 0, sl = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        s += D[r][k] * SX[k * 3 + c];
        sl += D[r][k] * R[k * 3 + c];
      }
      Jp[r][c] = s;            // -D * (-[Xc]x)
      Jp[r][3 + c] = -D[r][c]; // -D * I
      Jl[r][c] = -sl;          // -D * R
    }
}
__device__ __forceinline__ void point_jac(int t, const SE3& T, const double* cam, const double* Xg, double (&Jp)[3][6],
                                          double (&Jl)[3][3]) {
  double R[9];
  q_to_R(T.q, R);
  point_jac_R(t, R, T.t, cam, Xg, Jp, Jl);
}

// the pose block of one point edge: Hpp (upper triangle, pk6) = w Jp^T Jp, bp = -w Jp^T e
__device__ __forceinline__ void point_pose_terms(const double (&Jp)[3][6], double w, const double (&er)[3],
                                                 double (&Hp)[21], double (&bpv)[6]) {
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int b = a; b < 6; b++) Hp[pk6(a, b)] = w * (Jp[0][a] * Jp[0][b] + Jp[1][a] * Jp[1][b] + Jp[2][a] * Jp[2][b]);
    bpv[a] = -w * (Jp[0][a] * er[0] + Jp[1][a] * er[1] + Jp[2][a] * er[2]);
  }
}

// Writes the pose-side records of point edge e (when its pose is optimised): Hpl, and -- only with PDIAG
// (the first linearisation of an optimize(), read by computeLambdaInit's pose_diag) -- the six diagonal
// entries of Hpp.  The pose block itself (Hpp, bp) is never stored for a point edge: the diagonal pose
// pair's Schur chunk recomputes it from the state (point_pose_block), which costs less than the 216 bytes
// per edge and trial of writing it and reading it back.  Accumulates the landmark side (Hll 3x3, bl 3) into
// hl / bv.  The operands in registers (pose T, camera, landmark, the edge's error er).
template <bool PDIAG>
__device__ __forceinline__ void point_edge_core(const Problem& P, const Lin& L, const Active& A, int e, int t,
                                                bool pose_opt, const SE3& T, const double* cam, const double* Xg,
                                                const double* er4, double (&hl)[9], double (&bv)[3],
                                                double* dg6 = nullptr) {
  double Jp[3][6], Jl[3][3];
  point_jac(t, T, cam, Xg, Jp, Jl);
  const bool st = t == 1;
  const double w = edge_weight_of(P, A, er4, t);
  const double er[3] = {er4[0], er4[1], st ? er4[2] : 0.0};
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) hl[a * 3 + b] += w * (Jl[0][a] * Jl[0][b] + Jl[1][a] * Jl[1][b] + Jl[2][a] * Jl[2][b]);
#pragma unroll
  for (int a = 0; a < 3; a++) bv[a] += -w * (Jl[0][a] * er[0] + Jl[1][a] * er[1] + Jl[2][a] * er[2]);
  if (!pose_opt) return;
  double* Hpl = L.Hpl + 18 * e;  // (hpl_off: a point edge)
#pragma unroll
  for (int a = 0; a < 6; a++) {
    if (PDIAG) {
      const double d = w * (Jp[0][a] * Jp[0][a] + Jp[1][a] * Jp[1][a] + Jp[2][a] * Jp[2][a]);
      L.Hpp[21 * e + pk6(a, a)] = d;
      if (dg6) dg6[a] = d;
    }
#pragma unroll
    for (int b = 0; b < 3; b++) Hpl[a * 3 + b] = w * (Jp[0][a] * Jl[0][b] + Jp[1][a] * Jl[1][b] + Jp[2][a] * Jl[2][b]);
  }
}

// The pose block (Hpp upper triangle, bp) of a live point edge of type t on an optimised pose at the state
// its records were linearised at (pose rotation R / translation tt, camera cam, observation ob, point Xg of
// the current bank): the error, the robust weight and the pose Jacobian formed again, exactly as
// point_edge_core's linearisation (same operations on the same operands).
__device__ __forceinline__ void point_pose_block(const Problem& P, const Active& A, int t, const double* Rt,
                                                 const double* cam, const double* ob, const double* Xg,
                                                 double (&Hp)[21], double (&bpv)[6]) {
  double R[9];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = Rt[i];
  const double* tt = Rt + 9;
  double er4[4];
  point_error_R(t, cam, ob, R, tt, Xg, er4);
  double Jp[3][6], Jl[3][3];
  point_jac_R(t, R, tt, cam, Xg, Jp, Jl);
  const double w = edge_weight_of(P, A, er4, t);
  const double er[3] = {er4[0], er4[1], t == 1 ? er4[2] : 0.0};
  point_pose_terms(Jp, w, er, Hp, bpv);
}

// A diagonal pose pair's chunk: its pose (every e1 of its pairs is on it) and the cameras, for
// point_pose_block; the cameras in the chunk wave's LDS
struct DiagPose {
  const double* pose;  // R (9, row-major) and t (3) of the pose
  const double* cams;  // [ncam][5]
};

// (point edges: Hpl, and with PDIAG the Hpp diagonal pose_diag reads; see point_edge_core)
template <bool PDIAG>
__device__ __forceinline__ void zero_pose_records(const Lin& L, int e) {
  if (PDIAG)
#pragma unroll
    for (int k = 0; k < 6; k++) L.Hpp[21 * e + pk6(k, k)] = 0.0;
#pragma unroll
  for (int k = 0; k < 18; k++) L.Hpl[18 * e + k] = 0.0;
}

// point edges: analytic Jacobians (g2o types_sba).  Mono edges carry a zero third
// row, so every index below is a compile-time constant (register resident, no scratch).
// Writes the pose-side records of edge e (when its pose is optimised) and accumulates
// the landmark side (Hll 3x3, bl 3) into hl / bv.
__device__ __forceinline__ void point_edge(const Problem& P, const Lin& L, const Active& A, int e, bool pose_opt,
                                           const double* Tb, const double* Xg, double (&hl)[9], double (&bv)[3]) {
  if (A.elevel && A.elevel[e]) {  // outside this phase: exact-zero records, no contribution
    if (pose_opt) zero_pose_records<true>(L, e);
    return;
  }
  const int t = P.etype[e];
  point_edge_core<true>(P, L, A, e, t, pose_opt, load_T(Tb + 8 * P.epose[e]), P.cams + 5 * P.ecam[e], Xg, L.err + 4 * e, hl,
                  bv);
}

__device__ __forceinline__ void atomic_max_pos(double* addr, double v) {
  // non-negative doubles order like their bit patterns
  atomicMax(reinterpret_cast<unsigned long long*>(addr), (unsigned long long)__double_as_longlong(v));
}

// sum over the kGroup lanes of a landmark group (fixed butterfly: deterministic; every
// lane of the wave takes part)
constexpr int kGroup = 8;
#ifndef RSPL_UE_WAVES
#define RSPL_UE_WAVES 4
#endif
constexpr int kUeWaves = RSPL_UE_WAVES;  // waves per update_errors workgroup that carry landmark groups
template <int N>
__device__ __forceinline__ void group_sum(double (&v)[N]) {
#pragma unroll
  for (int o = 1; o < kGroup; o <<= 1)
#pragma unroll
    for (int i = 0; i < N; i++) v[i] += __shfl_xor(v[i], o);
}

// point landmarks: a group of kGroup lanes per landmark, lane j linearises edges j, j+8, ...
// of the landmark's CSR list; the group sums Hll / bl (no per-edge landmark records)
__device__ __forceinline__ void lin_point_landmarks(const Problem& P, const Lin& L, const Active& A, const Sys& S,
                                                    int t, bool maxd) {
  const int g = t / kGroup, j = t % kGroup;
  double hl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0};
  const bool in = g < P.nq;
  if (in) {
    const int k1 = A.lm_off[g + 1];
    for (int k = A.lm_off[g] + j; k < k1; k += kGroup)
      point_edge(P, L, A, (k), A.lm_pose[k] >= 0, P.T, P.X + 3 * g, hl, bv);
  }
  group_sum(hl);
  group_sum(bv);
  if (!in || j != 0 || !A.lm_act[g]) return;
  double* H = S.Hll + 16 * g;
#pragma unroll
  for (int i = 0; i < 9; i++) H[i] = hl[i];
#pragma unroll
  for (int i = 9; i < 16; i++) H[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++) S.bl[4 * g + i] = bv[i];
  S.bl[4 * g + 3] = 0.0;
  if (maxd) atomic_max_pos(S.out + 2, fmax(fabs(hl[0]), fmax(fabs(hl[4]), fabs(hl[8]))));
}

// Gauss-Jordan inverse with partial pivoting, fully unrolled (register resident).
// Progressive conditional row swaps select the same pivot as a max search.
template <int N>
__device__ __forceinline__ bool small_inv(const double* A, double* I) {
  double M[N][2 * N];
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      M[i][j] = A[i * N + j];
      M[i][N + j] = (i == j) ? 1.0 : 0.0;
    }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < N; c++) {
#pragma unroll
    for (int r = c + 1; r < N; r++) {
      const bool sw = fabs(M[r][c]) > fabs(M[c][c]);
#pragma unroll
      for (int k = 0; k < 2 * N; k++) {
        const double a = M[c][k], b = M[r][k];
        M[c][k] = sw ? b : a;
        M[r][k] = sw ? a : b;
      }
    }
    ok = ok && (M[c][c] != 0.0);
    const double iv = 1.0 / M[c][c];
#pragma unroll
    for (int k = 0; k < 2 * N; k++) M[c][k] *= iv;
#pragma unroll
    for (int r = 0; r < N; r++)
      if (r != c) {
        const double f = M[r][c];
#pragma unroll
        for (int k = 0; k < 2 * N; k++) M[r][k] -= f * M[c][k];
      }
  }
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) I[i * N + j] = M[i][N + j];
  return ok;
}

// (Hll_g + lambda I)^-1, zero-padded to 4x4 for points
__device__ __forceinline__ bool lm_dinv(const double* Hll, bool point, double lambda, double (&D)[16]) {
  if (point) {
    double H[9], Di[9];
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = Hll[i];
    H[0] += lambda;
    H[4] += lambda;
    H[8] += lambda;
    const bool ok = small_inv<3>(H, Di);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) D[i * 4 + j] = (i < 3 && j < 3) ? Di[i * 3 + j] : 0.0;
    return ok;
  }
  double H[16];
#pragma unroll
  for (int i = 0; i < 16; i++) H[i] = Hll[i];
#pragma unroll
  for (int i = 0; i < 4; i++) H[i * 5] += lambda;
  return small_inv<4>(H, D);
}

// line edges: g2o's numeric central difference (delta 1e-9).  A workgroup takes the
// <= kLineBlk = 8 edges of a run of whole line landmarks (A.ltab, CSR order) and splits the 20
// perturbed error evaluations of each by kind, so no
// wave diverges between the two transcendental paths: wave 0 evaluates the +-delta line
// perturbations of all 8 edges (Line3D::oplus, 8 lanes per edge), waves 1-2 the +-delta pose
// perturbations (SE3 exp, 12 lanes per edge).  The workgroup sums each landmark's edge
// records in CSR order into the landmark block itself; only a landmark with more than
// kLineBlk edges (split over workgroups) goes through per-edge records written through (sc1)
// and a last-edge ticket.
// MODE kLinSpec: the speculative linearisation (at the candidate P.Tn / candidate lines) inside
// update_errors_kernel, from the kernel's start: wave 0 forms the candidate of each of the block's
// line landmarks itself -- the same back-substitution as the landmark groups (8 lanes per
// landmark, the same butterfly, from the current records Lc / Sc) -- so it never waits for the
// groups; wave 3 evaluates each edge's own error at the candidate.
// MODE kLinSetup: the first pass of a device-LM optimize() (setup_kernel): wave 3 evaluates each
// edge's error at the current state (no separate error kernel), the block returns the robust cost of
// its edges (*chi_out, slot order) and, with cls (the second optimize), classifies its edges from
// their last computed errors itself (classify_edge) -- the landmark groups of the same launch write
// the levels, so none is read here.  The line edges' errors are not stored: the first trial's update
// rewrites every edge's error before anything reads them.
// candidate pose i of this trial (g2o VertexSE3Expmap::oplusImpl, the left update exp(xp) T):
// copied when the pose is not optimised or the solve failed
__device__ __forceinline__ void cand_pose(const Problem& P, const Active& A, const double* x, int i, bool failed,
                                          double (&o)[8]) {
  const int a = A.pidx[i];
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = P.T[8 * i + k];
  if (a < 0 || failed) return;
  double xp[6];
#pragma unroll
  for (int k = 0; k < 6; k++) xp[k] = x[6 * a + k];
  const SE3 r = se3_mul(se3_exp(xp), load_T(o));
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = r.q[k];
#pragma unroll
  for (int k = 0; k < 3; k++) o[4 + k] = r.t[k];
  o[7] = 0;
}

// outlier levels after the first optimize / final inlier flags (g2o_optimization.cc:176-231).
// Reads only fields that are NOT banked: L.err (swapped by neither bank_lin nor accept_swap) and the state
// P.T / P.X.  The speculative final kernel (SpecFinish, ba.cpp) reuses the Lin captured before optimize(5)
// and banks only the state; a classification that read a banked Lin field (Hpp, bp, Hll, bl, Hpl) would
// differ between that path and the host-ordered one (tests/test_gpu_ba.py test_ba_final_kernel_paths_agree).
__device__ __forceinline__ void edge_status(const Problem& P, const Lin& L, int e, double& chi2, bool& depth_ok) {
  const int t = P.etype[e];
  chi2 = 0;
  for (int k = 0; k < edim(t); k++) chi2 += L.err[4 * e + k] * L.err[4 * e + k];
  chi2 *= einfo(t);
  depth_ok = true;
  if (t < 2) {
    const SE3 T = load_T(P.T + 8 * P.epose[e]);
    double R[9], Xc[3];
    q_to_R(T.q, R);
    mat3_vec(R, P.X + 3 * P.elm[e], Xc);
    depth_ok = Xc[2] + T.t[2] > 0.0;
  }
}
constexpr int kLinPlain = 0, kLinSpec = 1, kLinSetup = 2;
// phase-2 level of edge e from its last computed error (classify_edge, g2o_optimization.cc:176-213)
__device__ __forceinline__ bool edge_outlier(const Problem& P, const Lin& L, int e) {
  double chi2;
  bool depth_ok;
  edge_status(P, L, e, chi2, depth_ok);
  return chi2 > pick4(P.th, P.etype[e]) || !depth_ok;
}
// line landmark g is active: it has an edge of level 0 (cls) / the phase's activity (A.lm_act)
__device__ __forceinline__ bool line_active(const Problem& P, const Lin& L, const Active& A, int g, bool cls) {
  if (!cls) return A.lm_act[g] != 0;
  for (int k = A.lm_off[g]; k < A.lm_off[g + 1]; k++)
    if (!edge_outlier(P, L, k)) return true;
  return false;
}
template <int MODE>
__device__ __forceinline__ void lin_lines(const Problem& P, const Lin& L, const Active& A, const Sys& S, int blk,
                                          bool maxd, const Lin* Lc = nullptr, const Sys* Sc = nullptr,
                                          double lambda = 0.0, bool failed = false,
                                          unsigned long long* stamp = nullptr, bool cls = false,
                                          double* chi_out = nullptr, double* pdg = nullptr, int pd_nb = 0,
                                          int pd_b = 0) {
  constexpr bool SPEC = MODE == kLinSpec, SETUP = MODE == kLinSetup, OWN_ERR = SPEC || SETUP;
  __shared__ double ev[kLineBlk][20][4];
  __shared__ double J[kLineBlk][4 * 6 + 4 * 4];
  __shared__ double Lsh[kLineBlk][6];
  __shared__ double es[kLineBlk][4];
  __shared__ int einfo_s[kLineBlk][4];  // edge id, type, flags (1 on, 2 live, 4 pose optimised), landmark
  __shared__ double cv[kLineBlk][20];   // landmark-side records (Hll 16, bl 4) of each edge
  __shared__ double Tsh[kLineBlk][8];   // SPEC: each edge's candidate pose
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int4 tb = A.ltab[blk];
  const int p0 = tb.x, cnt = tb.y & 0xff, gb = tb.z, ge = tb.w;
  const bool split = (tb.y >> 8) != 0;
  auto edge = [&](int slot, int& e, int& t, bool& on, bool& live) {
    e = einfo_s[slot][0];
    t = einfo_s[slot][1];
    on = einfo_s[slot][2] & 1;
    live = einfo_s[slot][2] & 2;
  };
  __shared__ double cand[kLineBlk][6];  // SPEC: the candidate line of landmark gb + m
  if (SPEC && wv == 0) {
    const int m = lane >> 3, j = lane & 7;
    const int g = gb + m;
    const bool in = g < ge;
    const int l = g - P.nq;
    const bool upd = in && A.lm_act[g] && !failed;
    double c[4] = {0, 0, 0, 0}, hb[20], lmv[6] = {0, 0, 0, 0, 0, 0};
    if (in) {  // the landmark-only operands in the first round trip
#pragma unroll
      for (int q = 0; q < 16; q++) hb[q] = Sc->Hll[16 * g + q];
#pragma unroll
      for (int q = 0; q < 4; q++) hb[16 + q] = Sc->bl[4 * g + q];
#pragma unroll
      for (int q = 0; q < 6; q++) lmv[q] = P.L[6 * l + q];
    }
    if (upd)
      for (int k = A.lm_off[g] + j; k < A.lm_off[g + 1]; k += kGroup) {
        const int a = A.lm_pose[k];
        if (a < 0) continue;
        const double* B = Lc->Hpl + hpl_off(P.Ep, k);  // (a line edge: 6 x 4)
        const double* xp = S.x + 6 * a;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          double sm = 0;
#pragma unroll
          for (int r = 0; r < 6; r++) sm += B[r * 4 + q] * xp[r];
          c[q] -= sm;
        }
      }
    group_sum(c);
    if (upd) {
#pragma unroll
      for (int q = 0; q < 4; q++) c[q] += hb[16 + q];
      double D[16];
      lm_dinv(hb, false, lambda, D);
      double xl[4];
#pragma unroll
      for (int r = 0; r < 4; r++) xl[r] = D[r * 4] * c[0] + D[r * 4 + 1] * c[1] + D[r * 4 + 2] * c[2] + D[r * 4 + 3] * c[3];
      line_oplus(lmv, xl);
    }
    if (in && j == 0)
#pragma unroll
      for (int q = 0; q < 6; q++) cand[m][q] = lmv[q];
  }
  // per edge (SPEC: wave 1, beside wave 0's candidate lines): its attributes and the current line
  // (SPEC: its candidate pose) into LDS
  const int es_ = SPEC ? tid - 64 : tid;
  if (es_ >= 0 && es_ < kLineBlk) {
    const int tid = es_;
    const bool on = tid < cnt;
    const int e = on ? (p0 + tid) : 0;
    const int t = on ? P.etype[e] : 2;
    // outside this phase: exact-zero records (setup: the level from the edge's last error)
    const bool live = on && !(SETUP ? (cls && edge_outlier(P, L, e)) : (A.elevel && A.elevel[e]));
    const bool popt = on && A.pidx[P.epose[e]] >= 0;
    einfo_s[tid][0] = e;
    einfo_s[tid][1] = t;
    einfo_s[tid][2] = (on ? 1 : 0) | (live ? 2 : 0) | (popt ? 4 : 0);
    einfo_s[tid][3] = on ? P.elm[e] : gb;
    if (live) {
      const int l = P.elm[e] - P.nq;
      if (SPEC) {
        double Tc[8];
        cand_pose(P, A, S.x, P.epose[e], failed, Tc);
#pragma unroll
        for (int k = 0; k < 8; k++) Tsh[tid][k] = Tc[k];
      } else {
        for (int k = 0; k < 6; k++) Lsh[tid][k] = P.L[6 * l + k];
      }
    }
  }
  __syncthreads();
  if (stamp && tid == 0) stamp[0] = wall_clock64();
  const double delta = 1e-9, scal = 1.0 / (2 * delta);
  {
    // this thread's evaluation: wave 0 line perturbations, waves 1-2 pose perturbations,
    // wave 3 (SPEC) the unperturbed error
    int slot = -1, m = 0;
    if (wv == 0) {
      slot = lane >> 3;
      m = lane & 7;  // ev row 2d + sign, d < 4
    } else if (wv < 3) {
      const int idx = (wv - 1) * 64 + lane;
      if (idx < 12 * kLineBlk) {
        slot = idx / 12;
        m = 8 + idx % 12;  // ev row 2d + sign, d = 4..9
      }
    } else if (OWN_ERR && lane < kLineBlk) {
      slot = lane;
      m = 20;
    }
    if (P.line_jac) {  // analytic: one lane per edge (wave 0), its error too (OWN_ERR)
      slot = (wv == 0 && lane < kLineBlk) ? lane : -1;
      m = OWN_ERR ? 20 : 21;
    }
    int e = 0, t = 2;
    bool on = false, live = false;
    if (slot >= 0) edge(slot, e, t, on, live);
    if (live && P.line_jac) {
      const SE3 T = load_T(SPEC ? &Tsh[slot][0] : P.T + 8 * P.epose[e]);
      const double* cam = P.cams + 5 * P.ecam[e];
      const double* obs = obs_of(P, e, t);
      double Lp[6];
      for (int k = 0; k < 6; k++) Lp[k] = SPEC ? cand[einfo_s[slot][3] - gb][k] : Lsh[slot][k];
      double Jp[24], Jl[16];
#pragma unroll
      for (int k = 0; k < 24; k++) Jp[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 16; k++) Jl[k] = 0.0;
      line_jac_analytic(cam, T, Lp, obs, t == 3, Jp, Jl);
      // whole rows (static indices: no scratch); rows >= edim(t) are zero and never read
#pragma unroll
      for (int k = 0; k < 16; k++) J[slot][24 + k] = Jl[k];
#pragma unroll
      for (int k = 0; k < 24; k++) J[slot][k] = Jp[k];
      if (OWN_ERR) {
        double er[4] = {0, 0, 0, 0};
        edge_error(t, cam, obs, T, Lp, er);
        for (int k = 0; k < 4; k++) es[slot][k] = er[k];
      }
    } else if (live) {
      const int d = m >> 1;
      const double sgn = (m & 1) ? -delta : delta;
      const SE3 T = load_T(SPEC ? &Tsh[slot][0] : P.T + 8 * P.epose[e]);
      const double* cam = P.cams + 5 * P.ecam[e];
      const double* obs = obs_of(P, e, t);
      double Lp[6];
      for (int k = 0; k < 6; k++) Lp[k] = SPEC ? cand[einfo_s[slot][3] - gb][k] : Lsh[slot][k];
      double er[4] = {0, 0, 0, 0};
      if (wv == 0) {
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = q == d ? sgn : 0.0;  // static indices: no scratch
        line_oplus(Lp, v);
        edge_error(t, cam, obs, T, Lp, er);
      } else if (wv < 3) {
        double u[6];
#pragma unroll
        for (int q = 0; q < 6; q++) u[q] = q == d - 4 ? sgn : 0.0;
        edge_error(t, cam, obs, se3_mul(se3_exp(u), T), Lp, er);
      } else {
        edge_error(t, cam, obs, T, Lp, er);
      }
      if (m < 20)
        for (int k = 0; k < 4; k++) ev[slot][m][k] = er[k];
      else
        for (int k = 0; k < 4; k++) es[slot][k] = er[k];
    }
  }
  __syncthreads();
  if (stamp && tid == 0) stamp[1] = wall_clock64();
  if (SETUP && tid == 0) {  // the robust cost of the block's edges at the current state, slot order
    double c = 0;
    for (int slot = 0; slot < cnt; slot++) {
      int e, t;
      bool on, live;
      edge(slot, e, t, on, live);
      if (!live) continue;
      double chi2 = 0;
      for (int k = 0; k < edim(t); k++) chi2 += es[slot][k] * es[slot][k];
      chi2 *= einfo(t);
      double cst = chi2;
      if (A.robust) {
        double r1;
        huber(chi2, pick4(P.delta, t), cst, r1);
      }
      c += cst;
    }
    *chi_out = c;
  }
  // J layout per edge: Jp [4][6] at 0, Jl [4][4] at 24 (the analytic path wrote it directly)
  // every J entry of every slot (rows >= edim(t) and slots that are not live: exact zeros), and each
  // slot's robust weight once (SPEC / SETUP: the slot's own error; else the edge's stored one)
  __shared__ double wsh[kLineBlk];
  for (int idx = tid; idx < (P.line_jac ? 0 : 40 * kLineBlk); idx += 256) {
    const int slot = idx / 40, rd = idx - 40 * slot, r = rd / 10, d = rd % 10;
    int e, t;
    bool on, live;
    edge(slot, e, t, on, live);
    const double v = (live && r < edim(t)) ? scal * (ev[slot][2 * d][r] - ev[slot][2 * d + 1][r]) : 0.0;
    if (d < 4) J[slot][24 + r * 4 + d] = v;
    else J[slot][r * 6 + (d - 4)] = v;
  }
  if (tid >= 192 && tid < 192 + kLineBlk) {
    const int slot = tid - 192;
    int e, t;
    bool on, live;
    edge(slot, e, t, on, live);
    const double* er = OWN_ERR ? &es[slot][0] : L.err + 4 * e;
    wsh[slot] = live ? edge_weight_of(P, A, er, t) : 0.0;
  }
  __syncthreads();
  // the 86 contributions per edge (contrib's layout: Hll, bl, Hpp, bp, Hpl), one kind per pass so that
  // a wave never diverges between kinds; four rows unrolled (the rows past edim(t) are zeros and add
  // exact zeros: the same sums, in the same order, as contrib()).  Hpp: the 21 upper entries stored.
  auto rowsum = [&](const double* x, int sx, const double* y, int sy) {
    double t0 = x[0], t1 = x[sx], t2 = x[2 * sx], t3 = x[3 * sx];
    double u0 = y[0], u1 = y[sy], u2 = y[2 * sy], u3 = y[3 * sy];
    double s = 0;
    s += t0 * u0;
    s += t1 * u1;
    s += t2 * u2;
    s += t3 * u3;
    return s;
  };
  auto slot_of = [&](int idx, int per, int& e, int& t, bool& live, bool& popt) {
    const int slot = idx / per;
    bool on;
    edge(slot, e, t, on, live);
    popt = (einfo_s[slot][2] & 4) != 0;
    return on ? slot : -1;
  };
  for (int idx = tid; idx < 20 * kLineBlk; idx += 256) {  // Hll (o < 16), bl
    int e, t;
    bool live, popt;
    const int slot = slot_of(idx, 20, e, t, live, popt);
    if (slot < 0) continue;
    const int o = idx - 20 * slot;
    const double* Jl = &J[slot][24];
    double v;
    if (o < 16) {
      v = live ? wsh[slot] * rowsum(Jl + o / 4, 4, Jl + o % 4, 4) : 0.0;
    } else {
      const double* er = OWN_ERR ? &es[slot][0] : L.err + 4 * e;
      double eb[4];
#pragma unroll
      for (int r = 0; r < 4; r++) eb[r] = r < edim(t) ? er[r] : 0.0;
      v = live ? -wsh[slot] * rowsum(Jl + (o - 16), 4, eb, 1) : 0.0;
    }
    cv[slot][o] = v;
    if (split)
      __hip_atomic_store(o < 16 ? L.Hll + 16 * e + o : L.bl + 4 * e + o - 16, v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  for (int idx = tid; idx < 21 * kLineBlk; idx += 256) {  // Hpp, upper triangle (pk6 order)
    int e, t;
    bool live, popt;
    const int slot = slot_of(idx, 21, e, t, live, popt);
    if (slot < 0 || !popt) continue;
    const int q = idx - 21 * slot;
    int a = 0, base = 0;
    while (q >= base + 6 - a) base += 6 - a++;
    const int b = a + (q - base);
    const double* Jp = &J[slot][0];
    L.Hpp[21 * e + q] = live ? wsh[slot] * rowsum(Jp + a, 6, Jp + b, 6) : 0.0;
  }
  for (int idx = tid; idx < 30 * kLineBlk; idx += 256) {  // bp (k < 6), Hpl (6 x 4)
    int e, t;
    bool live, popt;
    const int slot = slot_of(idx, 30, e, t, live, popt);
    if (slot < 0 || !popt) continue;
    const int k = idx - 30 * slot;
    const double* Jp = &J[slot][0];
    if (k < 6) {
      const double* er = OWN_ERR ? &es[slot][0] : L.err + 4 * e;
      double eb[4];
#pragma unroll
      for (int r = 0; r < 4; r++) eb[r] = r < edim(t) ? er[r] : 0.0;
      L.bp[6 * e + k] = live ? -wsh[slot] * rowsum(Jp + k, 6, eb, 1) : 0.0;
    } else {
      const int a = (k - 6) / 4, b = (k - 6) % 4;
      L.Hpl[hpl_off(P.Ep, e) + k - 6] = live ? wsh[slot] * rowsum(Jp + a, 6, &J[slot][24] + b, 4) : 0.0;
    }
  }
  if (SETUP && pdg)  // computeLambdaInit's pose-diagonal partials of this workgroup's edges (slot order), as
                    // the Hpp pass's diagonal entries (pose_diag_range's slots)
    for (int q = tid; q < 6 * A.K; q += 256) {
      const int j = q / 6, i = q - 6 * j;
      double sm = 0;
      for (int slot = 0; slot < cnt; slot++) {
        int e, t;
        bool on, live;
        edge(slot, e, t, on, live);
        if (!(einfo_s[slot][2] & 4) || A.pidx[P.epose[e]] != j) continue;
        const double* Jp = &J[slot][0];
        sm += live ? wsh[slot] * rowsum(Jp + i, 6, Jp + i, 6) : 0.0;
      }
      __hip_atomic_store(pdg + ((size_t)j * pd_nb + pd_b) * 6 + i, sm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  if (!split) {  // whole landmarks: their blocks from this workgroup's records, CSR (slot) order
    __syncthreads();
    if (tid < 20 * (ge - gb)) {
      const int g = gb + tid / 20, o = tid % 20;
      const int s0 = A.lm_off[g] - p0, s1 = A.lm_off[g + 1] - p0;
      if (s1 > s0) {
        double sm = 0;
        for (int q = s0; q < s1; q++) sm += cv[q][o];
        if (o < 16) S.Hll[16 * g + o] = sm;
        else S.bl[4 * g + o - 16] = sm;
        bool act = !SETUP && A.lm_act[g];
        if (SETUP)
          for (int q = s0; q < s1; q++) act = act || (einfo_s[q][2] & 2);
        if (maxd && o == 0 && act) {  // max |diagonal| of the block, as the ticket path
          double mx = 0;
          for (int dgi = 0; dgi < 16; dgi += 5) {
            double sd = 0;
            for (int q = s0; q < s1; q++) sd += cv[q][dgi];
            mx = fmax(mx, fabs(sd));
          }
          atomic_max_pos(S.out + 2, mx);
        }
      }
    }
    return;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // split landmark, per edge (32 lanes each): ticket; the last edge sums the landmark's records
  {
    const int slot = 2 * wv + (lane >> 5), ln = lane & 31;
    int e, t;
    bool on, live;
    edge(slot, e, t, on, live);
    if (on) {
      const int gl = einfo_s[slot][3], l = gl - P.nq;
      const int k0 = A.lm_off[gl], k1 = A.lm_off[gl + 1];
      unsigned tk = 0;
      if (ln == 0) tk = __hip_atomic_fetch_add(S.lm_ctr + l, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tk = __shfl(tk, lane & 32);
      if (tk == (unsigned)(k1 - k0 - 1)) {
        if (ln == 0) __hip_atomic_store(S.lm_ctr + l, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        double sm = 0;
        if (ln < 20) {
          const double* base = ln < 16 ? L.Hll + ln : L.bl + (ln - 16);
          const int str = ln < 16 ? 16 : 4;
          for (int k = k0; k < k1; k++)
            sm += __hip_atomic_load(base + (size_t)str * (k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (ln < 16) S.Hll[16 * gl + ln] = sm;
          else S.bl[4 * gl + ln - 16] = sm;
        }
        double mx = (ln < 16 && ln % 5 == 0) ? fabs(sm) : 0.0;
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
        if (maxd && ln == 0 && (SETUP ? line_active(P, L, A, gl, cls) : A.lm_act[gl] != 0)) atomic_max_pos(S.out + 2, mx);
      }
    }
  }
}

// deterministic block reduction of NV values per thread: wave shuffles, then waves in order
template <int NV>
__device__ __forceinline__ void block_reduce(double (&acc)[NV], double* lds /* [nwaves][NV] */) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    acc[i] = wave::xsum64(acc[i]);  // (the xor butterfly's sums, on lane moves)
  }
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < NV; i++) lds[wv * NV + i] = acc[i];
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0;
    for (int w = 0; w < nw; w++) s += lds[w * NV + threadIdx.x];
    lds[threadIdx.x] = s;  // result in lds[0..NV)
  }
  __syncthreads();
}

}  // namespace ba
}  // namespace rspl
