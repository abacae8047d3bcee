// Local bundle adjustment (LocalmapOptimization, src/g2o_optimization/g2o_optimization.cc:21-252)
// as an fp64 Levenberg-Marquardt on gfx950.  Same algorithm as the CPU restatement
// (oracle/ba.c, which restates the g2o pieces it relies on): SE3 left exp-map update,
// analytic point Jacobians, numeric (delta 1e-9) line Jacobians, Huber IRLS weights,
// Schur complement on marginalised points + lines, dense Cholesky of the reduced
// camera system.  Every reduction runs in a fixed order (CSR lists, fixed trees), so
// a call is bitwise reproducible.  Not a dense contraction: no MFMA; HBM/latency bound.
//
// This header: the device code every BA unit shares (ba_first.hip: first pass and bookkeeping,
// ba_schur.hip: Schur complement and solvers, ba_trial.hip: cost, update and the trial entry points) --
// edge geometry and errors, Huber, the mailbox, the device-side LM control and its banks, tickets
// and block sums.  Everything here is __device__ __forceinline__; the linearisation family is in
// ba_linearize.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "ba_kernels.hpp"
#include "se3_device.hpp"

namespace rspl {
namespace ba {

__device__ __forceinline__ double n3(const double* v) {
  #pragma clang fp contract(off)  // bit-identical to the CPU restatement (oracle/ba.c, -ffp-contract=off)
  return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  #pragma clang fp contract(off)  // bit-identical to the CPU restatement (oracle/ba.c, -ffp-contract=off)
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// g2o::Line3D::oplus (orthonormal 4-DoF update; vertex_line3d.h:26-29)
__device__ __forceinline__ void line_oplus(double* L, const double* v) {
  #pragma clang fp contract(off)  // bit-identical to the CPU restatement (oracle/ba.c, -ffp-contract=off)
  const double* w = L;
  const double* d = L + 3;
  const double mx = n3(d), my = n3(w);
  const double wn = 1.0 / sqrt(mx * mx + my * my);
  const double Wm[4] = {my * wn, -mx * wn, mx * wn, my * wn};
  const double mn = 1.0 / my, dn = 1.0 / mx;
  double mdc[3];
  cross3(w, d, mdc);
  const double mdn = 1.0 / n3(mdc);
  const double U[9] = {w[0] * mn, d[0] * dn, mdc[0] * mdn, w[1] * mn, d[1] * dn, mdc[1] * mdn,
                       w[2] * mn, d[2] * dn, mdc[2] * mdn};
  const double cs = cos(v[3]), sn = sin(v[3]);
  const double Wu[4] = {cs, -sn, sn, cs};
  double q[4] = {sqrt(1 - (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])), v[0], v[1], v[2]};
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] /= qn;
  double Uu[9];
  q_to_R(q, Uu);
  double U2[9], W2[4];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += U[i * 3 + k] * Uu[k * 3 + j];
      U2[i * 3 + j] = s;
    }
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2; j++) W2[i * 2 + j] = Wm[i * 2 + 0] * Wu[0 * 2 + j] + Wm[i * 2 + 1] * Wu[1 * 2 + j];
  double out[6];
  for (int i = 0; i < 3; i++) {
    out[i] = W2[0] * U2[i * 3 + 0];
    out[3 + i] = W2[2] * U2[i * 3 + 1];
  }
  for (int rep = 0; rep < 2; rep++) {  // fromOrthonormal normalises, oplus normalises again
    const double s = 1.0 / n3(out + 3);
    for (int i = 0; i < 6; i++) out[i] *= s;
  }
  for (int i = 0; i < 6; i++) L[i] = out[i];
}

__device__ __forceinline__ SE3 load_T(const double* T) {
  SE3 r;
  for (int i = 0; i < 4; i++) r.q[i] = T[i];
  for (int i = 0; i < 3; i++) r.t[i] = T[4 + i];
  return r;
}

// Edge residual for pose estimate T and landmark values lm (point [3] or line [6]).
__device__ __forceinline__ void edge_error(int type, const double* cam, const double* obs, const SE3& T, const double* lm, double (&e)[4]) {
  #pragma clang fp contract(off)  // bit-identical to the CPU restatement (oracle/ba.c, -ffp-contract=off)
  double R[9];
  q_to_R(T.q, R);
  if (type < 2) {  // EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ: e = obs - proj(T p)
    double Xc[3];
    mat3_vec(R, lm, Xc);
    for (int i = 0; i < 3; i++) Xc[i] += T.t[i];
    const double iz = 1.0 / Xc[2];
    const double u = cam[0] * Xc[0] * iz + cam[2];
    const double v = cam[1] * Xc[1] * iz + cam[3];
    e[0] = obs[0] - u;
    e[1] = obs[1] - v;
    if (type == 1) e[2] = obs[2] - (u - cam[4] * iz);
    return;
  }
  // EdgeSE3ProjectLine / EdgeStereoSE3ProjectLine (edge_project_line.cc:21-42, edge_project_stereo_line.cc:22-51)
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
  const double Kv0 = -fy * cx, Kv1 = -fx * cy, Kv2 = fx * fy;
  // both sides spelled out (every index of e / obs static: no scratch)
  auto side_err = [&](double tx0, const double* o, double& ea, double& eb) {
    const double t[3] = {tx0, T.t[1], T.t[2]};
    double Rw[3], Rd[3], tx[3];
    mat3_vec(R, lm, Rw);
    mat3_vec(R, lm + 3, Rd);
    cross3(t, Rd, tx);
    const double w0 = Rw[0] + tx[0], w1 = Rw[1] + tx[1], w2 = Rw[2] + tx[2];
    const double l0 = fy * w0, l1 = fx * w1, l2 = Kv0 * w0 + Kv1 * w1 + Kv2 * w2;
    const double nrm = sqrt(l0 * l0 + l1 * l1);
    ea = (o[0] * l0 + o[1] * l1 + l2) / nrm;
    eb = (o[2] * l0 + o[3] * l1 + l2) / nrm;
  };
  side_err(T.t[0], obs, e[0], e[1]);
  if (type == 3) side_err(T.t[0] - cam[4] / fx, obs + 4, e[2], e[3]);  // T_right(0,3) -= b, b = bf / fx
}

// Line-edge Jacobians, analytic (Problem::line_jac = 1): the delta -> 0 limit of g2o's central difference
// (truncation O(delta^2) ~ 1e-18 relative at delta 1e-9; the central difference itself carries ~1e-7 relative
// cancellation noise).  The same derivation and operation order as oracle/ba.c line_jac_analytic (FP
// contraction off: bit-identical to it): pose d wc / d omega = -[wc]x (+ [b]x [c]x on the right camera of a
// stereo edge, c = (bf / fx, 0, 0)), d wc / d upsilon = -[b]x with b = R d; line (Line3D::oplus at 0 after
// its |d| = 1 normalisation) d w / dv = [0, -2 rho u3, 2 rho u2, -(1 + rho^2) u1], d d / dv = [2 u3, 0, -2 u1, 0];
// error e_k = (o_k . l01 + l2) / |l01|, l = [fy wc0, fx wc1, Kv . wc].  Jp [4][6], Jl [4][4] (rows 2 / 4).
__device__ __forceinline__ void skew3(const double* v, double* S) {
  S[0] = 0; S[1] = -v[2]; S[2] = v[1];
  S[3] = v[2]; S[4] = 0; S[5] = -v[0];
  S[6] = -v[1]; S[7] = v[0]; S[8] = 0;
}

__device__ __forceinline__ void line_jac_analytic(const double* cam, const SE3& T, const double* L, const double* obs,
                                                  bool stereo, double* Jp, double* Jl) {
  #pragma clang fp contract(off)  // bit-identical to the CPU restatement (oracle/ba.c, -ffp-contract=off)
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], bf = cam[4];
  const double M[9] = {fy, 0, 0, 0, fx, 0, -fy * cx, -fx * cy, fx * fy};
  const double dn = n3(L + 3), wn = n3(L);
  double w[3], d[3], u1[3], u3[3], wxd[3];
  for (int i = 0; i < 3; i++) {
    w[i] = L[i] / dn;
    d[i] = L[3 + i] / dn;
    u1[i] = L[i] / wn;
  }
  cross3(L, L + 3, wxd);
  const double cn = n3(wxd);
  for (int i = 0; i < 3; i++) u3[i] = wxd[i] / cn;
  const double rho = wn / dn;
  double dw[4][3], dd[4][3];
  for (int i = 0; i < 3; i++) {
    dw[0][i] = 0;                dd[0][i] = 2 * u3[i];
    dw[1][i] = -2 * rho * u3[i]; dd[1][i] = 0;
    dw[2][i] = 2 * rho * d[i];   dd[2][i] = -2 * u1[i];
    dw[3][i] = -(1 + rho * rho) * u1[i]; dd[3][i] = 0;
  }
  double R[9], a[3], bb[3], Sb[9];
  q_to_R(T.q, R);
  mat3_vec(R, w, a);
  mat3_vec(R, d, bb);
  skew3(bb, Sb);
  for (int side = 0; side < (stereo ? 2 : 1); side++) {
    double t[3] = {T.t[0], T.t[1], T.t[2]};
    const double c[3] = {side == 1 ? bf / fx : 0.0, 0.0, 0.0};
    t[0] -= c[0];
    double txb[3], wc[3];
    cross3(t, bb, txb);
    for (int i = 0; i < 3; i++) wc[i] = a[i] + txb[i];
    double l[3];
    mat3_vec(M, wc, l);
    const double n = sqrt(l[0] * l[0] + l[1] * l[1]);
    double Sw[9], Sc[9], BC[9];
    skew3(wc, Sw);
    skew3(c, Sc);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += Sb[i * 3 + k] * Sc[k * 3 + j];
        BC[i * 3 + j] = s;
      }
    double Gp[3][6], Gl[3][4];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        Gp[i][j] = -Sw[i * 3 + j] + BC[i * 3 + j];
        Gp[i][3 + j] = -Sb[i * 3 + j];
      }
    for (int k = 0; k < 4; k++) {
      double Rw[3], Rd[3], tx[3];
      mat3_vec(R, dw[k], Rw);
      mat3_vec(R, dd[k], Rd);
      cross3(t, Rd, tx);
      for (int i = 0; i < 3; i++) Gl[i][k] = Rw[i] + tx[i];
    }
    for (int ep = 0; ep < 2; ep++) {
      const double* o = obs + 4 * side + 2 * ep;
      const double num = o[0] * l[0] + o[1] * l[1] + l[2];
      const double de_dl[3] = {o[0] / n - num * l[0] / (n * n * n), o[1] / n - num * l[1] / (n * n * n), 1.0 / n};
      double de_dwc[3];
      for (int j = 0; j < 3; j++) de_dwc[j] = de_dl[0] * M[0 * 3 + j] + de_dl[1] * M[1 * 3 + j] + de_dl[2] * M[2 * 3 + j];
      const int r = 2 * side + ep;
      for (int j = 0; j < 6; j++) Jp[r * 6 + j] = de_dwc[0] * Gp[0][j] + de_dwc[1] * Gp[1][j] + de_dwc[2] * Gp[2][j];
      for (int k = 0; k < 4; k++) Jl[r * 4 + k] = de_dwc[0] * Gl[0][k] + de_dwc[1] * Gl[1][k] + de_dwc[2] * Gl[2][k];
    }
  }
}

// a per-type constant of the kernel-argument structs with a select chain: a dynamic index would
// copy the whole by-value struct to scratch
__device__ __forceinline__ double pick4(const double (&a)[4], int t) {
  return t == 0 ? a[0] : t == 1 ? a[1] : t == 2 ? a[2] : a[3];
}

// per-edge Hpp records keep the upper triangle (21 doubles, row-major): the blocks are exactly
// symmetric (the same products summed in the same order for (a, b) and (b, a))
__host__ __device__ constexpr int pk6(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

// Hpl records: a point edge (positions [0, Ep)) 6 x 3 at 18 e (row stride 3), a line edge 6 x 4 at
// 18 Ep + 24 (e - Ep) (row stride 4) -- a point record carries no zero column (144 instead of 192 bytes,
// written once and read by the Schur chunks and the next update per trial)
__device__ __forceinline__ int hpl_off(int Ep, int e) { return e < Ep ? 18 * e : 18 * Ep + 24 * (e - Ep); }
// edge e's record as 6 x 4 (column 3 zero for a point edge); every load at a valid address, then selected
__device__ __forceinline__ void load_hpl4(const double* H, int Ep, int e, double (&B)[24]) {
  const int o = hpl_off(Ep, e), st = e < Ep ? 3 : 4;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const double v = H[o + r * st + (c < st ? c : st - 1)];
      B[r * 4 + c] = c < st ? v : 0.0;
    }
}

__device__ __forceinline__ int edim(int t) { return t == 0 ? 2 : t == 1 ? 3 : t == 2 ? 2 : 4; }

// point edges only (t < 2), every index static: edge_error's point branch and its chi2 (info I)
__device__ __forceinline__ double point_error_R(int t, const double* cam, const double* obs, const double (&R)[9],
                                                const double* tt, const double* X, double (&e)[4]) {
  double Xc[3];
  mat3_vec(R, X, Xc);
  for (int i = 0; i < 3; i++) Xc[i] += tt[i];
  const double iz = 1.0 / Xc[2];
  const double u = cam[0] * Xc[0] * iz + cam[2];
  const double v = cam[1] * Xc[1] * iz + cam[3];
  e[0] = obs[0] - u;
  e[1] = obs[1] - v;
  e[2] = t == 1 ? obs[2] - (u - cam[4] * iz) : 0.0;
  e[3] = 0.0;
  double chi2 = 0;
  chi2 += e[0] * e[0];
  chi2 += e[1] * e[1];
  if (t == 1) chi2 += e[2] * e[2];
  return chi2 * 1.0;
}
__device__ __forceinline__ double point_error(int t, const double* cam, const double* obs, const SE3& T,
                                              const double* X, double (&e)[4]) {
  double R[9];
  q_to_R(T.q, R);
  return point_error_R(t, cam, obs, R, T.t, X, e);
}

// edge e's observation (type t): point edges [0, Ep) at stride 4 (u, v, u_r), line edges [Ep, E)
// at stride 8 after them (edges are in landmark-CSR order: point landmarks first)
__device__ __forceinline__ const double* obs_of(const Problem& P, int e, int t) {
  return t < 2 ? P.eobs + 4 * e : P.eobs + 4 * P.Ep + 8 * (e - P.Ep);
}

__device__ __forceinline__ double einfo(int t) { return t < 2 ? 1.0 : 0.1; }

__device__ __forceinline__ const double* lm_ptr(const Problem& P, int g) {
  return g < P.nq ? P.X + 3 * g : P.L + 6 * (g - P.nq);
}

// Huber (RobustKernelHuber::robustify): rho0, rho1
__device__ __forceinline__ void huber(double e2, double delta, double& r0, double& r1) {
  const double dsqr = delta * delta;
  if (e2 <= dsqr) {
    r0 = e2;
    r1 = 1.0;
  } else {
    const double s = sqrt(e2);
    r0 = 2 * s * delta - dsqr;
    r1 = delta / s;
  }
}

// Mailbox post into fine-grained (uncached) host memory: the four values, then -- once they
// have completed (vmcnt) -- the sequence number the host spins on.  No release fence: a
// system/agent-scope release writes back the whole L2 (~3.5 us, MI355X_MICROARCH.md), once per
// LM trial on the critical path; the host reads only these uncached words.
__device__ __forceinline__ void post_mail(Mail* m, double v0, double v1, double v2, double v3, unsigned long long seq) {
  // vseq first (a reader that sees it change knows v is being rewritten), then v, then seq
  __hip_atomic_store(&m->vseq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(&m->v[0], v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->v[1], v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->v[2], v2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->v[3], v3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(&m->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- device-side LM control (Sys::lm) ----
// Trial entry: false when the optimize() has already stopped (this trial is a no-op); else the
// damping, the current bank and whether the candidate's speculative linearisation is wanted
// (not in the last iteration).  Uniform scalar loads; the control was written by the previous
// trial's last kernel (kernel boundary = visibility).
struct LmView {
  double lambda;
  int cur, spec;
};
__device__ __forceinline__ bool lm_view(const Sys& S, LmView& v) {
  const LmCtrl* c = S.lm + S.lm_slot;
  if (c->stop) return false;
  v.lambda = c->lambda;
  v.cur = c->cur;
  v.spec = c->it + 1 < c->iters;
  return true;
}
template <typename T>
__device__ __forceinline__ void swp(T& a, T& b) {
  T t = a;
  a = b;
  b = t;
}
// bank 1 current: the host's candidate state / spare records are the current ones
__device__ __forceinline__ void bank_state(Problem& P) {
  swp(P.T, P.Tn);
  swp(P.X, P.Xn);
  swp(P.L, P.Ln);
}
__device__ __forceinline__ void bank_lin(Lin& L, Lin& Ls, Sys& S, Sys& Ss) {
  swp(L.Hpp, Ls.Hpp);
  swp(L.bp, Ls.bp);
  swp(L.Hll, Ls.Hll);
  swp(L.bl, Ls.bl);
  swp(L.Hpl, Ls.Hpl);
  swp(S.Hll, Ss.Hll);
  swp(S.bl, Ss.bl);
}
// Last-block ticket: this block's partials were stored device-coherent (relaxed agent-scope
// atomics, written through), so completing them (vmcnt) before a relaxed ticket increment is
// enough -- an acq_rel ticket would write back and invalidate the L2 in every block.
__device__ __forceinline__ unsigned ticket(unsigned* counter) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double block_sum256(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ void prof_stamp(const Sys& S, int slot) {
  if (S.prof) S.prof[slot] = wall_clock64();
}

}  // namespace ba
}  // namespace rspl
