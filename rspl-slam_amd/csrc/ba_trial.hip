// Local BA (see ba_device.hpp), the tail of an LM trial and the trial entry points: back-substitution and
// candidate state, the candidate's cost (and, fused, its speculative linearisation and the device-side LM
// decision), and the host functions that queue one trial for each driver of ba.cpp.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "ba_kernels.hpp"
#include "ba_launch.hpp"
#include "ba_linearize.hpp"

namespace rspl {
namespace ba {

// One trial's verdict, g2o OptimizationAlgorithmLevenberg::solve as restated by ba.cpp optimize_host()
// (g2o_optimization.cc:172-210 runs optimize(10) / optimize(5)): rho test with the LM scale,
// damping update (accept: lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), ni = 2; reject:
// lambda *= ni, ni *= 2), at most 10 trials per iteration, stop at qmax == 10 or rho == 0.
// Returns 1 when the optimize() is finished.
__device__ int lm_decide(const LmCtrl* c, LmCtrl* n, double chi2, double scale, double fail) {
  const bool ok = fail == 0.0;
  const double tempChi = ok ? chi2 : DBL_MAX;
  double rho = c->chi - tempChi;
  rho /= ok ? scale + 1e-3 : 1.0;
  double lambda = c->lambda, ni = c->ni;
  int qmax = c->qmax, it = c->it;
  bool brk = false;
  *n = *c;
  if (rho > 0 && isfinite(tempChi) && ok) {
    double alpha = 1. - cube(2 * rho - 1);  // pow(2 rho - 1, 3)
    alpha = fmin(alpha, 2. / 3.);
    lambda *= fmax(1. / 3., alpha);
    ni = 2;
    n->chi = tempChi;
    n->cur = c->cur ^ 1;
  } else {
    lambda *= ni;
    ni *= 2;
    brk = !isfinite(lambda);
  }
  if (!brk) qmax++;
  int stop = 0;
  if (brk || !(rho < 0 && qmax < 10)) {  // the iteration ends
    it++;
    if (qmax == 10 || rho == 0 || !isfinite(lambda) || it >= c->iters) stop = 1;
    else qmax = 0;
  }
  n->lambda = lambda;
  n->ni = ni;
  n->qmax = qmax;
  n->it = it;
  n->trials = c->trials + 1;
  n->stop = stop;
  return stop;
}

// ---------------------------------------------------------------------------
// errors + robust chi2 per active edge.  The last block to finish (ticket counter)
// sums the block partials -- and the update kernel's scale partials -- in a fixed
// order, posts {chi2, scale, maxdiag, fail} + seq to the host-mapped mailbox and
// re-arms the device state (counter, fail flag, maxdiag) for the next trial.
// (In this unit with update_kernel: the two share block_sum256, and compiled apart each
// gets a differently scheduled last reduction step.)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void errors_kernel(Problem P, Lin L, Active A, Sys S, int nb_scale,
                                                     unsigned long long seq) {
  __shared__ double red[256];
  __shared__ int last;
  const int i = blockIdx.x * 256 + threadIdx.x;
  double c = 0.0;
  if (i < A.Ea && (!A.elevel || !A.elevel[i])) {
    const int e = i;
    const int t = P.etype[e];
    const SE3 T = load_T(P.T + 8 * P.epose[e]);
    double er[4] = {0, 0, 0, 0};
    edge_error(t, P.cams + 5 * P.ecam[e], obs_of(P, e, t), T, lm_ptr(P, P.elm[e]), er);
    double chi2 = 0;
    for (int k = 0; k < edim(t); k++) chi2 += er[k] * er[k];
    chi2 *= einfo(t);
    for (int k = 0; k < 4; k++) L.err[4 * e + k] = er[k];
    if (A.robust) {
      double r1;
      huber(chi2, pick4(P.delta, t), c, r1);
    } else {
      c = chi2;
    }
  }
  const double bsum = block_sum256(c, red);
  if (threadIdx.x == 0) {
    __hip_atomic_store(S.partial + blockIdx.x, bsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned tk = ticket(S.counter);
    last = tk == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  double c2 = 0, sc = 0;
  for (int k = threadIdx.x; k < (int)gridDim.x; k += 256)
    c2 += __hip_atomic_load(S.partial + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int k = threadIdx.x; k < nb_scale; k += 256) sc += S.partial2[k];
  const double chi2 = block_sum256(c2, red);
  const double scale = block_sum256(sc, red);
  if (threadIdx.x == 0) {
    const double f = (double)__hip_atomic_load(S.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double mx = S.out[2];
    S.out[0] = chi2;
    S.out[1] = scale;
    S.out[3] = f;
    if (S.shard_out) {  // sharded: this rank's share goes to the all-reduce, shard_post posts
      S.shard_out[0] = chi2;
      S.shard_out[1] = scale;
      S.shard_out[2] = f;
      __hip_atomic_store(S.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(S.fail, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      S.out[2] = 0.0;
      return;
    }
    __hip_atomic_store(S.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(S.fail, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    S.out[2] = 0.0;
    if (seq) post_mail(S.mail, chi2, scale, mx, f, seq);  // seq 0: nobody waits (device-side LM)
  }
}

// Back-substitution xl = Dinv (bl - sum_e Hpl_e^T xp) fused with the candidate state
// (poses T <- exp(xp) T, points += xl, lines oplus(xl); inactive vertices copied: ping-pong
// buffers) and the LM scale x.(lambda x + b) per block.
__global__ __launch_bounds__(256) void update_kernel(Problem P, Lin L, Active A, Sys S, double lambda) {
  __shared__ double red[256];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool failed = *S.fail != 0;
  double sc = 0;
  if (i < P.np) {
    const double* Tp = P.T + 8 * i;
    double* Tq = P.Tn + 8 * i;
    const int a = A.pidx[i];
    if (a >= 0 && !failed) {
      const double* xp = S.x + 6 * a;
      const SE3 r = se3_mul(se3_exp(xp), load_T(Tp));
      for (int k = 0; k < 4; k++) Tq[k] = r.q[k];
      for (int k = 0; k < 3; k++) Tq[4 + k] = r.t[k];
      Tq[7] = 0;
      if (S.pose_scale)
        for (int k = 0; k < 6; k++) sc += xp[k] * (lambda * xp[k] + S.bp[6 * a + k]);
    } else {
      for (int k = 0; k < 8; k++) Tq[k] = Tp[k];
    }
  } else if (i < P.np + P.nq + P.nl) {
    const int g = i - P.np;
    const bool point = g < P.nq;
    const bool upd = A.lm_act[g] && !failed;
    double xl[4] = {0, 0, 0, 0};
    if (upd) {
      double c[4];
      for (int k = 0; k < 4; k++) c[k] = S.bl[4 * g + k];
      const int k0 = A.lm_off[g], k1 = A.lm_off[g + 1];
      for (int kb = k0; kb < k1; kb += 4) {
        int es[4], as[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int k = min(kb + u, k1 - 1);
          es[u] = (k);
          as[u] = kb + u < k1 ? A.lm_pose[k] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          double B[24];
          load_hpl4(L.Hpl, P.Ep, es[u], B);
          const double* xp = S.x + 6 * max(as[u], 0);
#pragma unroll
          for (int j = 0; j < 4; j++) {
            double s = 0;
#pragma unroll
            for (int r = 0; r < 6; r++) s += B[r * 4 + j] * xp[r];
            c[j] -= as[u] >= 0 ? s : 0.0;
          }
        }
      }
      double D[16];
      if (!lm_dinv(S.Hll + 16 * g, point, lambda, D)) atomicOr(S.fail, 1);
#pragma unroll
      for (int r = 0; r < 4; r++) xl[r] = D[r * 4] * c[0] + D[r * 4 + 1] * c[1] + D[r * 4 + 2] * c[2] + D[r * 4 + 3] * c[3];
#pragma unroll
      for (int k = 0; k < 4; k++) sc += xl[k] * (lambda * xl[k] + S.bl[4 * g + k]);
    }
    if (point) {
      for (int k = 0; k < 3; k++) P.Xn[3 * g + k] = P.X[3 * g + k] + xl[k];
    } else {
      const int l = g - P.nq;
      double Lv[6];
      for (int k = 0; k < 6; k++) Lv[k] = P.L[6 * l + k];
      if (upd) line_oplus(Lv, xl);
      for (int k = 0; k < 6; k++) P.Ln[6 * l + k] = Lv[k];
    }
  }
  const double s = block_sum256(sc, red);
  if (threadIdx.x == 0) S.partial2[blockIdx.x] = s;
}

// Fast-path trial tail (after schur_solve has written the candidate poses and the pose
// part of the scale): per landmark a group of kGroup lanes does the back-substitution
// xl = Dinv (bl - sum_e Hpl_e^T xp) (edges split over the lanes, group sum), the candidate
// landmark (points += xl, lines oplus; copied when inactive: ping-pong), the scale term, and
// then the robust cost of the landmark's edges against the candidate poses.  The last block
// (ticket) sums the block partials in order and posts {chi2, scale, maxdiag, fail} + seq.
// Spec: the speculative linearisation of the candidate fused into update_errors_kernel
// (records into the spare set Ls / Ss).  Blocks [0, nbu) are the landmark groups: besides the
// update and the errors, a point group linearises its landmark's edges at the candidate from
// the errors in its registers, and a line group writes the candidate line.  Blocks [nbu, ...) are
// line-edge workgroups (lin_lines<kLinSpec>) that form their landmarks' candidates themselves, so
// they run from the kernel's start.  The mailbox ticket counts only the group blocks, so the
// host decides while the line workgroups still run.
template <bool SPEC>
__global__ __launch_bounds__(256) void update_errors_kernel(Problem P, Lin L, Active A, Sys S, double lambda,
                                                            unsigned long long seq, Lin Ls, Sys Ss, int nbu) {
  __shared__ double red[4 * 2];
  __shared__ int last;
  const bool stamp = threadIdx.x == 0 && blockIdx.x < 4096;
  if (stamp) prof_stamp(S, kProfUe + 4 * blockIdx.x);
  bool spec = SPEC;  // the candidate's speculative linearisation (device LM: not in the last iteration)
  if (SPEC && (int)blockIdx.x >= nbu) {  // line workgroups
    if (S.lm) {
      LmView v;
      if (!lm_view(S, v)) return;
      lambda = v.lambda;
      spec = v.spec;
      if (v.cur) {
        bank_state(P);
        bank_lin(L, Ls, S, Ss);
      }
    }
    if (!spec) return;
    lin_lines<kLinSpec>(P, Ls, A, Ss, blockIdx.x - nbu, false, &L, &S, lambda, *S.fail != 0,
                    S.prof ? S.prof + kProfUe + 4 * blockIdx.x + 1 : nullptr);
    if (stamp) prof_stamp(S, kProfUe + 4 * blockIdx.x + 3);
    return;
  }
  if (!SPEC) nbu = gridDim.x;
  // the candidate poses, cameras and pose steps of this trial go to LDS once per block, in the same
  // round trip as each group's landmark-only operands; the group's first edge per lane is fetched
  // in the next (every later access to them is LDS or registers: two dependent round trips).  The
  // landmark-only operands of BOTH banks are requested before the LM control is read (the control
  // picks the current bank), so that read is not a round trip of its own.
  __shared__ double sT[64 * 8], scam[16 * 5], sx[6 * 32];
  const int tid = threadIdx.x;
  // kUeWaves of the 4 waves carry landmark groups: fewer landmarks per workgroup spread the groups over
  // more CUs (the others only stage the block's poses and take part in the barriers)
  // the landmark block: with A.ue_bpr the workgroups of Schur chunk range lb (its lmchunk landmarks) go to
  // the XCD that ran the range's chunks (lb % 8, chunk_seg): their records are in that XCD's L2
  int ub = blockIdx.x;
  if (SPEC && A.ue_bpr > 0) {
    const int b = blockIdx.x, x = b & 7, sl = b >> 3, r = sl / A.ue_bpr, lb = 8 * r + x;
    constexpr int per = 64 * kUeWaves / kGroup;  // landmarks per workgroup (as set_update_geometry)
    ub = lb < A.nchk ? lb * A.ue_bpr + (sl - r * A.ue_bpr) : (A.nL + per - 1) / per + 1;  // (else: no landmark)
  }
  const int t = ub * (64 * kUeWaves) + tid, g = t / kGroup, j = t % kGroup;
  const bool in = tid < 64 * kUeWaves && g < A.nL;
  const bool point = g < P.nq;
  int k0 = 0, k1 = 0;
  bool act = false;
  double dl[16], blg[4], lm[6] = {0, 0, 0, 0, 0, 0};  // dl: Hll of the landmark (inverted below)
  double dl2[16], blg2[4], lm2[6] = {0, 0, 0, 0, 0, 0};  // the other bank's
#pragma unroll
  for (int q = 0; q < 16; q++) dl[q] = dl2[q] = 0.0;
#pragma unroll
  for (int q = 0; q < 4; q++) blg[q] = blg2[q] = 0.0;
  if (in) {
    k0 = A.lm_off[g];
    k1 = A.lm_off[g + 1];
    act = A.lm_act[g] != 0;
#pragma unroll
    for (int q = 0; q < 16; q++) {
      dl[q] = point && q >= 9 ? 0.0 : S.Hll[16 * g + q];
      dl2[q] = point && q >= 9 ? 0.0 : Ss.Hll[16 * g + q];
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      blg[q] = S.bl[4 * g + q];
      blg2[q] = Ss.bl[4 * g + q];
    }
    if (point) {
#pragma unroll
      for (int q = 0; q < 3; q++) {
        lm[q] = P.X[3 * g + q];
        lm2[q] = P.Xn[3 * g + q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < 6; q++) {
        lm[q] = P.L[6 * (g - P.nq) + q];
        lm2[q] = P.Ln[6 * (g - P.nq) + q];
      }
    }
  }
  if (S.lm) {
    LmView v;
    if (!lm_view(S, v)) {  // stopped: carry the control over to the next trial's slot
      if (blockIdx.x == 0 && threadIdx.x == 0) S.lm[S.lm_slot ^ 1] = S.lm[S.lm_slot];
      return;
    }
    lambda = v.lambda;
    spec = SPEC && v.spec;
    if (v.cur) {
      bank_state(P);
      bank_lin(L, Ls, S, Ss);
#pragma unroll
      for (int q = 0; q < 16; q++) dl[q] = dl2[q];
#pragma unroll
      for (int q = 0; q < 4; q++) blg[q] = blg2[q];
#pragma unroll
      for (int q = 0; q < 6; q++) lm[q] = lm2[q];
    }
  }
  const bool failed = *S.fail != 0;
  for (int q = tid; q < 5 * P.ncam; q += 256) scam[q] = P.cams[q];
  for (int q = tid; q < 6 * A.K; q += 256) sx[q] = S.x[q];
  // the lane's first edge (most landmarks have <= kGroup edges): everything it needs in one round trip
  const int kf = k0 + j;
  const bool has = in && kf < k1;
  int af = -1, tf = 0, pf = 0, cf = 0, lvf = 0;
  double Bf[24], of[8];
  if (has) {
    af = A.lm_pose[kf];
    tf = P.etype[kf];
    pf = P.epose[kf];
    cf = P.ecam[kf];
    lvf = A.elevel ? A.elevel[kf] : 0;
    load_hpl4(L.Hpl, P.Ep, kf, Bf);
    const double* o = obs_of(P, kf, point ? 0 : 2);
#pragma unroll
    for (int q = 0; q < 8; q++) of[q] = (q < 3 || !point) ? o[q] : 0.0;
  }
  // the candidate poses (np <= 64) while the first edges are in flight; block 0 publishes them
  // for the verdict and the next trial
  if (tid < P.np) {
    double Tc[8];
    cand_pose(P, A, S.x, tid, failed, Tc);
#pragma unroll
    for (int k = 0; k < 8; k++) sT[8 * tid + k] = Tc[k];
    if (blockIdx.x == 0)
#pragma unroll
      for (int k = 0; k < 8; k++) P.Tn[8 * tid + k] = Tc[k];
  }
  __syncthreads();
  if (stamp) prof_stamp(S, kProfUe + 4 * blockIdx.x + 1);  // operands loaded
  const bool upd = in && act && !failed;
  // back-substitution xl = Dinv (bl - sum_e Hpl_e^T xp): the first edge from registers, any later
  // ones (landmarks with more than kGroup edges) from memory
  double c[4] = {0, 0, 0, 0};
  if (upd) {
    if (has && af >= 0) {
      const double* xp = sx + 6 * af;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        double s = 0;
#pragma unroll
        for (int r = 0; r < 6; r++) s += Bf[r * 4 + q] * xp[r];
        c[q] -= s;
      }
    }
    for (int k = kf + kGroup; k < k1; k += kGroup) {
      const int a = A.lm_pose[k];
      if (a < 0) continue;
      double B[24];
      load_hpl4(L.Hpl, P.Ep, k, B);
      const double* xp = sx + 6 * a;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        double s = 0;
#pragma unroll
        for (int r = 0; r < 6; r++) s += B[r * 4 + q] * xp[r];
        c[q] -= s;
      }
    }
  }
  group_sum(c);
  double xl[4] = {0, 0, 0, 0};
  double sc = 0, chi = 0;
  if (upd) {
#pragma unroll
    for (int q = 0; q < 4; q++) c[q] += blg[q];
    {
      double D[16];
      if (!lm_dinv(dl, point, lambda, D) && j == 0) atomicOr(S.fail, 1);
#pragma unroll
      for (int q = 0; q < 16; q++) dl[q] = point ? (q < 9 ? D[4 * (q / 3) + q % 3] : 0.0) : D[q];
    }
    if (point) {
#pragma unroll
      for (int r = 0; r < 3; r++) xl[r] = dl[r * 3] * c[0] + dl[r * 3 + 1] * c[1] + dl[r * 3 + 2] * c[2];
    } else {
#pragma unroll
      for (int r = 0; r < 4; r++)
        xl[r] = dl[r * 4] * c[0] + dl[r * 4 + 1] * c[1] + dl[r * 4 + 2] * c[2] + dl[r * 4 + 3] * c[3];
    }
    if (j == 0)
#pragma unroll
      for (int q = 0; q < 4; q++) sc += xl[q] * (lambda * xl[q] + blg[q]);
  }
  const bool lin_pts = SPEC && spec && in && point;  // linearise the point edges at the candidate
  double hl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0};
  if (in) {
    if (point) {
#pragma unroll
      for (int q = 0; q < 3; q++) lm[q] += xl[q];
      if (j == 0)
#pragma unroll
        for (int q = 0; q < 3; q++) P.Xn[3 * g + q] = lm[q];
    } else {
      const int l = g - P.nq;
      if (upd) line_oplus(lm, xl);
      if (j == 0)
#pragma unroll
        for (int q = 0; q < 6; q++) P.Ln[6 * l + q] = lm[q];
    }
    // robust cost of the landmark's edges at the candidate (+ the point edges' linearisation)
    auto edge_cost = [&](int k, int te, int pose, int cam, int lev, const double (&ob)[8], int a) {
      if (lev) {
        if (lin_pts && a >= 0) zero_pose_records<false>(Ls, k);
        return;
      }
      const SE3 T = load_T(sT + 8 * pose);
      const double* cm = scam + 5 * cam;
      double er[4] = {0, 0, 0, 0};
      double chi2;
      if (point) {
        chi2 = point_error(te, cm, ob, T, lm, er);
      } else {
        edge_error(te, cm, ob, T, lm, er);
        chi2 = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (q < edim(te)) chi2 += er[q] * er[q];
        chi2 *= einfo(te);
      }
#pragma unroll
      for (int q = 0; q < 4; q++) L.err[4 * k + q] = er[q];
      double cst = chi2;
      if (A.robust) {
        double r1;
        huber(chi2, pick4(P.delta, te), cst, r1);
      }
      chi += cst;
      if (lin_pts) point_edge_core<false>(P, Ls, A, k, te, a >= 0, T, cm, lm, er, hl, bv);
    };
    if (has) edge_cost(kf, tf, pf, cf, lvf, of, af);
    for (int k = kf + kGroup; k < k1; k += kGroup) {
      const int te = P.etype[k];
      const double* o = obs_of(P, k, te);
      double ob[8];
#pragma unroll
      for (int q = 0; q < 8; q++) ob[q] = (q < 3 || !point) ? o[q] : 0.0;
      edge_cost(k, te, P.epose[k], P.ecam[k], A.elevel ? A.elevel[k] : 0, ob, A.lm_pose[k]);
    }
  }
  if (SPEC && spec) {  // point landmarks: the landmark blocks of the candidate's linearisation
    group_sum(hl);
    group_sum(bv);
    if (in && point && j == 0 && act) {
      double* H = Ss.Hll + 16 * g;
#pragma unroll
      for (int i = 0; i < 9; i++) H[i] = hl[i];
#pragma unroll
      for (int i = 9; i < 16; i++) H[i] = 0.0;
#pragma unroll
      for (int i = 0; i < 3; i++) Ss.bl[4 * g + i] = bv[i];
      Ss.bl[4 * g + 3] = 0.0;
    }
  }
  if (stamp) prof_stamp(S, kProfUe + 4 * blockIdx.x + 2);
  double acc[2] = {chi, sc};
  block_reduce<2>(acc, red);
  if (threadIdx.x == 0) {
    __hip_atomic_store(S.partial + blockIdx.x, red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(S.partial2 + blockIdx.x, red[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned tk = ticket(S.counter);
    last = tk == (unsigned)nbu - 1;
  }
  __syncthreads();
  if (stamp) prof_stamp(S, kProfUe + 4 * blockIdx.x + 3);
  if (!last) return;
  double f2[2] = {0, 0};
  for (int k = threadIdx.x; k < nbu; k += 256) {
    f2[0] += __hip_atomic_load(S.partial + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    f2[1] += __hip_atomic_load(S.partial2 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  block_reduce<2>(f2, red);
  if (threadIdx.x == 0) {
    const double chi2 = red[0], scale = red[1] + S.out[4];
    const double f = (double)__hip_atomic_load(S.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double mx = S.out[2];
    S.out[0] = chi2;
    S.out[1] = scale;
    S.out[3] = f;
    if (S.shard_out) {  // sharded: landmark part only; shard_post adds the pose part S.out[4] once
      S.shard_out[0] = chi2;
      S.shard_out[1] = red[1];
      S.shard_out[2] = f;
      __hip_atomic_store(S.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(S.fail, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      S.out[2] = 0.0;
      return;
    }
    __hip_atomic_store(S.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(S.fail, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    S.out[2] = 0.0;
    if (S.lm) {  // device-side LM: decide here; the host reads the outcome only at the end
      LmCtrl* c = S.lm + (S.lm_slot ^ 1);
      const double lam0 = S.lm[S.lm_slot].lambda, chi0 = S.lm[S.lm_slot].chi;
      const int stop = lm_decide(S.lm + S.lm_slot, c, chi2, scale, f);
      if (S.lm_trace && c->trials <= 64) {
        double* t = S.lm_trace + 8 * (c->trials - 1);
        t[0] = chi2; t[1] = scale; t[2] = f; t[3] = lam0; t[4] = chi0; t[5] = c->cur; t[6] = c->it; t[7] = c->qmax;
      }
      // system-scope stores into host memory, each waited for: only when the host reads them
      if (stop || S.lm_post) post_mail(S.mail, c->chi, (double)c->it, (double)c->cur, (double)stop, seq);
      return;
    }
    post_mail(S.mail, chi2, scale, mx, f, seq);
  }
}

// landmark sharding (trial_chunks / trial_solve): the landmark-inversion flag rides the all-reduce of the
// pose-pair sums, staged into the slot behind them and adopted from the sum
__global__ void shard_fail_stage_kernel(Sys S, double* slot) {
  *slot = (double)__hip_atomic_load(S.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void shard_fail_adopt_kernel(Sys S, const double* slot) {
  __hip_atomic_store(S.fail, *slot != 0.0 ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
int errors_blocks(int Ea) { return Ea > 0 ? (Ea + 255) / 256 : 1; }
int update_blocks(const Problem& P) {
  const int nv = P.np + P.nq + P.nl;
  return nv > 0 ? (nv + 255) / 256 : 1;
}

hipError_t compute_errors(const Problem& P, const Lin& L, const Active& A, Sys& S, unsigned long long seq,
                          hipStream_t s) {
  hipLaunchKernelGGL(errors_kernel, dim3(errors_blocks(A.Ea)), dim3(256), 0, s, P, L, A, S, 0, seq);
  return hipGetLastError();
}

int update_errors_blocks(const Active& A) {
  if (A.ue_bpr > 0) return 8 * ((A.nchk + 7) / 8) * A.ue_bpr;
  return A.nL > 0 ? (A.nL * kGroup + 64 * kUeWaves - 1) / (64 * kUeWaves) : 1;
}

void set_update_geometry(Active& A) {
  constexpr int per = 64 * kUeWaves / kGroup;  // landmarks per update workgroup
  A.ue_bpr = A.nchk >= 8 && A.lmchunk % per == 0 ? A.lmchunk / per : 0;
}

// trial tail of a window beyond fast_path, after its Schur chunks: pose-pair sums + Cholesky in global
// memory, back-substitution + candidate state, the candidate's cost (posted with seq; 0: not posted)
static hipError_t global_tail(const Problem& P, const Lin& L, const Active& A, const Sys& S, double lambda,
                              unsigned long long seq, hipStream_t s) {
  launch_global_solve(A, S, lambda, s);
  const int nbu = update_blocks(P);
  hipLaunchKernelGGL(update_kernel, dim3(nbu), dim3(256), 0, s, P, L, A, S, lambda);
  Problem Pn = P;  // cost of the candidate state
  Pn.T = P.Tn; Pn.X = P.Xn; Pn.L = P.Ln;
  hipLaunchKernelGGL(errors_kernel, dim3(errors_blocks(A.Ea)), dim3(256), 0, s, Pn, L, A, S, nbu, seq);
  return hipGetLastError();
}

hipError_t trial_host_large(const Problem& P, const Lin& L, const Active& A, Sys& S, double lambda,
                            unsigned long long seq, hipStream_t s) {
  if (fast_path(A.K)) return hipErrorInvalidValue;  // (trial_dev, or trial_chunks / trial_solve when sharded)
  if (chunk_count(A) > 0) launch_chunks(P, L, A, S, lambda, L, S, false, s);
  return global_tail(P, L, A, S, lambda, seq, s);
}

hipError_t trial_dev(const Problem& P, const Lin& L, const Active& A, Sys& S, unsigned long long seq, hipStream_t s,
                     const Spec& spec, hipEvent_t* ev) {
  if (!S.lm || !fast_path(A.K)) return hipErrorInvalidValue;
  if (ev) (void)hipEventRecord(ev[0], s);
  if (chunk_count(A) > 0) launch_chunks(P, L, A, S, 0.0, spec.Ls, spec.Ss, wave_path(A.K), s);
  const hipError_t e = launch_solve(P, A, S, 0.0, s, true);
  if (e != hipSuccess) return e;
  const int nbu = update_errors_blocks(A), nbl = A.n_lblk;
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(update_errors_kernel<true>, dim3(nbu + nbl), dim3(256), 0, s, P, L, A, S, 0.0, seq, spec.Ls,
                     spec.Ss, nbu);
  if (ev) (void)hipEventRecord(ev[2], s);
  return hipGetLastError();
}

hipError_t trial_chunks(const Problem& P, const Lin& L, const Active& A, Sys& S, double lambda, hipStream_t s) {
  if (chunk_count(A) > 0) launch_chunks(P, L, A, S, lambda, L, S, false, s);
  hipLaunchKernelGGL(shard_fail_stage_kernel, dim3(1), dim3(1), 0, s, S, S.pairfin + (size_t)A.npairs * 48);
  return hipGetLastError();
}

hipError_t trial_solve(const Problem& P, const Lin& L, const Active& A, Sys& S, double lambda, hipStream_t s) {
  hipLaunchKernelGGL(shard_fail_adopt_kernel, dim3(1), dim3(1), 0, s, S, S.pairfin + (size_t)A.npairs * 48);
  if (!fast_path(A.K)) return global_tail(P, L, A, S, lambda, 0ull, s);
  const hipError_t e = launch_solve(P, A, S, lambda, s, false);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(update_errors_kernel<false>, dim3(update_errors_blocks(A)), dim3(256), 0, s, P, L, A, S, lambda,
                     0ull, L, S, 0);
  return hipGetLastError();
}

}  // namespace ba
}  // namespace rspl
