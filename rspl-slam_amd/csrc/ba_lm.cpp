// Local BA: one g2o SparseOptimizer::optimize(iters).
// The Levenberg-Marquardt control (g2o OptimizationAlgorithmLevenberg: tau 1e-5,
// good-step factor clamp [1/3, 2/3], ni doubling, 10 trials) has two drivers: optimize_dev keeps it on
// the device (ba::LmCtrl) and queues the trials back to back; optimize_host decides on the host, one
// mailbox round trip per trial, for the landmark-sharded handle and windows beyond ba::fast_path.
// A trial is 2-3 kernels (Schur chunks; LDL^T solve + candidate poses, fused into the chunks on small
// windows; landmark update + cost); its last block posts {chi2, scale, fail} and a
// sequence number to a pinned host-mapped mailbox that the host spins on (no stream
// synchronisation, no D2H copy on the critical path).
#include <cmath>
#include <limits>

#include "ba_handle.hpp"

using namespace rspl;

namespace {

// (Lin, Sys) views of the handle's banks: the current one into (Lr, S), the spare one into (Ls, Ss), which
// otherwise copy them (the errors, the system and the control are shared)
void bank_views(const rspl_ba* b, ba::Lin& Lr, ba::Sys& S, ba::Lin& Ls, ba::Sys& Ss) {
  ba::view_bank(b->bank[0], Lr, S);
  Ls = Lr;
  Ss = S;
  ba::view_bank(b->bank[1], Ls, Ss);
}

// an accepted candidate becomes the current state; with lin also its speculative linearisation
void accept_swap(rspl_ba* b, ba::Problem& P, ba::Lin& Lr, ba::Sys& S, bool lin) {
  std::swap(P.T, P.Tn);
  std::swap(P.X, P.Xn);
  std::swap(P.L, P.Ln);
  if (!lin) return;
  std::swap(b->bank[0], b->bank[1]);
  ba::view_bank(b->bank[0], Lr, S);
}

// optimize(iters) with the LM control on the device (fast path, unsharded): the first errors, the
// first linearisation and the control's initialisation, then `iters` trials queued back to back
// with no host round trip -- each trial's last kernel takes the accept / reject decision (ba::LmCtrl)
// and the next trial's kernels read it.  The host waits once, for the trial that stops the
// optimize(); when rejected trials leave iterations undone it queues more.  At the end the host
// pointer view follows the device's current bank.
int optimize_dev(rspl_ba* b, ba::Problem& P, ba::Lin& Lr, ba::Sys& S, const ba::Active& A, int iters,
                 double* chi2_out, int* done_out, const ba::DevLmArgs& d) {
  hipStream_t st = b->stream;
  uint8_t* const cls_level = d.cls_level;
  ba::SpecFinish* const fin = d.fin;
  ba::SpecSetup* const nxt = d.nxt;
  S.lm = b->lmctl;
  S.lm_slot = 0;
  static const bool trace = getenv("RSPL_BA_LMTRACE") != nullptr;
  if (trace && !b->lm_trace) {
    RSPL_HIP(hipMalloc((void**)&b->lm_trace, sizeof(double) * 8 * 64));
    RSPL_HIP(hipMemset(b->lm_trace, 0, sizeof(double) * 8 * 64));
  }
  S.lm_trace = trace ? b->lm_trace + (iters == 10 ? 0 : 8 * 32) : nullptr;
  // errors, cost and linearisation at the current state (with cls_level: the second optimize's
  // outlier levels and landmark activity first) + computeLambdaInit into the control (slot 0);
  // nothing is posted: the host waits for the trials only
  if (d.setup_done) {
    // (queued behind the previous optimize()'s trials: SpecSetup)
  } else {
    int rg;
    if ((rg = ba::grow_device(b, b->pdg, b->pdg_cap, (size_t)ba::setup_pdg_len(A), (size_t)1 << 14, ba::kGrewPdg)))
      return rg;
    ba::Sys Su = S;  // RSPL_BA_PROF: the first optimize's setup phases too
    Su.prof = b->prof && !b->prof_nb[0] && !cls_level ? b->prof : nullptr;
    RSPL_HIP(ba::setup_dev(P, Lr, A, Su, cls_level, cls_level ? const_cast<uint8_t*>(A.lm_act) : nullptr, iters,
                           d.build_pp ? b->pp_buf : nullptr, d.build_pp && !d.pp_staged ? b->pp_cnt : nullptr,
                           b->pp_off, b->pdg, st));
  }
  unsigned long long q = b->seq;
  const unsigned long long q_first = b->seq + 1;
  ba::Lin Ls;
  ba::Sys Ss;
  bank_views(b, Lr, S, Ls, Ss);
  int queued = 0;
  const int kev0 = b->kev_used;  // this optimize's first event triple
  auto enqueue = [&](int n) -> int {
    for (int k = 0; k < n; k++, queued++) {
      q = ++b->seq;
      ba::Spec sp{Ls, Ss};
      if (queued == 3) ba::arm_prof(b, A, S);
      S.lm_slot = queued & 1;
      S.lm_post = k == n - 1;
      hipEvent_t* ev = nullptr;
      if (b->ktime_on) {
        if ((size_t)3 * (b->kev_used + 1) > b->kev.size()) {  // (pre-created by rspl_ba_kernel_timing)
          for (int i = 0; i < 3; i++) {
            hipEvent_t e;
            RSPL_HIP(hipEventCreateWithFlags(&e, kTimingEventFlags));
            b->kev.push_back(e);
          }
          b->grew |= ba::kGrewEvents;
        }
        ev = &b->kev[3 * (size_t)b->kev_used++];
      }
      const hipError_t e = ba::trial_dev(P, Lr, A, S, q, st, sp, ev);
      S.prof = nullptr;
      if (e != hipSuccess) {
        set_error("BA trial launch failed: %s", hipGetErrorString(e));
        return RSPL_E_DEVICE;
      }
    }
    return RSPL_OK;
  };
  int rc;
  unsigned long long q_last = 0;
  auto enqueue_batch = [&](int n) -> int {  // n trials (+ the speculative finish behind them)
    int r;
    if ((r = enqueue(n))) return r;
    q_last = b->seq;
    if (fin) {
      ba::Sys Sf = S;
      Sf.lm = b->lmctl;
      Sf.lm_slot = queued & 1;  // the control slot the last queued trial writes
      Sf.prof = nullptr;
      fin->q = ++b->seq;
      fin->on = true;
      RSPL_HIP(ba::finish(P, fin->L, fin->E, fin->ginv, fin->inl, fin->Th, fin->Xh, fin->Lh, Sf, fin->q, st));
    }
    return RSPL_OK;
  };
  if ((rc = enqueue_batch(iters))) return rc;
  if (fin) ba::preupload_next(b);  // the call's last kernels are queued: the next call's upload behind them
  // the second optimize()'s setup behind each batch, gated on the control the batch's last trial writes (the
  // one behind the batch in which this optimize() stops is the one that runs)
  auto queue_spec_setup = [&]() -> int {
    if (!nxt || (size_t)ba::setup_pdg_len(nxt->A2) > b->pdg_cap) return RSPL_OK;
    ba::Sys S2 = S;
    S2.lm = b->lmctl;
    S2.lm_slot = 0;
    S2.prof = nullptr;
    S2.lm_trace = nullptr;
    RSPL_HIP(ba::setup_dev(P, Lr, nxt->A2, S2, nxt->level, const_cast<uint8_t*>(nxt->A2.lm_act), nxt->iters2,
                           nullptr, nullptr, nullptr, b->pdg, st, queued & 1, &Ls, &Ss));
    nxt->queued = true;
    nxt->extra = false;
    return RSPL_OK;
  };
  if ((rc = queue_spec_setup())) return rc;
  double v[4];
  for (;;) {
    // wait for the stopping trial (trials queued after it post nothing) or the last queued one
    if ((rc = ba::spin_mail(b, "the LM trials", [&] {
          // seqlock read: the next trial may be posting while we read; v is s1's iff vseq is still s1
          const unsigned long long s1 = __atomic_load_n(&b->mail->seq, __ATOMIC_ACQUIRE);
          if (s1 >= q_first && s1 <= q_last) {
            volatile const double* mv = b->mail->v;
            for (int k = 0; k < 4; k++) v[k] = mv[k];
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            return __atomic_load_n(&b->mail->vseq, __ATOMIC_ACQUIRE) == s1 && (s1 == q_last || v[3] != 0.0);
          }
          if (fin && s1 == fin->q) {  // the speculative finish already posted over the stopping trial's
            volatile const double* mv = b->mail->v;  // seq (it posts only the seq: v / vseq stay the trial's)
            for (int k = 0; k < 4; k++) v[k] = mv[k];
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            const unsigned long long vs = __atomic_load_n(&b->mail->vseq, __ATOMIC_ACQUIRE);
            return vs >= q_first && vs <= q_last && v[3] != 0.0;
          }
          return false;
        })))
      return rc;
    if (v[3] != 0.0) {
      if (b->ktime_on) {  // the trials up to the stopping one did work (later ones are no-ops)
        unsigned long long s1 = __atomic_load_n(&b->mail->seq, __ATOMIC_ACQUIRE);
        for (unsigned long long t = q_first; t <= s1 && t <= q_last; t++) b->kev_eval.push_back(kev0 + (int)(t - q_first));
      }
      break;
    }
    // rejected trials left iterations to do: queue one trial per remaining iteration
    if (nxt) nxt->extra = nxt->topped_up = true;
    if ((rc = enqueue_batch(std::max(1, iters - (int)v[1])))) return rc;
    if ((rc = queue_spec_setup())) return rc;
  }
  S.lm = nullptr;
  if (v[2] != 0.0) accept_swap(b, P, Lr, S, true);  // the device's current bank is the host's spare one
  *chi2_out = v[0];
  *done_out = (int)v[1];
  return RSPL_OK;
}

// optimize(iters) with the LM control on the host, for what the device driver does not take: the
// landmark-sharded handle (the ranks' all-reduces sit between a trial's kernels) and windows beyond
// fast_path (global-memory Cholesky).  One mailbox round trip per trial.
int optimize_host(rspl_ba* b, ba::Problem& P, ba::Lin& Lr, ba::Sys& S, const ba::Active& A, int iters,
                  double* chi2_out, int* done_out) {
  hipStream_t st = b->stream;
  double v[4];
  int rc;
  const bool sh = b->allreduce != nullptr;
  const int n6 = 6 * A.K;
  double* so = b->red + n6 + b->nranks;  // this rank's {chi2, scale, fail} (S.shard_out)
  unsigned long long q = ++b->seq;
  RSPL_HIP(ba::compute_errors(P, Lr, A, S, q, st));
  if (sh) {  // sum the ranks' costs (and, before the first iteration, the lambda-init diagonals)
    if (iters > 0) {
      RSPL_HIP(ba::linearize(P, Lr, A, S, true, st));
      RSPL_HIP(ba::shard_fold(A, S, b->red, b->rank, b->nranks, st));
      if ((rc = ba::shard_allreduce(b, b->red, ba::shard_red_len(A.K, b->nranks)))) return rc;
      RSPL_HIP(ba::shard_post(S, b->red, n6, b->nranks, 0, 0, q, st));
    } else {
      if ((rc = ba::shard_allreduce(b, so, 3))) return rc;
      RSPL_HIP(ba::shard_post(S, b->red, n6, b->nranks, 1, 0, q, st));
    }
  } else if (iters > 0) {  // the first linearisation does not depend on the cost: queue it right behind
    RSPL_HIP(ba::linearize(P, Lr, A, S, true, st));
    q = ++b->seq;
    RSPL_HIP(ba::post(S, q, st, &A));  // posts chi2 (S.out[0]) and the max diagonal (S.out[2])
  }
  if ((rc = ba::wait_mail(b, q, v))) return rc;
  double currentChi = v[0];
  double lambda = 1e-5 * v[2], ni = 2;  // computeLambdaInit: tau * max diagonal
  int done = 0;
  for (int it = 0; it < iters; it++) {
    // iterations after the first start from an accepted candidate, whose linearisation the
    // speculative pass of that trial already produced (now current after the swap)
    double rho = 0;
    int qmax = 0;
    do {
      q = ++b->seq;
      if (sh) {  // Schur chunks -> sum of the reduced systems -> identical solve on every rank
        RSPL_HIP(ba::trial_chunks(P, Lr, A, S, lambda, st));
        if ((rc = ba::shard_allreduce(b, S.pairfin, (size_t)A.npairs * 48 + 1))) return rc;
        RSPL_HIP(ba::trial_solve(P, Lr, A, S, lambda, st));
        if ((rc = ba::shard_allreduce(b, so, 3))) return rc;
        RSPL_HIP(ba::shard_post(S, b->red, n6, b->nranks, 1, ba::fast_path(A.K) ? 1 : 0, q, st));
      } else {
        if (it == 3 && qmax == 0) ba::arm_prof(b, A, S);
        RSPL_HIP(ba::trial_host_large(P, Lr, A, S, lambda, q, st));
        S.prof = nullptr;
      }
      // speculative linearisation of the candidate into the spare set, queued behind the trial: the GPU
      // runs it while the host reads the mailbox, so the next iteration's first kernel is already queued
      // when the host decides (a rejected trial wastes it; the current set stays)
      if (it + 1 < iters) {
        ba::Lin Ls;
        ba::Sys Ss;
        bank_views(b, Lr, S, Ls, Ss);
        ba::Problem Pc = P;
        Pc.T = P.Tn; Pc.X = P.Xn; Pc.L = P.Ln;
        RSPL_HIP(ba::linearize(Pc, Ls, A, Ss, false, st));
      }
      if ((rc = ba::wait_mail(b, q, v))) return rc;
      if (getenv("RSPL_BA_LMTRACE"))
        fprintf(stderr, "lmtrace-host iters=%d it %d q %d chi2 %.17g scale %.6g fail %g lambda %.6g chi0 %.17g\n", iters, it,
                qmax, v[0], v[1], v[3], lambda, currentChi);
      const bool ok = v[3] == 0.0;
      const double tempChi = ok ? v[0] : std::numeric_limits<double>::max();
      rho = currentChi - tempChi;
      const double scale = ok ? v[1] + 1e-3 : 1.0;
      rho /= scale;
      if (rho > 0 && std::isfinite(tempChi) && ok) {
        double alpha = 1. - std::pow(2 * rho - 1, 3);
        alpha = std::min(alpha, 2. / 3.);
        lambda *= std::max(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
        // accept: the candidate becomes the current state, and its speculative linearisation
        // (when one was made) the current one
        accept_swap(b, P, Lr, S, it + 1 < iters);
      } else {
        lambda *= ni;  // reject: the current state was never modified (no restore needed)
        ni *= 2;
        if (!std::isfinite(lambda)) break;
      }
      qmax++;
    } while (rho < 0 && qmax < 10);
    done++;
    if (qmax == 10 || rho == 0 || !std::isfinite(lambda)) break;
  }
  *chi2_out = currentChi;
  *done_out = done;
  return RSPL_OK;
}

}  // namespace

namespace rspl {
namespace ba {

int shard_allreduce(rspl_ba* b, double* d, size_t n) {
  const int rc = b->allreduce(b->ar_ctx, d, n, b->stream);
  if (rc) {
    set_error("BA shard all-reduce failed (rank %d of %d, %zu doubles, rc %d)", b->rank, b->nranks, n, rc);
    return RSPL_E_DEVICE;
  }
  return RSPL_OK;
}

bool dev_lm(const rspl_ba* b, const Active& A, int iters) {
  return b->allreduce == nullptr && iters > 0 && fast_path(A.K);
}

int optimize(rspl_ba* b, Problem& P, Lin& Lr, Sys& S, const Active& A, int iters, double* chi2_out, int* done_out,
             const DevLmArgs& d) {
  return dev_lm(b, A, iters) ? optimize_dev(b, P, Lr, S, A, iters, chi2_out, done_out, d)
                             : optimize_host(b, P, Lr, S, A, iters, chi2_out, done_out);
}

}  // namespace ba
}  // namespace rspl
