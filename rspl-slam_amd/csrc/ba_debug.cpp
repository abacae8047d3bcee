// Local BA: measurement and test hooks -- the RSPL_BA_PROF in-kernel trace, kernel timing, the RSPL_BA_LMTRACE
// dump and the rspl_ba_debug_* entry points.  Nothing here is on a call's path unless it was switched on.
#include "ba_handle.hpp"

using namespace rspl;

namespace rspl {
namespace ba {

void arm_prof(rspl_ba* b, const Active& A, Sys& S) {
  if (!b->prof || b->prof_nb[0]) return;
  S.prof = b->prof;
  b->prof_A = A;
  b->prof_nb[0] = chunk_count(A);
  b->prof_nb[1] = update_errors_blocks(A) + A.n_lblk;
  b->prof_nb[2] = update_errors_blocks(A);
  b->prof_nb[3] = A.nchk;
  b->prof_nb[4] = A.K;
}

// RSPL_BA_PROF: one traced trial per call -> one stderr line of in-kernel spans (us, from the
// device's 100 MHz wall clock): pair_chunk first..last block start, span; gap to the solve;
// solve phases (assembly, factor, back-substitution, poses); gap; update_errors span
void report_prof(rspl_ba* b) {
  std::vector<unsigned long long> h(kProfLen);
  if (hipStreamSynchronize(b->stream) != hipSuccess ||
      hipMemcpy(h.data(), b->prof, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return;
  // per kernel: first block start, then over blocks [b0, b1) the latest stamp of each slot
  auto us = [](unsigned long long a, unsigned long long c) { return c && a ? ((double)c - (double)a) / 100.0 : -1.0; };
  auto first = [&](int off, int b0, int b1) {
    unsigned long long t = ~0ull;
    for (int i = b0; i < std::min(b1, 4096); i++)
      if (h[off + 4 * i]) t = std::min(t, h[off + 4 * i]);
    return t;
  };
  auto last = [&](int off, int b0, int b1, int slot) {
    unsigned long long t = 0;
    for (int i = b0; i < std::min(b1, 4096); i++) t = std::max(t, h[off + 4 * i + slot]);
    return t;
  };
  auto q = [](std::vector<double>& v, double f) {  // quantile (sorts v)
    if (v.empty()) return -1.0;
    std::sort(v.begin(), v.end());
    return v[std::min(v.size() - 1, (size_t)(f * v.size()))];
  };
  const int npc = b->prof_nb[0], nue = b->prof_nb[1], nbu = b->prof_nb[2];
  const unsigned long long p0 = first(kProfPc, 0, npc), u0 = first(kProfUe, 0, nue);
  fprintf(stderr,
          "ba_prof us: pcstarts %.1f pcloop %.1f pcticket %.1f pcend %.1f gap %.1f asm %.1f factor %.1f back %.1f"
          " poses %.1f gap %.1f uestarts %.1f loaded %.1f grpdone %.1f groupsend %.1f lineswait %.1f linescomp %.1f"
          " linesend %.1f sApanel %.1f sAtrail %.1f sBpanel %.1f sBtrail %.1f\n",
          us(p0, last(kProfPc, 0, npc, 0)), us(p0, last(kProfPc, 0, npc, 1)),
          us(p0, last(kProfPc, 0, npc, 2)), us(p0, last(kProfPc, 0, npc, 3)),
          us(last(kProfPc, 0, npc, 3), h[0]), us(h[0], h[1]), us(h[1], h[2]), us(h[2], h[3]), us(h[3], h[4]),
          us(h[4], u0), us(u0, last(kProfUe, 0, nue, 0)), us(u0, last(kProfUe, 0, nbu, 1)),
          us(u0, last(kProfUe, 0, nbu, 2)), us(u0, last(kProfUe, 0, nbu, 3)),
          us(u0, last(kProfUe, nbu, nue, 1)), us(u0, last(kProfUe, nbu, nue, 2)),
          us(u0, last(kProfUe, nbu, nue, 3)), us(h[1], h[5]), us(h[5], h[6]), us(h[6], h[7]), us(h[7], h[8]));
  fprintf(stderr,
          "ba_prof setup us: landmarks %.1f +pdiag %.1f lines %.1f +pdiag %.1f pair fill %.1f | blocks done %.1f cost %.1f "
          "pose diagonals + control %.1f\n",
          us(h[9], h[kProfX]), us(h[9], h[kProfX + 1]), us(h[9], h[kProfX + 2]),
          us(h[9], h[kProfX + 3]), us(h[9], h[kProfX + 4]), us(h[9], h[10]),
          us(h[10], h[11]), us(h[11], h[12]));
  {  // per chunk: start -> loop done, quantiles over the diagonal / off-diagonal pose pairs' chunks
    const int nchk = b->prof_nb[3], K = b->prof_nb[4];
    std::vector<double> dg, od;
    for (int c = 0; c < std::min(npc, 4096) && nchk > 0; c++) {
      const unsigned long long t0 = h[kProfPc + 4 * c], t1 = h[kProfPc + 4 * c + 1];
      if (!t0 || !t1) continue;
      int pr = chunk_geo(b->prof_A, c).pr, a = 0, base = 0;
      while (pr >= base + (K - a)) base += K - a++;
      ((pr - base == 0) ? dg : od).push_back(((double)t1 - (double)t0) / 100.0);
    }
    fprintf(stderr, "ba_chunks us: diag50 %.1f diag90 %.1f diagmax %.1f off50 %.1f off90 %.1f offmax %.1f "
            "ndiag %zu noff %zu\n", q(dg, 0.5), q(dg, 0.9), q(dg, 1.0), q(od, 0.5), q(od, 0.9), q(od, 1.0),
            dg.size(), od.size());
  }
  {  // line workgroups of update_errors: per block start -> operands (wait), -> evaluations (comp), -> end
    std::vector<double> w, c, e, tot;
    for (int i = nbu; i < std::min(nue, 4096); i++) {
      const unsigned long long* r = &h[kProfUe + 4 * i];
      if (!r[0] || !r[1] || !r[2] || !r[3]) continue;
      w.push_back((r[1] - (double)r[0]) / 100.0);
      c.push_back((r[2] - (double)r[1]) / 100.0);
      e.push_back((r[3] - (double)r[2]) / 100.0);
      tot.push_back((r[3] - (double)u0) / 100.0);
    }
    fprintf(stderr, "ba_lines us (p50/p90/max): operands %.1f/%.1f/%.1f evals %.1f/%.1f/%.1f tail %.1f/%.1f/%.1f "
            "end %.1f/%.1f/%.1f n %zu\n", q(w, .5), q(w, .9), q(w, 1), q(c, .5), q(c, .9), q(c, 1), q(e, .5), q(e, .9),
            q(e, 1), q(tot, .5), q(tot, .9), q(tot, 1), w.size());
  }
  b->prof_nb[0] = 0;
  (void)hipMemset(b->prof, 0, sizeof(unsigned long long) * kProfLen);
}

void add_kernel_times(rspl_ba* b) {
  for (int i : b->kev_eval) {
    float a = 0.f, c = 0.f;
    if (hipEventElapsedTime(&a, b->kev[3 * (size_t)i], b->kev[3 * (size_t)i + 1]) == hipSuccess &&
        hipEventElapsedTime(&c, b->kev[3 * (size_t)i + 1], b->kev[3 * (size_t)i + 2]) == hipSuccess) {
      b->kt_ms[0] += a;
      b->kt_ms[1] += c;
      b->kt_n[0]++;
      b->kt_n[1]++;
    }
  }
}

void dump_lm_trace(rspl_ba* b) {
  std::vector<double> h(8 * 64);
  if (hipMemcpy(h.data(), b->lm_trace, sizeof(double) * h.size(), hipMemcpyDeviceToHost) == hipSuccess)
    for (int k = 0; k < 64; k++)
      if (h[8 * k] != 0.0)
        fprintf(stderr, "lmtrace phase %d trial %d chi2 %.17g scale %.6g fail %g lambda %.6g chi0 %.17g cur %g it %g q %g\n",
                k / 32, k % 32, h[8 * k], h[8 * k + 1], h[8 * k + 2], h[8 * k + 3], h[8 * k + 4], h[8 * k + 5],
                h[8 * k + 6], h[8 * k + 7]);
  (void)hipMemset(b->lm_trace, 0, sizeof(double) * h.size());
}

}  // namespace ba
}  // namespace rspl

namespace {
// a host-only hook's problem sizes
int check_problem_sizes(const rspl_ba_problem* pr, const char* who) {
  RSPL_CHECK_ARG(pr->n_poses >= 0 && pr->n_points >= 0 && pr->n_lines >= 0 && pr->n_mono >= 0 &&
                     pr->n_stereo >= 0 && pr->n_mono_line >= 0 && pr->n_stereo_line >= 0 &&
                     (pr->n_poses == 0 || pr->pose_fixed) && pr->n_cameras >= 1,
                 "%s: bad problem sizes", who);
  return RSPL_OK;
}
}  // namespace

extern "C" int rspl_ba_kernel_timing(rspl_ba* b, int every) {
  RSPL_CHECK_ARG(b && every >= 0, "rspl_ba_kernel_timing: NULL handle or every < 0");
  RSPL_BA_REFUSE_QUEUED(b, "rspl_ba_kernel_timing");
  // the events of a call's trials, created here rather than inside a timed call (a call queues 15 trials
  // plus top-ups after rejected ones; more are created on demand, flagged in the trace record)
  for (size_t n = b->kev.size(); every > 0 && n < 3 * (size_t)ba::kEventTrials; n++) {
    hipEvent_t e;
    RSPL_HIP(hipEventCreateWithFlags(&e, kTimingEventFlags));
    b->kev.push_back(e);
  }
  b->ktime_every = every;
  b->ncalls = 0;
  return RSPL_OK;
}

extern "C" int rspl_ba_kernel_times(rspl_ba* b, double* ms, long long* launches) {
  RSPL_CHECK_ARG(b && ms && launches, "rspl_ba_kernel_times: NULL argument");
  for (int i = 0; i < 2; i++) {
    ms[i] = b->kt_ms[i];
    launches[i] = b->kt_n[i];
    b->kt_ms[i] = 0;
    b->kt_n[i] = 0;
  }
  return RSPL_OK;
}

extern "C" int rspl_ba_debug_pairs(rspl_ba* b, int rebuild, int32_t* pp_off, int cap_off, int32_t* pp, long long cap_pairs,
                                   int* n_chunks, long long* n_pairs, int* fused) {
  RSPL_CHECK_ARG(b && pp_off && pp && n_chunks && n_pairs, "rspl_ba_debug_pairs: NULL argument");
  RSPL_BA_REFUSE_QUEUED(b, "rspl_ba_debug_pairs");
  RSPL_CHECK_ARG(b->last.valid, "rspl_ba_debug_pairs: no completed unsharded call");
  ba::Active A = b->last.A;
  const int nc = ba::chunk_count(A);
  *n_chunks = nc;
  *n_pairs = 0;
  if (fused) *fused = b->last.fused;
  RSPL_CHECK_ARG(cap_off >= nc + 1, "rspl_ba_debug_pairs: %d offsets, room for %d", nc + 1, cap_off);
  RSPL_HIP(hipStreamSynchronize(b->stream));
  if (rebuild) {  // count, scan and fill on the device (the path of the sharded handle and of wide windows)
    A.pp_off = b->pp_off;
    RSPL_HIP(ba::build_pairs(A, b->pp_cnt, b->pp_off, b->pp_buf, b->stream));
    RSPL_HIP(hipStreamSynchronize(b->stream));
  }
  pp_off[0] = 0;
  if (nc == 0) return RSPL_OK;
  RSPL_HIP(hipMemcpy(pp_off, A.pp_off, sizeof(int) * (nc + 1), hipMemcpyDeviceToHost));
  *n_pairs = pp_off[nc];
  RSPL_CHECK_ARG(pp_off[nc] >= 0 && (size_t)pp_off[nc] <= b->pp_cap && *n_pairs <= cap_pairs,
                 "rspl_ba_debug_pairs: %d pairs, list capacity %zu, room for %lld", pp_off[nc], b->pp_cap, cap_pairs);
  if (*n_pairs) RSPL_HIP(hipMemcpy(pp, b->pp_buf, sizeof(int4) * (size_t)*n_pairs, hipMemcpyDeviceToHost));
  return RSPL_OK;
}

extern "C" int rspl_ba_debug_final(rspl_ba* b, uint8_t* inlier, double* T_dev, double* T_out, double* X, double* L) {
  RSPL_CHECK_ARG(b && inlier && T_dev && T_out && X && L, "rspl_ba_debug_final: NULL argument");
  RSPL_BA_REFUSE_QUEUED(b, "rspl_ba_debug_final");
  RSPL_CHECK_ARG(b->last.valid, "rspl_ba_debug_final: no completed unsharded call");
  const ba::Problem& P = b->last.P;
  const int E = b->last.E;
  RSPL_HIP(hipStreamSynchronize(b->stream));
  if (E) {  // the classify kernel's final pass: one flag per CSR position, carried to the caller's order here
    uint8_t* d = nullptr;
    RSPL_HIP(hipMalloc((void**)&d, E));
    std::vector<uint8_t> f(E);
    std::vector<int> gmap(E);
    hipError_t e = ba::classify(P, b->last.L, E, nullptr, d, 1, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(f.data(), d, E, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(gmap.data(), b->last.gmap, sizeof(int) * E, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    RSPL_HIP(e);
    for (int k = 0; k < E; k++) inlier[gmap[k]] = f[k];
  }
  if (P.np) RSPL_HIP(hipMemcpy(T_dev, P.T, sizeof(double) * 8 * P.np, hipMemcpyDeviceToHost));
  if (P.nq) RSPL_HIP(hipMemcpy(X, P.X, sizeof(double) * 3 * P.nq, hipMemcpyDeviceToHost));
  if (P.nl) RSPL_HIP(hipMemcpy(L, P.L, sizeof(double) * 6 * P.nl, hipMemcpyDeviceToHost));
  std::copy(b->last.T_out, b->last.T_out + 8 * (size_t)P.np, T_out);
  return RSPL_OK;
}

extern "C" int rspl_ba_debug_stage(const rspl_ba_problem* pr, int par_edges, int rank, int nranks, int* n_local,
                                   int* lm_off, int8_t* etype, int* epose, int* elm, int* ecam, int* gmap,
                                   int* lpose, double* eobs) {
  RSPL_CHECK_ARG(pr && n_local && lm_off && etype && epose && elm && ecam && gmap && lpose && eobs,
                 "rspl_ba_debug_stage: NULL argument");
  int rc;
  if ((rc = check_problem_sizes(pr, "rspl_ba_debug_stage"))) return rc;
  RSPL_CHECK_ARG(nranks >= 1 && rank >= 0 && rank < nranks, "rspl_ba_debug_stage: bad rank");
  ba::Stager stg;
  if ((rc = stg.count(pr, nranks > 1, rank, nranks, par_edges))) return rc;
  std::vector<int> pidx(pr->n_poses);
  stg.number_poses(pr, pidx.data());
  ba::Stager::Out so{lm_off, etype, epose, elm, ecam, gmap, lpose, eobs, pidx.data()};
  stg.place(pr, so);
  n_local[0] = stg.E;
  n_local[1] = stg.Ep;
  return RSPL_OK;
}

extern "C" int rspl_ba_debug_pair_offsets(const rspl_ba_problem* pr, int max_landmarks, int max_poses, int32_t* pp_off,
                                          int cap, int* n_chunks) {
  RSPL_CHECK_ARG(pr && pp_off && n_chunks, "rspl_ba_debug_pair_offsets: NULL argument");
  int rc;
  if ((rc = check_problem_sizes(pr, "rspl_ba_debug_pair_offsets"))) return rc;
  const int nL = pr->n_points + pr->n_lines;
  RSPL_CHECK_ARG(max_landmarks >= nL && max_poses >= pr->n_poses, "rspl_ba_debug_pair_offsets: window beyond the handle");
  ba::Stager stg;
  if ((rc = stg.count(pr, false, 0, 1, 0))) return rc;
  const int E = stg.E;
  std::vector<int> pidx(pr->n_poses);
  const int K = stg.number_poses(pr, pidx.data());
  std::vector<int> lm_off(nL + 1), epose(E + 1), elm(E + 1), ecam(E + 1), gmap(E + 1), lpose(E + 1);
  std::vector<int8_t> etype(E + 1);
  std::vector<double> eobs(8 * (size_t)E + 8);
  std::vector<uint8_t> lm_act(nL + 1);
  ba::Stager::Out so{lm_off.data(), etype.data(), epose.data(), elm.data(), ecam.data(),
                     gmap.data(),   lpose.data(), eobs.data(),  pidx.data()};
  stg.place(pr, so);
  for (int g = 0; g < nL; g++) lm_act[g] = lm_off[g + 1] > lm_off[g];
  ba::Active G{};
  ba::plan_window(G, nL, K, ba::chunk_slots_for(max_landmarks, max_poses), false);
  *n_chunks = ba::chunk_count(G);
  RSPL_CHECK_ARG(cap >= *n_chunks + 1, "rspl_ba_debug_pair_offsets: %d offsets, room for %d", *n_chunks + 1, cap);
  ba::pair_offsets(G, lm_off.data(), lpose.data(), lm_act.data(), pp_off);
  return RSPL_OK;
}
