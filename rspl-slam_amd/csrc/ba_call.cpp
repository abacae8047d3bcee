// Local BA: one call.  Mirrors LocalmapOptimization (src/g2o_optimization/g2o_optimization.cc:21-252):
//   optimize(10) with Huber kernels -> chi2/depth outlier levels, kernels removed ->
//   initializeOptimization(0) + optimize(5) -> inlier flags -> write back T_wc, points, lines.
// stage_call is the host part (inputs into a pinned staging slot, host work only); run_call the device part:
// upload, bind, phase 1, phase 2, final kernel, write-back.  Host->device traffic goes through the pinned
// staging slot in one upload; the final kernel writes the results straight back into it.
#include <cmath>
#include <cstring>

#include "ba_handle.hpp"
#include "se3_host.hpp"

using namespace rspl;

namespace rspl {
namespace ba {

// Host staging of one call into stage slot `slot` (inputs only: nothing touches the device or the
// stream in steady state, so the tracking thread's next call is staged while the current one runs)
int stage_call(rspl_ba* b, int slot, const rspl_ba_problem* pr, rspl_ba_result* res, StagedCall& c, bool off_chain) {
  RSPL_CHECK_ARG(b && pr && res, "rspl_ba_local: NULL argument");
  const int np = pr->n_poses, nq = pr->n_points, nl = pr->n_lines;
  const int ne[4] = {pr->n_mono, pr->n_stereo, pr->n_mono_line, pr->n_stereo_line};
  RSPL_CHECK_ARG(np >= 0 && np <= b->cfg.max_poses && nq >= 0 && nq <= b->cfg.max_points && nl >= 0 &&
                     nl <= b->cfg.max_lines,
                 "problem exceeds the handle's vertex capacity");
  for (int t = 0; t < 4; t++) RSPL_CHECK_ARG(ne[t] >= 0 && ne[t] <= b->cfg.max_edges, "edge capacity exceeded");
  RSPL_CHECK_ARG(pr->n_cameras >= 1 && pr->n_cameras <= kMaxCams && pr->cameras, "1..16 cameras required");
  RSPL_CHECK_ARG(res->pose_q && res->pose_p && (res->points || !nq) && (res->lines || !nl), "NULL result arrays");
  RSPL_CHECK_ARG(np == 0 || pr->pose_fixed, "NULL pose_fixed");
  const int Eg = ne[0] + ne[1] + ne[2] + ne[3], nL = nq + nl;
  // landmark sharding: this rank keeps the edges of its landmarks (g % nranks == rank)
  const bool sh = b->allreduce != nullptr;
  HostMarks tm;
  tm.mark("start");
  // ---- one staging region for the whole call, mirrored by the device call buffer ----
  int rc;
  // pass 1: validate, count the local edges per landmark, mark the poses with edges (ba_stage.cpp;
  // large unsharded calls on the handle's host workers)
  if ((rc = b->stg.count(pr, sh, b->rank, b->nranks, kParEdges))) return rc;
  const int E = b->stg.E, Ep = b->stg.Ep;
  tm.mark("count");
  // the window's Schur chunk geometry (run_call's A starts from it)
  Active G{};
  plan_window(G, nL, b->stg.number_poses(pr, nullptr), b->chunk_slots, true);
  const CallLayout cl(pr->n_cameras, np, nq, nl, E, 4 * (size_t)Ep + 8 * (size_t)(E - Ep), (size_t)chunk_count(G));
  const DownLayout dl(np, nq, nl, Eg);  // inlier flags by global edge id
  bool grew = false;
  if ((rc = ensure_stage(b, slot, std::max(cl.bytes, dl.bytes), &grew))) return rc;
  if (grew) trace_flag(c.tr, kGrewStage);
  char* sg = b->stage[slot];
  // vertices: VertexSE3Expmap estimate = SE3Quat(q, p).inverse() (g2o_optimization.cc:42)
  double* T = reinterpret_cast<double*>(sg + cl.T);
  for (int p = 0; p < np; p++) se3h::pose_to_estimate(pr->pose_q + 4 * p, pr->pose_p + 3 * p, T + 8 * p);
  int* pidx = reinterpret_cast<int*>(sg + cl.pidx);
  const int K = b->stg.number_poses(pr, pidx);
  // pass 2: lm_off, and every local edge at its CSR position with its reduced pose and its caller's
  // edge id (landmark-CSR order, input order within a landmark: the order every per-landmark
  // reduction follows)
  int* lm_off = reinterpret_cast<int*>(sg + cl.lm_off);
  tm.mark("vertices");
  {
    Stager::Out so;
    so.lm_off = lm_off;
    so.etype = reinterpret_cast<int8_t*>(sg + cl.type);
    so.epose = reinterpret_cast<int*>(sg + cl.pose);
    so.elm = reinterpret_cast<int*>(sg + cl.lm);
    so.ecam = reinterpret_cast<int*>(sg + cl.cam);
    so.gmap = reinterpret_cast<int*>(sg + cl.gmap);
    so.lpose = reinterpret_cast<int*>(sg + cl.lm_pose);
    so.eobs = reinterpret_cast<double*>(sg + cl.obs);
    so.pidx = pidx;
    so.ginv = sh ? nullptr : reinterpret_cast<int*>(sg + cl.ginv);  // (the final kernel's flag order: unsharded calls)
    b->stg.place(pr, so);
  }
  tm.mark("scatter");
  uint8_t* lm_act = reinterpret_cast<uint8_t*>(sg + cl.lm_act);
  size_t pair_bound = 0;  // sum_g k_g^2 >= edge pairs of any pose pair
  for (int g = 0; g < nL; g++) {
    const size_t k = lm_off[g + 1] - lm_off[g];
    pair_bound += k * k;
    lm_act[g] = k > 0;
  }
  const int n_lblk = pack_line_blocks(lm_off, nq, nL, reinterpret_cast<int4*>(sg + cl.ltab));
  int* pairs = reinterpret_cast<int*>(sg + cl.pairs);
  for (int a = 0, q = 0; a < K; a++)
    for (int c = a; c < K; c++, q++) {
      pairs[2 * q] = a;
      pairs[2 * q + 1] = c;
    }
  tm.mark("tables");
  // the fused first pass (device LM, unsharded: run_call's pp_fused) fills the Schur chunks' edge-pair lists
  // against offsets counted here when this runs off the device's chain (the staging thread: the count costs
  // about as much as the rest of the staging, a call staged on its own chain counts on the device as before);
  // the exact total sizes the list
  c.pp_staged = off_chain && !sh && pr->iterations_first > 0 && fast_path(G.K);
  if (c.pp_staged)
    pair_bound = pair_offsets(G, lm_off, reinterpret_cast<const int*>(sg + cl.lm_pose), lm_act,
                              reinterpret_cast<int*>(sg + cl.pp_off));
  tm.mark("ppoff");
  memcpy(sg + cl.cams, pr->cameras, sizeof(double) * 5 * pr->n_cameras);
  if (nq) memcpy(sg + cl.X, pr->points, sizeof(double) * 3 * nq);
  if (nl) memcpy(sg + cl.L, pr->lines, sizeof(double) * 6 * nl);
  memset(sg + cl.level, 0, cl.bytes - cl.level);  // level, flags, out start at zero
  c.slot = slot;
  c.E = E;
  c.Ep = Ep;
  c.G = G;
  c.n_lblk = n_lblk;
  c.pair_bound = pair_bound;
  c.cl = cl;
  c.dl = dl;
  c.tm = tm;
  return RSPL_OK;
}

// The next queued call's inputs, uploaded into its slot's call buffer behind the current call's last
// queued kernels (optimize(5)'s trials and the gated final kernel): the upload (~40 us over PCIe at C3)
// then runs while the host notices the current call's end and queues the next one, instead of first in
// the next call's chain.  Tracking thread only; the next call must already be staged (its slot is then
// busy until it completes, and differs from the running call's).
void preupload_next(rspl_ba* b) {
  if (!b->tracking_call) return;
  std::shared_ptr<StagedCall> nx;
  {
    std::lock_guard<std::mutex> lk(b->qmu);
    if (!b->jobs.empty() && b->jobs.front().state == 2 && b->jobs.front().sc->rc == RSPL_OK) nx = b->jobs.front().sc;
  }
  if (!nx || nx->uploaded) return;
  if (upload_mapped(b->cbuf[nx->slot], b->stage_dev[nx->slot], nx->cl.bytes, b->stream) == hipSuccess)
    nx->uploaded = true;
}

}  // namespace ba
}  // namespace rspl

namespace {

// The device part of one staged call, step by step (run_call): what the steps share
struct Call {
  rspl_ba* b;
  const ba::StagedCall& c;
  const rspl_ba_problem* pr;
  rspl_ba_result* res;
  double* tr;  // the call's trace record
  ba::HostMarks tm;
  char* cb = nullptr;        // the slot's device call buffer (CallLayout)
  char* down = nullptr;      // device view of the staging slot, where the final kernel writes (DownLayout)
  uint8_t* level = nullptr;  // the edges' outlier levels (second optimize)
  ba::Problem P{};
  ba::Lin Lr{};
  ba::Sys S{};
  ba::Active A{};
  int Eg() const { return pr->n_mono + pr->n_stereo + pr->n_mono_line + pr->n_stereo_line; }
  uint8_t* inl_h() const { return reinterpret_cast<uint8_t*>(down + c.dl.inl); }
  double* T_h() const { return reinterpret_cast<double*>(down + c.dl.T); }
  double* X_h() const { return reinterpret_cast<double*>(down + c.dl.X); }
  double* L_h() const { return reinterpret_cast<double*>(down + c.dl.L); }
};

// the call's inputs in one upload: a copy kernel reading the host-mapped staging slot over PCIe.  Not
// hipMemcpyAsync: its H2D path stalled the first calls after the warmup by 7-10 ms each (the SDMA engine /
// blit-kernel choice settling; profiles/r05_bench_20step_before.json), which cost the driver's 20-step bench
// a quarter of its rate.
int upload_inputs(Call& k) {
  rspl_ba* b = k.b;
  int rc;
  k.tm.mark("run");
  b->grew = 0;
  if ((rc = ba::grow_device(b, b->pp_buf, b->pp_cap, k.c.pair_bound, (size_t)1 << 16, ba::kGrewPairs)))
    return rc;  // edge-pair lists
  k.cb = b->cbuf[k.c.slot];
  k.down = b->stage_dev[k.c.slot];
  if (!k.c.uploaded)  // (else queued behind the previous call's final kernel: preupload_next)
    RSPL_HIP(upload_mapped(k.cb, b->stage_dev[k.c.slot], k.c.cl.bytes, b->stream));
  k.tm.mark("upload");
  k.tr[ba::kTrUpload] = ba::mono_s();
  return RSPL_OK;
}

// Problem / Lin / Sys / Active of phase 1 (all edges, Huber) bound to the call buffer through its CallLayout,
// to the handle's arena and to the window geometry the staging planned
void bind_call(Call& k) {
  rspl_ba* b = k.b;
  const rspl_ba_problem* pr = k.pr;
  const ba::CallLayout& cl = k.c.cl;
  char* cb = k.cb;
  const bool sh = b->allreduce != nullptr;
  const int E = k.c.E, Ep = k.c.Ep, K = k.c.G.K;
  k.level = reinterpret_cast<uint8_t*>(cb + cl.level);
  ba::Problem& P = k.P;
  P.cams = reinterpret_cast<double*>(cb + cl.cams);
  P.T = reinterpret_cast<double*>(cb + cl.T);
  P.X = reinterpret_cast<double*>(cb + cl.X);
  P.L = reinterpret_cast<double*>(cb + cl.L);
  P.np = pr->n_poses; P.nq = pr->n_points; P.nl = pr->n_lines; P.ncam = pr->n_cameras;
  P.Tn = b->Tb; P.Xn = b->Xb; P.Ln = b->Lb;
  P.etype = reinterpret_cast<const int8_t*>(cb + cl.type);
  P.epose = reinterpret_cast<const int*>(cb + cl.pose);
  P.elm = reinterpret_cast<const int*>(cb + cl.lm);
  P.ecam = reinterpret_cast<const int*>(cb + cl.cam);
  P.eobs = reinterpret_cast<const double*>(cb + cl.obs);
  P.Ep = Ep;
  const double th[4] = {pr->th_mono_point, pr->th_stereo_point, pr->th_mono_line, pr->th_stereo_line};
  for (int t = 0; t < 4; t++) {
    P.th[t] = th[t];
    P.delta[t] = (double)(float)std::sqrt(th[t]);  // const float thHuber = sqrt(cfg.x) (:77-78, 125-126)
  }
  P.line_jac = b->line_jac;
  k.Lr.err = b->err;
  ba::Sys& S = k.S;
  ba::view_bank(b->bank[0], k.Lr, S);
  S.bp = b->bp; S.S = b->S; S.x = b->x; S.partial = b->partial;
  S.partial2 = b->partial2;
  S.out = reinterpret_cast<double*>(cb + cl.out);
  S.fail = reinterpret_cast<int*>(cb + cl.flags);
  S.counter = reinterpret_cast<unsigned*>(cb + cl.flags + sizeof(int));
  S.lm_ctr = b->lm_ctr;
  S.mail = b->mail_dev;
  S.chunk = b->chunk;
  S.pairfin = b->pairfin;
  S.pair_ctr = b->pair_ctr;
  S.solve_ctr = b->pair_ctr + b->maxK * (b->maxK + 1) / 2;
  S.shard_out = sh ? b->red + 6 * K + b->nranks : nullptr;
  S.pose_scale = !sh || b->rank == 0;
  ba::Active& A = k.A;
  A = k.c.G;  // K, npairs, nL, the chunk plan, the update geometry
  A.Ea = E;
  A.pidx = reinterpret_cast<const int*>(cb + cl.pidx);
  A.lm_off = reinterpret_cast<const int*>(cb + cl.lm_off);
  A.lm_pose = reinterpret_cast<const int*>(cb + cl.lm_pose);
  A.lm_act = reinterpret_cast<const uint8_t*>(cb + cl.lm_act);
  A.pairs = reinterpret_cast<const int*>(cb + cl.pairs);
  A.n_line_edges = E - Ep;
  A.ltab = reinterpret_cast<const int4*>(cb + cl.ltab);
  A.n_lblk = k.c.n_lblk;
  A.robust = 1;
  A.pp_off = k.c.pp_staged ? reinterpret_cast<const int*>(cb + cl.pp_off) : b->pp_off;
  A.pp = b->pp_buf;
}

// ---- phase 1: all edges, Huber ----
int phase1(Call& k, ba::SpecSetup& nxt) {
  rspl_ba* b = k.b;
  const rspl_ba_problem* pr = k.pr;
  const bool sh = b->allreduce != nullptr;
  int rc;
  // on the BA stream itself: a second stream would take a hardware queue of its own (streams map
  // round-robin onto GPU_MAX_HW_QUEUES) and push a pipeline stream onto the BA's queue -- measured:
  // bench 2.17 ms per step instead of 1.5 with a side stream for the pair lists
  // device LM: the first pass builds the lists (against the staged offsets when the staging thread counted
  // them); else (the sharded handle, windows beyond the fast path): counted, scanned and filled here
  const bool pp_fused = ba::dev_lm(b, k.A, pr->iterations_first);
  if (!pp_fused) RSPL_HIP(ba::build_pairs(k.A, b->pp_cnt, b->pp_off, b->pp_buf, b->stream));
  k.tm.mark("pairs");
  // phase 2's setup queued behind phase 1's trials (device LM on both, unsharded)
  b->last.valid = false;
  b->last.A = k.A;
  b->last.fused = pp_fused && k.c.pp_staged;
  nxt.A2 = k.A;
  nxt.A2.robust = 0;
  nxt.A2.elevel = k.level;
  nxt.A2.lm_act = b->lm_act2;
  nxt.level = k.level;
  nxt.iters2 = pr->iterations_second;
  const bool spec_setup = pp_fused && !sh && !b->ktime_on && ba::dev_lm(b, nxt.A2, pr->iterations_second);
  ba::DevLmArgs d1;
  d1.build_pp = pp_fused;
  d1.pp_staged = k.c.pp_staged;
  d1.nxt = spec_setup ? &nxt : nullptr;
  if ((rc = ba::optimize(b, k.P, k.Lr, k.S, k.A, pr->iterations_first, &k.res->chi2_first,
                         &k.res->iterations_done_first, d1)))
    return rc;
  k.tm.mark("opt1");
  k.tr[ba::kTrOpt1] = ba::mono_s();
  return RSPL_OK;
}

// ---- phase 2: level-0 edges, no kernel (initializeOptimization(0), :176-213) ----
// Same active structure with the level-1 edges masked (exact-zero records, no cost, errors
// kept as g2o keeps them), landmark activity recomputed from the levels on the device (device LM:
// inside the optimize's first launch).
int phase2(Call& k, const ba::SpecSetup& nxt, ba::SpecFinish& fin) {
  rspl_ba* b = k.b;
  const rspl_ba_problem* pr = k.pr;
  const bool sh = b->allreduce != nullptr;
  ba::Active& A = k.A;
  int rc;
  A.robust = 0;
  A.elevel = k.level;
  A.lm_act = b->lm_act2;
  const bool fused = ba::dev_lm(b, A, pr->iterations_second);
  if (!fused) {
    RSPL_HIP(ba::classify(k.P, k.Lr, k.c.E, k.level, nullptr, 0, b->stream));
    RSPL_HIP(ba::landmark_active(A, k.level, b->lm_act2, b->stream));
  }
  // the final kernel queued behind optimize(5)'s trials (device LM, unsharded): no host round trip
  // between that optimize()'s stop and the final kernel
  const bool spec_fin = fused && !sh && !b->ktime_on;  // (kernel timing maps events to contiguous trial seqs)
  if (spec_fin) {
    fin.L = k.Lr;
    fin.E = k.c.E;
    fin.ginv = reinterpret_cast<const int*>(k.cb + k.c.cl.ginv);
    fin.inl = k.inl_h();
    fin.Th = k.T_h();
    fin.Xh = k.X_h();
    fin.Lh = k.L_h();
  }
  ba::DevLmArgs d2;
  d2.cls_level = fused ? k.level : nullptr;
  d2.fin = spec_fin ? &fin : nullptr;
  d2.setup_done = nxt.queued && !nxt.extra;
  if ((rc = ba::optimize(b, k.P, k.Lr, k.S, A, pr->iterations_second, &k.res->chi2_second,
                         &k.res->iterations_done_second, d2)))
    return rc;
  k.tm.mark("opt2");
  k.tr[ba::kTrOpt2] = ba::mono_s();
  ba::trace_flag(k.tr, (nxt.queued && !nxt.extra ? ba::kSpecSetupRan : 0u) | (nxt.topped_up ? ba::kToppedUp : 0u));
  return RSPL_OK;
}

// ---- inlier flags + final state written by the GPU into the mapped staging buffer ----
// (the staging call region was consumed by the upload long before: the stream is in order)
int finish_call(Call& k, const ba::SpecFinish& fin) {
  rspl_ba* b = k.b;
  const bool sh = b->allreduce != nullptr;
  const ba::CallLayout& cl = k.c.cl;
  hipStream_t st = b->stream;
  int rc;
  const unsigned long long q = fin.on ? fin.q : ++b->seq;
  if (fin.on) {
    // already queued (SpecFinish)
  } else if (sh) {  // owned landmarks + local edge flags gathered by one more all-reduce: complete on every rank
    const size_t glen = 3 * (size_t)k.P.nq + 6 * (size_t)k.P.nl + k.Eg();
    if ((rc = ba::grow_device(b, b->gbuf, b->gcap, glen, (size_t)1024, 0u))) return rc;
    RSPL_HIP(hipMemsetAsync(b->gbuf, 0, sizeof(double) * glen, st));
    RSPL_HIP(ba::shard_gather(k.P, k.Lr, k.c.E, reinterpret_cast<const int*>(k.cb + cl.gmap), b->rank, b->nranks,
                              b->gbuf, st));
    if (glen && (rc = ba::shard_allreduce(b, b->gbuf, glen))) return rc;
    RSPL_HIP(ba::shard_finish(k.P, k.Eg(), b->gbuf, k.inl_h(), k.T_h(), k.X_h(), k.L_h(), k.S, q, st));
  } else {
    RSPL_HIP(ba::finish(k.P, k.Lr, k.c.E, reinterpret_cast<const int*>(k.cb + cl.ginv), k.inl_h(), k.T_h(), k.X_h(),
                        k.L_h(), k.S, q, st));
  }
  return ba::wait_mail(b, q, nullptr);
}

// what was switched on to measure the call, and the buffers it grew into its trace flags
void measure_call(Call& k) {
  rspl_ba* b = k.b;
  if (b->ktime_on) ba::add_kernel_times(b);  // every timed trial precedes the finish kernel: its events are complete
  if (b->prof && b->prof_nb[0]) ba::report_prof(b);
  ba::trace_flag(k.tr, b->grew);
  if (b->lm_trace) ba::dump_lm_trace(b);
}

// the results from the staging slot into the caller's arrays: points, lines, inlier flags, poses
void write_back(Call& k) {
  rspl_ba* b = k.b;
  const rspl_ba_problem* pr = k.pr;
  rspl_ba_result* res = k.res;
  const ba::DownLayout& dl = k.c.dl;
  const char* sg = b->stage[k.c.slot];
  const int np = pr->n_poses, nq = pr->n_points, nl = pr->n_lines;
  const int ne[4] = {pr->n_mono, pr->n_stereo, pr->n_mono_line, pr->n_stereo_line};
  if (nq) memcpy(res->points, sg + dl.X, sizeof(double) * 3 * nq);
  if (nl) memcpy(res->lines, sg + dl.L, sizeof(double) * 6 * nl);
  const double* Tout = reinterpret_cast<const double*>(sg + dl.T);
  uint8_t* outs[4] = {res->mono_inlier, res->stereo_inlier, res->mono_line_inlier, res->stereo_line_inlier};
  int e = 0;
  for (int t = 0; t < 4; t++) {
    if (outs[t]) memcpy(outs[t], sg + dl.inl + e, ne[t]);
    e += ne[t];
  }
  // write back T_wc = estimate().inverse() (:235-240)
  for (int p = 0; p < np; p++) se3h::estimate_to_pose(Tout + 8 * p, res->pose_q + 4 * p, res->pose_p + 3 * p);
  b->last.P = k.P;
  b->last.L = k.Lr;
  b->last.E = k.c.E;
  b->last.gmap = reinterpret_cast<const int*>(k.cb + k.c.cl.gmap);
  b->last.T_out = Tout;
  b->last.valid = b->allreduce == nullptr;
  k.tm.mark("final");
  k.tm.print("rspl_ba_local us:");
  k.tr[ba::kTrDone] = ba::mono_s();
  k.tr[ba::kTrIters] = res->iterations_done_first + res->iterations_done_second;
}

}  // namespace

namespace rspl {
namespace ba {

int run_call(rspl_ba* b, const StagedCall& c, const rspl_ba_problem* pr, rspl_ba_result* res, double* tr) {
  Call k{b, c, pr, res, tr, c.tm};
  SpecSetup nxt;
  SpecFinish fin;
  int rc;
  if ((rc = upload_inputs(k))) return rc;
  bind_call(k);
  if ((rc = phase1(k, nxt))) return rc;
  if ((rc = phase2(k, nxt, fin))) return rc;
  if ((rc = finish_call(k, fin))) return rc;
  measure_call(k);
  write_back(k);
  return RSPL_OK;
}

int local_call(rspl_ba* b, const rspl_ba_problem* pr, rspl_ba_result* res) {
  RSPL_CHECK_ARG(b && pr && res, "rspl_ba_local: NULL argument");
  StagedCall c;
  c.tr[kTrSubmitted] = c.tr[kTrStageBegin] = mono_s();
  c.tr[kTrLocal] = 1;
  int rc = stage_call(b, 0, pr, res, c, false);  // (staged on the call's own chain)
  c.tr[kTrStageEnd] = c.tr[kTrRunBegin] = mono_s();
  if (!rc) rc = run_call(b, c, pr, res, c.tr);
  if (!rc) {
    std::lock_guard<std::mutex> lk(b->qmu);
    push_trace(b, c.tr);
  }
  return rc;
}

}  // namespace ba
}  // namespace rspl
