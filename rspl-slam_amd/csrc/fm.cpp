// F-matrix RANSAC handle: C ABI (include/rspl.h, rspl_fm_*) over fm_kernels.hip.
// Mirrors cv::findFundamentalMat(points0, points1, cv::FM_RANSAC, 3, 0.99, inliers) as
// PointMatching::MatchingPoints calls it (src/point_matching.cc:34-45).  rspl_fm_solve restates the subset
// sampling on the host -- cv::RNG seeded (uint64)-1, 7 distinct indices, checkSubset's redraws -- so every
// iteration is known up front: the upload, three launches, one wait.  rspl_fm_enqueue is the device-resident
// chain: the gather kernel composes the matches and draws the subsets from the handle's table of raw draws.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "fm_kernels.hpp"
#include "fm_solve.hpp"
#include "ransac.hpp"

using namespace rspl;

struct rspl_fm {
  rspl_fm_config cfg{};
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  Arena arena;
  PinnedArena pinned;
  fm::Args a{};
  // host-mapped (pieces of `pinned`) staging of rspl_fm_solve's upload, with the device pointers the copy kernel reads
  fm::Desc *s_desc = nullptr, *s_desc_dev = nullptr;
  double *s_p0 = nullptr, *s_p0_dev = nullptr, *s_p1 = nullptr, *s_p1_dev = nullptr;
  int32_t *s_sub = nullptr, *s_sub_dev = nullptr;
  // host-mapped: the device-resident frames' parameters in, the results out
  fm::Param* params = nullptr;
  fm::Out* out = nullptr;
  uint8_t* inl = nullptr;
  bool pending = false;
  int batch = 0;  // frames of the last solve / enqueue
};

namespace {

// RANSACPointSetRegistrator::getSubset over cv::RNG::next for every iteration: 7 distinct indices, a subset
// failing checkSubset is drawn again from the continuing stream, at most kMaxAttempts times.  p0 / p1: the
// float-rounded pairs.  Returns the subsets found (the sequence ends where getSubset gives up).
int subsets(int count, int iters, const double* p0, const double* p1, int32_t* idx) {
  uint64_t s = (uint64_t)-1;
  for (int h = 0; h < iters; h++) {
    int32_t* o = idx + 7 * h;
    bool found = false;
    for (int attempt = 0; attempt < fm::kMaxAttempts && !found; attempt++) {
      double s0[14], s1[14];
      ransac::draw_subset<7>(s, count, o);
      for (int i = 0; i < 7; i++) {
        const int v = o[i];
        s0[2 * i] = p0[2 * v]; s0[2 * i + 1] = p0[2 * v + 1];
        s1[2 * i] = p1[2 * v]; s1[2 * i + 1] = p1[2 * v + 1];
      }
      found = fm::check_subset(s0, s1);
    }
    if (!found) return h;
  }
  return iters;
}

bool good_ransac(double threshold, double confidence) {
  return std::isfinite(threshold) && threshold > 0 && confidence >= 0 && confidence <= 1;
}

void fill_results(rspl_fm* h, int batch, rspl_fm_result* res) {
  for (int b = 0; b < batch; b++) {
    const fm::Out& o = h->out[b];
    rspl_fm_result& r = res[b];
    r.n_inliers = o.n_inliers;
    r.hypotheses = o.hyps;
    memcpy(r.F, o.F, sizeof(r.F));
    if (r.inlier) memcpy(r.inlier, h->inl + (size_t)b * h->cfg.max_matches, o.n);
  }
}

}  // namespace

extern "C" int rspl_fm_create(const rspl_fm_config* cfg, rspl_fm** out) {
  RSPL_CHECK_ARG(cfg && out, "rspl_fm_create: NULL argument");
  *out = nullptr;
  RSPL_CHECK_ARG(cfg->max_batch > 0 && cfg->max_matches > 0 && cfg->max_matches <= fm::kMaxMatches,
                 "rspl_fm_create: max_batch %d, max_matches %d (at most %d)", cfg->max_batch, cfg->max_matches,
                 fm::kMaxMatches);
  RSPL_CHECK_ARG(cfg->max_iters >= 1 && cfg->max_iters <= fm::kMaxIters, "rspl_fm_create: max_iters %d outside 1..%d",
                 cfg->max_iters, fm::kMaxIters);
  RSPL_CHECK_ARG((size_t)cfg->max_batch * cfg->max_matches <= (size_t)1 << 26,
                 "rspl_fm_create: max_batch * max_matches too large");
  // The draw table holds exactly what the device-resident path can use: the generator is deterministic, so
  // the draws max_iters + kRedrawSlack subsets consume are computed here for EVERY match count an enqueue can
  // meet (8 .. max_matches).  need[count] is what the gather kernel tabulates for that count.  Small counts
  // reject the most duplicates (count 8: ~13.7 draws per subset); where max_iters + kRedrawSlack subsets do
  // not fit the kernel's LDS tables, the slack shrinks, and below kMinSlack the handle is refused.
  const int B = cfg->max_batch, K = cfg->max_matches;
  std::vector<uint32_t> draws = ransac::raw_draws(fm::kDrawCap);
  std::vector<int32_t> need(K + 1, 0);
  int nd = 0;
  for (int c = 8; c <= K; c++) {
    int fit = 0, fit_draws = 0;
    const int all = ransac::draws_needed<7>(draws, c, cfg->max_iters + fm::kRedrawSlack, &fit, &fit_draws);
    RSPL_CHECK_ARG(all >= 0 || fit >= cfg->max_iters + fm::kMinSlack,
                   "rspl_fm_create: %d iterations of %d matches need more than %d RNG draws", cfg->max_iters, c,
                   fm::kDrawCap);
    need[c] = all >= 0 ? all : fit_draws;
    nd = std::max(nd, need[c]);
  }
  draws.resize(std::max(nd, 1));
  RSPL_HIP(hipSetDevice(cfg->device));
  auto* h = new rspl_fm();
  h->cfg = *cfg;
  const size_t E = (size_t)B * K, S = (size_t)B * fm::kMaxIters;
  fm::Args& a = h->a;
  uint32_t* d_draws = nullptr;
  int32_t* d_need = nullptr;
  auto carve = [&](auto& A, auto& P) {
    h->s_desc = P.template take<fm::Desc>(B, &h->s_desc_dev);
    h->s_p0 = P.template take<double>(2 * E, &h->s_p0_dev);
    h->s_p1 = P.template take<double>(2 * E, &h->s_p1_dev);
    h->s_sub = P.template take<int32_t>(7 * S, &h->s_sub_dev);
    h->params = P.template take<fm::Param>(B, &a.host_params);
    h->out = P.template take<fm::Out>(B, &a.out);
    h->inl = P.template take<uint8_t>(E, &a.inl);
    d_draws = A.template take<uint32_t>(draws.size());
    d_need = A.template take<int32_t>(need.size());
    a.frames = A.template take<fm::Desc>(B);
    a.p0 = A.template take<double>(2 * E);
    a.p1 = A.template take<double>(2 * E);
    a.subsets = A.template take<int32_t>(7 * S);
    a.models = A.template take<double>(27 * S);
    a.nmodels = A.template take<int32_t>(S);
    a.counts = A.template take<int32_t>(3 * S);
    a.params = A.template take<fm::Param>(B);
    a.match0 = A.template take<int32_t>(E);
    a.match1 = A.template take<int32_t>(E);
  };
  Sizer sz, psz;
  carve(sz, psz);
  int rc = h->arena.reserve(sz.used + 256);
  if (!rc) rc = h->pinned.reserve(psz.used + 256);
  if (rc) {
    rspl_fm_destroy(h);
    return rc;
  }
  carve(h->arena, h->pinned);
  bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&h->done, hipEventDisableTiming) == hipSuccess;
  // (the scratch is zeroed once so that a debug read-back of slots no kernel wrote is defined)
  ok = ok && hipMemset(h->arena.base, 0, h->arena.used) == hipSuccess &&
       hipMemcpy(d_draws, draws.data(), sizeof(uint32_t) * draws.size(), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_need, need.data(), sizeof(int32_t) * need.size(), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    set_error("rspl_fm_create: stream / event / pinned allocation failed");
    rspl_fm_destroy(h);
    return RSPL_E_DEVICE;
  }
  a.K = K;
  a.max_iters = cfg->max_iters;
  a.draws = d_draws;
  a.need = d_need;
  a.n_draws = nd;
  *out = h;
  return RSPL_OK;
}

extern "C" void rspl_fm_destroy(rspl_fm* h) {
  if (!h) return;
  if (h->pending && h->done) (void)hipEventSynchronize(h->done);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->arena.release();
  h->pinned.release();
  if (h->done) (void)hipEventDestroy(h->done);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int rspl_fm_solve(rspl_fm* h, const rspl_fm_problem* probs, int batch, rspl_fm_result* res) {
  RSPL_CHECK_ARG(h && (batch == 0 || (probs && res)), "rspl_fm_solve: NULL argument");
  RSPL_CHECK_ARG(batch >= 0 && batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
  RSPL_CHECK_ARG(!h->pending, "rspl_fm_solve: an enqueue is in flight, fetch it first");
  const int K = h->cfg.max_matches;
  for (int b = 0; b < batch; b++) {
    const rspl_fm_problem& p = probs[b];
    RSPL_CHECK_ARG(p.n >= 0 && p.n <= K && (p.n == 0 || (p.points0 && p.points1)),
                   "frame %d: %d matches outside [0, %d] or NULL points", b, p.n, K);
    RSPL_CHECK_ARG(good_ransac(p.threshold, p.confidence), "frame %d: bad RANSAC parameters", b);
  }
  if (batch == 0) return RSPL_OK;
  for (int b = 0; b < batch; b++) {
    const rspl_fm_problem& p = probs[b];
    double* q0 = h->s_p0 + 2 * (size_t)b * K;
    double* q1 = h->s_p1 + 2 * (size_t)b * K;
    for (int i = 0; i < 2 * p.n; i++) {
      q0[i] = (double)(float)p.points0[i];  // cv::Point2f
      q1[i] = (double)(float)p.points1[i];
    }
    int32_t* sub = h->s_sub + 7 * (size_t)b * fm::kMaxIters;
    fm::Desc& d = h->s_desc[b];
    d.n = p.n;
    d.iters = 0;
    if (p.n == fm::kModelPoints) {  // the direct solve
      for (int i = 0; i < 7; i++) sub[i] = i;
      d.iters = 1;
    } else if (p.n > fm::kModelPoints) {
      d.iters = subsets(p.n, h->cfg.max_iters, q0, q1, sub);
    }
    d.thr = (float)(p.threshold * p.threshold);
    d.pad = 0;
    d.confidence = p.confidence;
  }
  hipStream_t st = h->stream;
  const fm::Args& a = h->a;
  const size_t nb = (size_t)batch;
  RSPL_HIP(upload_mapped(a.frames, h->s_desc_dev, sizeof(fm::Desc) * nb, st));
  RSPL_HIP(upload_mapped(a.p0, h->s_p0_dev, sizeof(double) * 2 * nb * K, st));
  RSPL_HIP(upload_mapped(a.p1, h->s_p1_dev, sizeof(double) * 2 * nb * K, st));
  RSPL_HIP(upload_mapped(a.subsets, h->s_sub_dev, sizeof(int32_t) * 7 * nb * fm::kMaxIters, st));
  RSPL_HIP(fm::solve(a, batch, false, st));
  RSPL_HIP(hipStreamSynchronize(st));
  h->batch = batch;
  fill_results(h, batch, res);
  return RSPL_OK;
}

extern "C" int rspl_fm_enqueue(rspl_fm* h, int batch, const rspl_fm_frame* frames, void* stream) {
  RSPL_CHECK_ARG(h && (batch == 0 || frames), "rspl_fm_enqueue: NULL argument");
  RSPL_CHECK_ARG(batch >= 0 && batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
  RSPL_CHECK_ARG(!h->pending, "rspl_fm_enqueue: the previous enqueue has not been fetched");
  for (int b = 0; b < batch; b++) {
    const rspl_fm_frame& fr = frames[b];
    RSPL_CHECK_ARG(fr.d_features0 && fr.d_n0 && fr.d_features1 && fr.d_n1 && fr.d_idx0 && fr.d_idx1 && fr.d_idx0_out &&
                       fr.d_idx1_out,
                   "frame %d: NULL device pointer", b);
    RSPL_CHECK_ARG(good_ransac(fr.threshold, fr.confidence), "frame %d: bad RANSAC parameters", b);
  }
  for (int b = 0; b < batch; b++) {
    const rspl_fm_frame& fr = frames[b];
    fm::Param& p = h->params[b];
    p.feat0 = fr.d_features0;
    p.feat1 = fr.d_features1;
    p.n0 = fr.d_n0;
    p.n1 = fr.d_n1;
    p.idx0 = fr.d_idx0;
    p.idx1 = fr.d_idx1;
    p.idx0_out = fr.d_idx0_out;
    p.idx1_out = fr.d_idx1_out;
    p.threshold = fr.threshold;
    p.confidence = fr.confidence;
  }
  h->batch = batch;
  if (batch == 0) return RSPL_OK;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  RSPL_HIP(fm::gather(h->a, batch, st));
  RSPL_HIP(fm::solve(h->a, batch, true, st));
  RSPL_HIP(hipEventRecord(h->done, st));
  h->pending = true;
  return RSPL_OK;
}

extern "C" int rspl_fm_fetch(rspl_fm* h, rspl_fm_result* res) {
  RSPL_CHECK_ARG(h && (res || h->batch == 0), "rspl_fm_fetch: NULL argument");
  if (h->pending) {
    RSPL_HIP(hipEventSynchronize(h->done));
    h->pending = false;
  }
  fill_results(h, h->batch, res);
  return RSPL_OK;
}

extern "C" int rspl_fm_debug_subsets(int count, int iters, const double* points0, const double* points1, int32_t* idx,
                                     int* n_found) {
  RSPL_CHECK_ARG(count > fm::kModelPoints && iters >= 0 && points0 && points1 && idx && n_found,
                 "rspl_fm_debug_subsets: bad arguments (count must exceed 7)");
  std::vector<double> q0(2 * (size_t)count), q1(2 * (size_t)count);
  for (int i = 0; i < 2 * count; i++) {
    q0[i] = (double)(float)points0[i];
    q1[i] = (double)(float)points1[i];
  }
  *n_found = subsets(count, iters, q0.data(), q1.data(), idx);
  return RSPL_OK;
}

extern "C" int rspl_fm_debug_seven_point(const double* p0, const double* p1, double* F, int* n_models) {
  RSPL_CHECK_ARG(p0 && p1 && F && n_models, "rspl_fm_debug_seven_point: NULL argument");
  double q0[14], q1[14], w[fm::kWork];
  for (int i = 0; i < 14; i++) {
    q0[i] = (double)(float)p0[i];
    q1[i] = (double)(float)p1[i];
  }
  *n_models = fm::seven_point<1>(q0, q1, w, F);
  return RSPL_OK;
}

extern "C" int rspl_fm_debug_hypotheses(rspl_fm* h, int frame, int max, int32_t* n_models, int32_t* counts, double* F) {
  RSPL_CHECK_ARG(h && n_models && counts && F && max >= 0, "rspl_fm_debug_hypotheses: bad arguments");
  RSPL_CHECK_ARG(frame >= 0 && frame < h->batch, "frame %d not in the last batch", frame);
  RSPL_CHECK_ARG(!h->pending, "rspl_fm_debug_hypotheses: an enqueue is in flight, fetch it first");
  fm::Desc d;
  RSPL_HIP(hipMemcpy(&d, h->a.frames + frame, sizeof(d), hipMemcpyDeviceToHost));
  const int n = std::min(max, d.iters);
  if (n <= 0) return 0;
  const size_t h0 = (size_t)frame * fm::kMaxIters;
  RSPL_HIP(hipMemcpy(n_models, h->a.nmodels + h0, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  RSPL_HIP(hipMemcpy(counts, h->a.counts + 3 * h0, sizeof(int32_t) * 3 * n, hipMemcpyDeviceToHost));
  RSPL_HIP(hipMemcpy(F, h->a.models + 27 * h0, sizeof(double) * 27 * n, hipMemcpyDeviceToHost));
  return n;
}
