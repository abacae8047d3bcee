// Tracking-step handle: C ABI (include/rspl.h, rspl_track_*) over track_kernels.hip, pnp_kernels.hip and
// frame_kernels.hip.  Mirrors MapBuilder::TrackFrame + FramePoseOptimization (src/map_builder.cc:448-611)
// for a batch of independent frames as one stream-ordered chain: gather | PnP (two kernels) | seed |
// FrameOptimization | write-back, six launches and one event, no host work in between.  The solvers run
// on this handle's own Args and buffers (pnp::solve / frame::optimize), all allocated at create.
// rspl_track_enqueue_ext appends one launch (track_line_kernels.hip): the frame's line tracking against its
// keyframe slot (:450-455, :490-501) and MapBuilder::AddKeyframe's decision (:616-636); its buffers are
// allocated by rspl_track_enable_lines.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "line_kernels.hpp"
#include "ransac.hpp"
#include "track_kernels.hpp"
#include "track_line_kernels.hpp"

using namespace rspl;

struct rspl_track {
  rspl_track_config cfg{};
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  Arena arena;
  PinnedArena pinned;
  track::Args ta{};
  pnp::Args pa{};
  frame::Args fa{};
  // keyframe tables, one per slot: device arrays, their pinned upload staging and its event
  double* kf_points = nullptr;
  uint8_t* kf_state = nullptr;
  int32_t* kf_tid = nullptr;
  char* kf_stage = nullptr;
  size_t kf_stage_slot = 0;
  std::vector<hipEvent_t> kf_ev;
  std::vector<int> n0;  // -1: the slot was never set
  // host-mapped (pieces of `pinned`): the per-frame parameters in, the results out
  track::Param* params = nullptr;
  track::Out* out = nullptr;
  int32_t *o_match_kf = nullptr, *o_track_id = nullptr;
  uint8_t* o_kept = nullptr;
  bool pending = false;
  int batch = 0;  // frames of the last enqueue
  // the line side (rspl_track_enable_lines): its own arenas, the slots' id staging, host-mapped parameters / results
  bool lines_on = false;
  bool ext = false;  // the last enqueue was rspl_track_enqueue_ext
  rspl_track_lines_config lcfg{};
  Arena larena;
  PinnedArena lpinned;
  track::LineArgs la{};
  std::vector<int> kf_nl;  // lines of each slot, 0 until set
  char* kfl_stage = nullptr;
  size_t kfl_stage_slot = 0;
  std::vector<hipEvent_t> kfl_ev;
  track::LineParam* lparams = nullptr;
  track::LineOut* lout = nullptr;
  int32_t *o_lmatch = nullptr, *o_ltid = nullptr, *o_lslot = nullptr;
};

namespace {

// what rspl_track_enable_lines allocated (all of it or, after a failure there, a part)
void release_lines(rspl_track* h) {
  for (hipEvent_t e : h->kfl_ev)
    if (e) (void)hipEventDestroy(e);
  h->kfl_ev.clear();
  h->larena.release();
  h->lpinned.release();
  if (h->kfl_stage) (void)hipHostFree(h->kfl_stage);
  h->kfl_stage = nullptr;
}

}  // namespace

extern "C" int rspl_track_create(const rspl_track_config* cfg, rspl_track** out) {
  RSPL_CHECK_ARG(cfg && out, "rspl_track_create: NULL argument");
  *out = nullptr;
  RSPL_CHECK_ARG(cfg->max_batch > 0 && cfg->max_keypoints > 0, "rspl_track_create: max_batch %d, max_keypoints %d",
                 cfg->max_batch, cfg->max_keypoints);
  RSPL_CHECK_ARG((size_t)cfg->max_batch * cfg->max_keypoints <= (size_t)1 << 28,
                 "rspl_track_create: max_batch * max_keypoints too large");
  // The draw table holds exactly what the worst count needs: the generator is deterministic, so the draws
  // kMaxIters subsets consume are computed here for EVERY count an enqueue can meet (8 .. max_keypoints)
  // and the maximum taken (count 8 rejects most: 4 of 8 values are duplicates for a subset's last index).
  const int B = cfg->max_batch, K = cfg->max_keypoints;
  std::vector<uint32_t> draws = ransac::raw_draws(track::kDrawCap);
  int nd = 0;
  for (int c = 8; c <= K; c++) {
    const int need = ransac::draws_needed<5>(draws, c, pnp::kMaxIters);
    RSPL_CHECK_ARG(need >= 0, "rspl_track_create: %d correspondences need more than %d RNG draws", c, track::kDrawCap);
    nd = std::max(nd, need);
  }
  draws.resize(std::max(nd, 1));
  RSPL_HIP(hipSetDevice(cfg->device));
  auto* h = new rspl_track();
  h->cfg = *cfg;
  h->n0.assign(B, -1);
  h->kf_ev.assign(B, nullptr);
  const size_t E = (size_t)B * K;
  track::Args& t = h->ta;
  pnp::Args& p = h->pa;
  frame::Args& f = h->fa;
  uint32_t* d_draws = nullptr;
  pnp::Out* pnp_out = nullptr;
  frame::Out* frame_out = nullptr;
  auto carve = [&](auto& A, auto& P) {
    h->params = P.template take<track::Param>(B, &t.host_params);
    h->out = P.template take<track::Out>(B, &t.out);
    h->o_match_kf = P.template take<int32_t>(E, &t.o_match_kf);
    h->o_track_id = P.template take<int32_t>(E, &t.o_track_id);
    h->o_kept = P.template take<uint8_t>(E, &t.o_kept);
    d_draws = A.template take<uint32_t>(draws.size());
    h->kf_points = A.template take<double>(3 * E);
    h->kf_tid = A.template take<int32_t>(E);
    h->kf_state = A.template take<uint8_t>(E);
    t.params = A.template take<track::Param>(B);
    t.pnp_desc = A.template take<pnp::Desc>(B);
    t.pts = A.template take<double>(3 * E);
    t.kps = A.template take<double>(2 * E);
    t.subsets = A.template take<int32_t>((size_t)5 * pnp::kMaxIters * B);
    t.frame_desc = A.template take<frame::Desc>(B);
    t.edges = A.template take<frame::Edge>(E);
    t.inl_in = A.template take<uint8_t>(E);
    t.corr_kp = A.template take<int32_t>(E);
    t.edge_kp = A.template take<int32_t>(E);
    t.kp_edge = A.template take<int32_t>(E);
    t.match_kf = A.template take<int32_t>(E);
    t.inl_tid = A.template take<int32_t>(E);
    t.counts = A.template take<int32_t>((size_t)4 * B);
    t.seed = A.template take<track::Seed>(B);
    p.inl = A.template take<uint8_t>(E);
    pnp_out = A.template take<pnp::Out>(B);
    p.hyp = A.template take<double>((size_t)12 * pnp::kMaxIters * B);
    p.hcnt = A.template take<int>((size_t)pnp::kMaxIters * B);
    f.err = A.template take<double>(4 * E);
    f.level = A.template take<uint8_t>(E);
    f.inl = A.template take<uint8_t>(E);
    f.inl_out = A.template take<uint8_t>(E);
    frame_out = A.template take<frame::Out>(B);
  };
  Sizer sz, psz;
  carve(sz, psz);
  int rc = h->arena.reserve(sz.used + 256);
  if (!rc) rc = h->pinned.reserve(psz.used + 256);
  if (rc) {
    rspl_track_destroy(h);
    return rc;
  }
  carve(h->arena, h->pinned);
  h->kf_stage_slot = al256((size_t)K * (3 * sizeof(double) + sizeof(int32_t) + 1));
  bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&h->done, hipEventDisableTiming) == hipSuccess &&
            hipHostMalloc((void**)&h->kf_stage, h->kf_stage_slot * B, hipHostMallocDefault) == hipSuccess;
  for (int s = 0; ok && s < B; s++) ok = hipEventCreateWithFlags(&h->kf_ev[s], hipEventDisableTiming) == hipSuccess;
  // (the scratch is zeroed once so that a debug read-back of slots no kernel wrote is defined)
  ok = ok && hipMemset(h->arena.base, 0, h->arena.used) == hipSuccess &&
       hipMemcpy(d_draws, draws.data(), sizeof(uint32_t) * draws.size(), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    set_error("rspl_track_create: stream / event / pinned allocation failed");
    rspl_track_destroy(h);
    return RSPL_E_DEVICE;
  }
  t.K = K;
  t.draws = d_draws;
  t.n_draws = nd;
  t.pnp_out = pnp_out;
  t.frame_out = frame_out;
  t.edge_inl = f.inl_out;
  p.frames = t.pnp_desc;
  p.pts = t.pts;
  p.kps = t.kps;
  p.subsets = t.subsets;
  p.out = pnp_out;
  p.prof = nullptr;
  f.frames = t.frame_desc;
  f.edges = t.edges;
  f.inl_in = t.inl_in;
  f.out = frame_out;
  *out = h;
  return RSPL_OK;
}

extern "C" void rspl_track_destroy(rspl_track* h) {
  if (!h) return;
  if (h->pending && h->done) (void)hipEventSynchronize(h->done);
  for (hipEvent_t e : h->kf_ev)
    if (e) {
      (void)hipEventSynchronize(e);
      (void)hipEventDestroy(e);
    }
  for (hipEvent_t e : h->kfl_ev)
    if (e) (void)hipEventSynchronize(e);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->arena.release();
  h->pinned.release();
  release_lines(h);
  if (h->kf_stage) (void)hipHostFree(h->kf_stage);
  if (h->done) (void)hipEventDestroy(h->done);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int rspl_track_set_keyframe(rspl_track* h, int slot, int n0, const double* points, const uint8_t* state,
                                       const int32_t* track_id, void* stream) {
  RSPL_CHECK_ARG(h, "rspl_track_set_keyframe: NULL handle");
  RSPL_CHECK_ARG(slot >= 0 && slot < h->cfg.max_batch, "slot %d outside [0, %d)", slot, h->cfg.max_batch);
  RSPL_CHECK_ARG(n0 >= 0 && n0 <= h->cfg.max_keypoints, "n0 %d exceeds max_keypoints %d", n0, h->cfg.max_keypoints);
  RSPL_CHECK_ARG(n0 == 0 || (points && state && track_id), "rspl_track_set_keyframe: NULL array");
  RSPL_CHECK_ARG(!h->pending, "rspl_track_set_keyframe: an enqueue is in flight, fetch it first");
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const size_t K = h->cfg.max_keypoints;
  // the slot's staging may still feed an earlier upload: that copy (only it) is waited for
  RSPL_HIP(hipEventSynchronize(h->kf_ev[slot]));
  char* sg = h->kf_stage + h->kf_stage_slot * slot;
  char* sg_tid = sg + 3 * sizeof(double) * K;
  char* sg_state = sg_tid + sizeof(int32_t) * K;
  if (n0) {
    memcpy(sg, points, 3 * sizeof(double) * n0);
    memcpy(sg_tid, track_id, sizeof(int32_t) * n0);
    memcpy(sg_state, state, n0);
    RSPL_HIP(hipMemcpyAsync(h->kf_points + 3 * K * slot, sg, 3 * sizeof(double) * n0, hipMemcpyHostToDevice, st));
    RSPL_HIP(hipMemcpyAsync(h->kf_tid + K * slot, sg_tid, sizeof(int32_t) * n0, hipMemcpyHostToDevice, st));
    RSPL_HIP(hipMemcpyAsync(h->kf_state + K * slot, sg_state, n0, hipMemcpyHostToDevice, st));
    RSPL_HIP(hipEventRecord(h->kf_ev[slot], st));
  }
  h->n0[slot] = n0;
  return RSPL_OK;
}

extern "C" int rspl_track_keyframe_table(rspl_track* h, int slot, int n0, double** d_points, uint8_t** d_state,
                                         int32_t** d_track_id) {
  RSPL_CHECK_ARG(h && d_points && d_state && d_track_id, "rspl_track_keyframe_table: NULL argument");
  RSPL_CHECK_ARG(slot >= 0 && slot < h->cfg.max_batch, "slot %d outside [0, %d)", slot, h->cfg.max_batch);
  RSPL_CHECK_ARG(n0 >= 0 && n0 <= h->cfg.max_keypoints, "n0 %d exceeds max_keypoints %d", n0, h->cfg.max_keypoints);
  RSPL_CHECK_ARG(!h->pending, "rspl_track_keyframe_table: an enqueue is in flight, fetch it first");
  // an earlier host upload into this slot has to land before a device producer overwrites it
  RSPL_HIP(hipEventSynchronize(h->kf_ev[slot]));
  const size_t K = h->cfg.max_keypoints;
  *d_points = h->kf_points + 3 * K * slot;
  *d_state = h->kf_state + K * slot;
  *d_track_id = h->kf_tid + K * slot;
  h->n0[slot] = n0;
  return RSPL_OK;
}

// rspl_track_enqueue (ext == NULL) and rspl_track_enqueue_ext: the same chain, then the line / decision launch
static int enqueue(rspl_track* h, int batch, const rspl_track_frame* frames, const rspl_track_frame_ext* ext,
                   void* stream) {
  RSPL_CHECK_ARG(h && (batch == 0 || frames), "rspl_track_enqueue: NULL argument");
  RSPL_CHECK_ARG(batch >= 0 && batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
  RSPL_CHECK_ARG(!h->pending, "rspl_track_enqueue: the previous enqueue has not been fetched");
  const size_t K = h->cfg.max_keypoints;
  int max_n = 0;
  for (int b = 0; b < batch; b++) {
    const rspl_track_frame& fr = frames[b];
    RSPL_CHECK_ARG(fr.slot >= 0 && fr.slot < h->cfg.max_batch && h->n0[fr.slot] >= 0,
                   "frame %d: keyframe slot %d is not set", b, fr.slot);
    RSPL_CHECK_ARG(fr.d_features && fr.d_n1 && fr.d_idx0 && fr.d_idx1, "frame %d: NULL device pointer", b);
    RSPL_CHECK_ARG(fr.th_mono_point > 0 && fr.th_stereo_point > 0 && fr.min_num_match >= 0,
                   "frame %d: bad thresholds", b);
    bool finite = std::isfinite(fr.fx) && std::isfinite(fr.fy) && std::isfinite(fr.cx) && std::isfinite(fr.cy) &&
                  std::isfinite(fr.bf);
    for (int k = 0; k < 12; k++) finite = finite && std::isfinite(fr.last_Twc[k]);
    RSPL_CHECK_ARG(finite && fr.fx != 0 && fr.fy != 0, "frame %d: bad camera or last pose", b);
    // the edge count is the device's; its bound min(n0, max_keypoints) = n0 sizes the launch
    max_n = std::max(max_n, h->n0[fr.slot]);
    if (ext) {
      const rspl_track_frame_ext& x = ext[b];
      RSPL_CHECK_ARG(x.n_lines >= 0 && x.n_lines <= h->lcfg.max_lines, "frame %d: n_lines %d outside [0, %d]", b,
                     x.n_lines, h->lcfg.max_lines);
      RSPL_CHECK_ARG(x.n_lines == 0 || x.d_lines, "frame %d: NULL d_lines with n_lines %d", b, x.n_lines);
      bool fin = std::isfinite(x.max_angle) && std::isfinite(x.max_distance);
      for (int k = 0; k < 12; k++) fin = fin && std::isfinite(x.kf_Twc[k]);
      RSPL_CHECK_ARG(fin, "frame %d: bad keyframe pose or thresholds", b);
    }
  }
  if (batch == 0) return RSPL_OK;
  for (int b = 0; ext && b < batch; b++) {
    const rspl_track_frame_ext& x = ext[b];
    track::LineParam& L = h->lparams[b];
    L.lines = x.d_lines;
    L.n_lines = x.n_lines;
    L.slot = frames[b].slot;
    L.kf_n_lines = h->kf_nl[L.slot];
    L.kf_frame_id = x.kf_frame_id;
    L.frame_id = x.frame_id;
    L.max_num_match = x.max_num_match;
    L.max_num_passed_frame = x.max_num_passed_frame;
    L.pad = 0;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) L.kf_R[3 * r + c] = x.kf_Twc[4 * r + c];
      L.kf_t[r] = x.kf_Twc[4 * r + 3];
    }
    L.max_angle = x.max_angle;
    L.max_distance = x.max_distance;
  }
  for (int b = 0; b < batch; b++) {
    const rspl_track_frame& fr = frames[b];
    track::Param& P = h->params[b];
    P.feat = fr.d_features;
    P.n1 = fr.d_n1;
    P.idx0 = fr.d_idx0;
    P.idx1 = fr.d_idx1;
    P.u_right = fr.d_u_right;
    P.kf_points = h->kf_points + 3 * K * fr.slot;
    P.kf_state = h->kf_state + K * fr.slot;
    P.kf_tid = h->kf_tid + K * fr.slot;
    P.n0 = h->n0[fr.slot];
    P.min_match = fr.min_num_match;
    P.iters = 100;  // cv::solvePnPRansac(..., 100, 20.0, 0.99, ...) (g2o_optimization.cc:438-439)
    P.pad = 0;
    P.cam[0] = fr.fx; P.cam[1] = fr.fy; P.cam[2] = fr.cx; P.cam[3] = fr.cy; P.cam[4] = fr.bf;
    P.thr2 = 20.0 * 20.0;
    P.confidence = 0.99;
    // const float deltaMonoPoint = sqrt(cfg.mono_point) (g2o_optimization.cc:279-280)
    P.delta[0] = (double)(float)std::sqrt(fr.th_mono_point);
    P.delta[1] = (double)(float)std::sqrt(fr.th_stereo_point);
    P.th[0] = fr.th_mono_point;
    P.th[1] = fr.th_stereo_point;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) P.last[3 * r + c] = fr.last_Twc[4 * r + c];
      P.last[9 + r] = fr.last_Twc[4 * r + 3];
    }
  }
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  RSPL_HIP(track::gather(h->ta, batch, st));
  RSPL_HIP(pnp::solve(h->pa, batch, 100, st));
  RSPL_HIP(track::seed(h->ta, batch, st));
  RSPL_HIP(frame::optimize(h->fa, batch, max_n, st));
  RSPL_HIP(track::write_back(h->ta, batch, st));
  if (ext) RSPL_HIP(track::frame_lines(h->ta, h->la, batch, st));
  RSPL_HIP(hipEventRecord(h->done, st));
  h->pending = true;
  h->batch = batch;
  h->ext = ext != nullptr;
  return RSPL_OK;
}

extern "C" int rspl_track_enqueue(rspl_track* h, int batch, const rspl_track_frame* frames, void* stream) {
  return enqueue(h, batch, frames, nullptr, stream);
}

extern "C" int rspl_track_enqueue_ext(rspl_track* h, int batch, const rspl_track_frame* frames,
                                      const rspl_track_frame_ext* ext, void* stream) {
  RSPL_CHECK_ARG(h && (batch == 0 || ext), "rspl_track_enqueue_ext: NULL argument");
  RSPL_CHECK_ARG(h->lines_on, "rspl_track_enqueue_ext: call rspl_track_enable_lines first");
  if (batch == 0) ext = nullptr;  // nothing is launched, as rspl_track_enqueue
  return enqueue(h, batch, frames, ext, stream);
}

extern "C" int rspl_track_enable_lines(rspl_track* h, const rspl_track_lines_config* cfg) {
  // (the configuration first, so that it is judged on its own, whatever the handle)
  RSPL_CHECK_ARG(cfg, "rspl_track_enable_lines: NULL configuration");
  RSPL_CHECK_ARG(cfg->max_lines >= 1 && cfg->max_lines <= 1024, "rspl_track_enable_lines: max_lines %d outside [1, 1024]",
                 cfg->max_lines);
  RSPL_CHECK_ARG(cfg->max_pairs > 0, "rspl_track_enable_lines: max_pairs %d is not positive", cfg->max_pairs);
  RSPL_CHECK_ARG(h, "rspl_track_enable_lines: NULL handle");
  RSPL_CHECK_ARG(h->cfg.max_keypoints <= lines::kMaxPointsLds,
                 "rspl_track_enable_lines: max_keypoints %d exceeds the %d a line workgroup holds", h->cfg.max_keypoints,
                 lines::kMaxPointsLds);
  RSPL_CHECK_ARG(!h->lines_on, "rspl_track_enable_lines: already enabled");
  RSPL_CHECK_ARG(!h->pending, "rspl_track_enable_lines: an enqueue is in flight, fetch it first");
  RSPL_HIP(hipSetDevice(h->cfg.device));
  const size_t S = h->cfg.max_batch, K = h->cfg.max_keypoints, ML = cfg->max_lines, cap = cfg->max_pairs;
  track::LineArgs& g = h->la;
  auto carve = [&](auto& A, auto& P) {
    h->lparams = P.template take<track::LineParam>(S, &g.lparams);
    h->lout = P.template take<track::LineOut>(S, &g.out);
    h->o_lmatch = P.template take<int32_t>(S * ML, &g.o_line_match);
    h->o_ltid = P.template take<int32_t>(S * ML, &g.o_line_tid);
    h->o_lslot = P.template take<int32_t>(S * ML, &g.o_line_slot);
    g.kf_off = A.template take<int>(S * (ML + 1));
    g.kf_idx = A.template take<int>(S * cap);
    g.kf_dist = A.template take<double>(S * cap);
    g.kf_kstart = A.template take<int>(S * (K + 1));
    g.kf_kline = A.template take<int>(S * cap);
    g.kf_status = A.template take<int>(S);
    g.kf_ltid = A.template take<int32_t>(S * ML);
    g.kf_lslot = A.template take<int32_t>(S * ML);
    g.off = A.template take<int>(S * (ML + 1));
    g.idx = A.template take<int>(S * cap);
    g.dist = A.template take<double>(S * cap);
    g.kline = A.template take<int>(S * cap);
    g.M = A.template take<int>(S * ML * ML);
    g.line_match = A.template take<int32_t>(S * ML);
    g.line_tid = A.template take<int32_t>(S * ML);
    g.line_slot = A.template take<int32_t>(S * ML);
  };
  Sizer sz, psz;
  carve(sz, psz);
  int rc = h->larena.reserve(sz.used + 256);
  if (!rc) rc = h->lpinned.reserve(psz.used + 256);
  if (rc) {
    release_lines(h);
    return rc;
  }
  carve(h->larena, h->lpinned);
  h->kf_nl.assign(S, 0);
  h->kfl_ev.assign(S, nullptr);
  h->kfl_stage_slot = al256(2 * sizeof(int32_t) * ML);
  bool ok = hipHostMalloc((void**)&h->kfl_stage, h->kfl_stage_slot * S, hipHostMallocDefault) == hipSuccess;
  for (size_t s = 0; ok && s < S; s++) ok = hipEventCreateWithFlags(&h->kfl_ev[s], hipEventDisableTiming) == hipSuccess;
  // (zeroed once: a slot whose lines were never set has status 0, and a debug read-back is defined)
  ok = ok && hipMemset(h->larena.base, 0, h->larena.used) == hipSuccess;
  if (!ok) {
    set_error("rspl_track_enable_lines: event / pinned allocation failed");
    release_lines(h);
    return RSPL_E_DEVICE;
  }
  g.K = (int)K;
  g.max_lines = (int)ML;
  g.cap = (int)cap;
  h->lcfg = *cfg;
  h->lines_on = true;
  return RSPL_OK;
}

extern "C" int rspl_track_set_keyframe_lines(rspl_track* h, int slot, int n_lines, const double* d_lines,
                                             const double* d_features, const int32_t* d_n0,
                                             const int32_t* line_track_id, const int32_t* line_slot, void* stream) {
  RSPL_CHECK_ARG(h, "rspl_track_set_keyframe_lines: NULL handle");
  RSPL_CHECK_ARG(h->lines_on, "rspl_track_set_keyframe_lines: call rspl_track_enable_lines first");
  RSPL_CHECK_ARG(slot >= 0 && slot < h->cfg.max_batch, "slot %d outside [0, %d)", slot, h->cfg.max_batch);
  RSPL_CHECK_ARG(n_lines >= 0 && n_lines <= h->lcfg.max_lines, "n_lines %d outside [0, %d]", n_lines, h->lcfg.max_lines);
  RSPL_CHECK_ARG(n_lines == 0 || (d_lines && d_features && d_n0 && line_track_id && line_slot),
                 "rspl_track_set_keyframe_lines: NULL array");
  RSPL_CHECK_ARG(!h->pending, "rspl_track_set_keyframe_lines: an enqueue is in flight, fetch it first");
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  if (n_lines) {
    const size_t ML = h->lcfg.max_lines;
    // the slot's staging may still feed an earlier upload: that copy (only it) is waited for
    RSPL_HIP(hipEventSynchronize(h->kfl_ev[slot]));
    int32_t* sg = (int32_t*)(h->kfl_stage + h->kfl_stage_slot * slot);
    memcpy(sg, line_track_id, sizeof(int32_t) * n_lines);
    memcpy(sg + ML, line_slot, sizeof(int32_t) * n_lines);
    RSPL_HIP(hipMemcpyAsync(h->la.kf_ltid + ML * slot, sg, sizeof(int32_t) * n_lines, hipMemcpyHostToDevice, st));
    RSPL_HIP(hipMemcpyAsync(h->la.kf_lslot + ML * slot, sg + ML, sizeof(int32_t) * n_lines, hipMemcpyHostToDevice, st));
    RSPL_HIP(hipEventRecord(h->kfl_ev[slot], st));
    RSPL_HIP(track::kf_lines(h->la, slot, d_lines, n_lines, d_features, d_n0, st));
  }
  h->kf_nl[slot] = n_lines;  // (0 lines: nothing of the slot is read)
  return RSPL_OK;
}

extern "C" int rspl_track_frame_lines(rspl_track* h, int frame, int32_t** d_line_track_id, int32_t** d_line_slot) {
  RSPL_CHECK_ARG(h && d_line_track_id && d_line_slot, "rspl_track_frame_lines: NULL argument");
  RSPL_CHECK_ARG(h->lines_on, "rspl_track_frame_lines: call rspl_track_enable_lines first");
  RSPL_CHECK_ARG(frame >= 0 && frame < h->cfg.max_batch, "frame %d outside [0, %d)", frame, h->cfg.max_batch);
  *d_line_track_id = h->la.line_tid + (size_t)h->lcfg.max_lines * frame;
  *d_line_slot = h->la.line_slot + (size_t)h->lcfg.max_lines * frame;
  return RSPL_OK;
}

extern "C" int rspl_track_debug_lines(rspl_track* h, int frame, rspl_track_debug_lines_out* d) {
  RSPL_CHECK_ARG(h && d, "rspl_track_debug_lines: NULL argument");
  RSPL_CHECK_ARG(!h->pending && h->ext, "rspl_track_debug_lines: fetch an rspl_track_enqueue_ext first");
  RSPL_CHECK_ARG(frame >= 0 && frame < h->batch, "frame %d not in the last batch", frame);
  const track::LineArgs& g = h->la;
  const track::LineParam& L = h->lparams[frame];
  const size_t ML = g.max_lines, cap = g.cap;
  auto get = [](void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  };
  // one side's CSR: the offsets, then as many pairs as they count (none after an overflow)
  auto side = [&](int nl, const int* off, const int* idx, const double* dist, int32_t* o_off, int32_t* o_idx,
                  double* o_dist) -> hipError_t {
    if (nl == 0) {
      if (o_off) o_off[0] = 0;
      return hipSuccess;
    }
    int tot = 0;
    hipError_t e = get(o_off, off, sizeof(int) * (nl + 1));
    if (e == hipSuccess) e = get(&tot, off + nl, sizeof(int));
    const size_t n = (size_t)tot <= cap ? tot : 0;
    if (e == hipSuccess) e = get(o_idx, idx, sizeof(int) * n);
    if (e == hipSuccess) e = get(o_dist, dist, sizeof(double) * n);
    return e;
  };
  d->n_lines = L.n_lines;
  d->kf_n_lines = L.kf_n_lines;
  RSPL_HIP(side(L.n_lines, g.off + (ML + 1) * frame, g.idx + cap * frame, g.dist + cap * frame, d->offsets,
                d->point_idx, d->dist));
  RSPL_HIP(side(L.kf_n_lines, g.kf_off + (ML + 1) * L.slot, g.kf_idx + cap * L.slot, g.kf_dist + cap * L.slot,
                d->kf_offsets, d->kf_point_idx, d->kf_dist));
  return RSPL_OK;
}

// rspl_track_fetch (xres == NULL) and rspl_track_fetch_ext
static int fetch(rspl_track* h, rspl_track_result* res, rspl_track_ext_result* xres) {
  RSPL_CHECK_ARG(h && res, "rspl_track_fetch: NULL argument");
  RSPL_CHECK_ARG(h->pending, "rspl_track_fetch: nothing was enqueued");
  RSPL_CHECK_ARG(!xres || h->ext, "rspl_track_fetch_ext: the enqueue was not rspl_track_enqueue_ext");
  RSPL_HIP(hipEventSynchronize(h->done));
  h->pending = false;
  const size_t K = h->cfg.max_keypoints;
  for (int b = 0; b < h->batch; b++) {
    const track::Out& o = h->out[b];
    rspl_track_result& r = res[b];
    memcpy(r.pose_q, o.q, sizeof(r.pose_q));
    memcpy(r.pose_p, o.p, sizeof(r.pose_p));
    r.pose_set = o.pose_set;
    r.n_inliers = o.n_inliers;
    r.n_pnp_inliers = o.n_pnp;
    r.pnp_used = o.pnp_used;
    r.n_keypoints = o.n1;
    r.n_matches = o.n_matches;
    r.n_kept = o.n_kept;
    r.n_mono = o.n_mono;
    r.n_stereo = o.n_stereo;
    r.rounds = o.rounds;
    memcpy(r.iterations, o.iters, sizeof(r.iterations));
    memcpy(r.chi2, o.chi2, sizeof(r.chi2));
    const size_t n = (size_t)std::min<int>(std::max(o.n1, 0), (int)K);
    if (r.match_kf) memcpy(r.match_kf, h->o_match_kf + K * b, sizeof(int32_t) * n);
    if (r.track_id) memcpy(r.track_id, h->o_track_id + K * b, sizeof(int32_t) * n);
    if (r.kept) memcpy(r.kept, h->o_kept + K * b, n);
  }
  for (int b = 0; xres && b < h->batch; b++) {
    const track::LineOut& o = h->lout[b];
    rspl_track_ext_result& x = xres[b];
    x.n_lines = o.n_lines;
    x.n_line_matches = o.n_matches;
    x.n_line_tracks = o.n_tracks;
    x.overflow = o.overflow;
    x.tracked_well = o.tracked_well;
    x.add_keyframe = o.add_keyframe;
    x.delta_angle = o.delta_angle;
    x.delta_distance = o.delta_distance;
    x.passed_frames = o.passed_frames;
    const size_t ML = h->lcfg.max_lines, n = (size_t)std::min<int>(std::max(o.n_lines, 0), (int)ML);
    if (x.line_match_kf) memcpy(x.line_match_kf, h->o_lmatch + ML * b, sizeof(int32_t) * n);
    if (x.line_track_id) memcpy(x.line_track_id, h->o_ltid + ML * b, sizeof(int32_t) * n);
    if (x.line_slot) memcpy(x.line_slot, h->o_lslot + ML * b, sizeof(int32_t) * n);
  }
  return RSPL_OK;
}

extern "C" int rspl_track_fetch(rspl_track* h, rspl_track_result* res) { return fetch(h, res, nullptr); }

extern "C" int rspl_track_fetch_ext(rspl_track* h, rspl_track_result* res, rspl_track_ext_result* xres) {
  RSPL_CHECK_ARG(xres, "rspl_track_fetch_ext: NULL argument");
  return fetch(h, res, xres);
}

extern "C" int rspl_track_debug_stage(rspl_track* h, int frame, rspl_track_debug* d) {
  RSPL_CHECK_ARG(h && d, "rspl_track_debug_stage: NULL argument");
  RSPL_CHECK_ARG(!h->pending, "rspl_track_debug_stage: fetch the enqueue first");
  RSPL_CHECK_ARG(frame >= 0 && frame < h->batch, "frame %d not in the last batch", frame);
  const size_t K = h->cfg.max_keypoints, o = K * frame;
  const track::Args& t = h->ta;
  auto get = [](void* dst, const void* src, size_t bytes) {
    return dst ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  };
  int32_t cn[4];
  pnp::Desc pd;
  pnp::Out po;
  track::Seed sd;
  RSPL_HIP(get(cn, t.counts + 4 * frame, sizeof(cn)));
  RSPL_HIP(get(&pd, t.pnp_desc + frame, sizeof(pd)));
  RSPL_HIP(get(&po, t.pnp_out + frame, sizeof(po)));
  RSPL_HIP(get(&sd, t.seed + frame, sizeof(sd)));
  d->n_corr = pd.n;
  d->n_mono = cn[2];
  d->n_stereo = cn[3];
  d->n_subsets = pd.iters;
  RSPL_HIP(get(d->corr_kp, t.corr_kp + o, sizeof(int32_t) * K));
  RSPL_HIP(get(d->edge_kp, t.edge_kp + o, sizeof(int32_t) * K));
  RSPL_HIP(get(d->pnp_points, t.pts + 3 * o, sizeof(double) * 3 * K));
  RSPL_HIP(get(d->pnp_keypoints, t.kps + 2 * o, sizeof(double) * 2 * K));
  RSPL_HIP(get(d->edges, t.edges + o, sizeof(frame::Edge) * K));
  RSPL_HIP(get(d->subsets, t.subsets + (size_t)5 * pnp::kMaxIters * frame, sizeof(int32_t) * 5 * pnp::kMaxIters));
  RSPL_HIP(get(d->pnp_inlier, h->pa.inl + o, K));
  RSPL_HIP(get(d->edge_inlier, h->fa.inl_out + o, K));
  memset(d->pnp_Rwc, 0, sizeof(d->pnp_Rwc));
  memset(d->pnp_twc, 0, sizeof(d->pnp_twc));
  if (po.n_inliers > 0) {
    memcpy(d->pnp_Rwc, po.Rwc, sizeof(d->pnp_Rwc));
    memcpy(d->pnp_twc, po.twc, sizeof(d->pnp_twc));
  }
  d->pnp_n_inliers = po.n_inliers;
  d->pnp_hypotheses = po.hyps;
  memcpy(d->seed_q, sd.q, sizeof(d->seed_q));
  memcpy(d->seed_p, sd.p, sizeof(d->seed_p));
  d->pnp_used = sd.pnp_used;
  return RSPL_OK;
}
