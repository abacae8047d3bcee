// The rspl_lines handle after the detector: point-to-line assignment, shared-point line
// matching and the stereo association of lines on the GPU (line_kernels.hip).  The detectors are in
// lines_detect.cpp, the host merge passes in line_merge.cpp.
//
//   AssignPointsToLines / MatchLines                 src/line_processor.cc:163-283 (kernels)
//   Frame::AddRightFeatures (line part)              src/frame.cc:150-203
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "line_kernels.hpp"
#include "lines_handle.hpp"

#pragma clang fp contract(off)

using namespace rspl;

extern "C" int rspl_lines_create(const rspl_lines_config* cfg, rspl_lines** out) {
  RSPL_CHECK_ARG(cfg && out, "rspl_lines_create: NULL argument");
  RSPL_CHECK_ARG(cfg->max_lines > 0 && cfg->max_lines <= 1024, "max_lines must be in [1, 1024]");
  RSPL_CHECK_ARG(cfg->max_points > 0 && cfg->max_points <= lines::kMaxPointsLds, "max_points must be in [1, %d]",
                 lines::kMaxPointsLds);
  RSPL_CHECK_ARG(cfg->max_pairs > 0 && cfg->max_matches >= 0, "max_pairs must be > 0, max_matches >= 0");
  *out = nullptr;
  RSPL_HIP(hipSetDevice(cfg->device));
  auto* h = new rspl_lines();
  h->cfg = *cfg;
  h->cap = cfg->max_pairs;
  const size_t L = cfg->max_lines, N = cfg->max_points, C = cfg->max_pairs, Mm = std::max(1, cfg->max_matches);
  // two assignment sets (left / right, or frame 0 / frame 1) and two matching problems
  auto carve = [&](auto& ar) {
    auto take = [&](auto*& p, size_t n) {
      using T = std::remove_pointer_t<std::remove_reference_t<decltype(p)>>;
      if constexpr (std::is_same_v<std::remove_reference_t<decltype(ar)>, Arena>) p = ar.template take<T>(n);
      else ar.template take<T>(n);
    };
    take(h->lines, 2 * L * 4); take(h->pts, 2 * N * 2); take(h->dist, 2 * C);
    take(h->n_lines, 2); take(h->n_points, 2); take(h->offsets, 2 * (L + 1)); take(h->idx, 2 * C);
    take(h->status, 3); take(h->matches, 2 * Mm * 2); take(h->n_matches, 2); take(h->M, 2 * L * L);
    take(h->inv, 2 * 2 * C); take(h->out, 2 * L);
  };
  Sizer sz;
  carve(sz);
  if (int rc = h->arena.reserve(sz.used)) {
    delete h;
    return rc;
  }
  carve(h->arena);
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMemset(h->status, 0, sizeof(int) * 3) != hipSuccess) {
    rspl_lines_destroy(h);
    set_error("stream creation failed");
    return RSPL_E_DEVICE;
  }
  *out = h;
  return RSPL_OK;
}

extern "C" void rspl_lines_destroy(rspl_lines* h) {
  if (!h) return;
  if (h->worker.joinable()) {
    {
      std::lock_guard<std::mutex> lk(h->mu);
      h->quit = true;
    }
    h->cv.notify_all();
    h->worker.join();
  }
  for (int k = 0; k < rspl_lines::kPinSlots; k++) {
    if (h->copy_ev[k]) {
      (void)hipEventSynchronize(h->copy_ev[k]);
      (void)hipEventDestroy(h->copy_ev[k]);
    }
    if (h->pin_lines[k]) (void)hipHostFree(h->pin_lines[k]);
  }
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->d_img) (void)hipFree(h->d_img);
  if (h->d_det) (void)hipFree(h->d_det);
  if (h->h_img) (void)hipHostFree(h->h_img);
  if (h->h_det) (void)hipHostFree(h->h_det);
  if (h->fld_img) (void)hipFree(h->fld_img);
  if (h->dev_pin) (void)hipHostFree(h->dev_pin);
  for (hipEvent_t e : h->fld_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->dev_in) (void)hipEventDestroy(h->dev_in);
  if (h->dev_done) (void)hipEventDestroy(h->dev_done);
  h->fld_arena.release();
  h->arena.release();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

namespace {

// one image's lines and keypoint (x, y) into assignment set `set`
int stage_image(rspl_lines* h, int set, const double* lines, int n_lines, const double* features, int n_points) {
  RSPL_CHECK_ARG(n_lines >= 0 && n_lines <= h->cfg.max_lines, "n_lines %d outside [0, %d]", n_lines, h->cfg.max_lines);
  RSPL_CHECK_ARG(n_points >= 0 && n_points <= h->cfg.max_points, "n_points %d outside [0, %d]", n_points,
                 h->cfg.max_points);
  RSPL_CHECK_ARG((n_lines == 0 || lines) && (n_points == 0 || features), "NULL lines / features");
  const size_t L = h->cfg.max_lines, N = h->cfg.max_points;
  std::vector<double> xy((size_t)2 * n_points);
  for (int j = 0; j < n_points; j++) {  // rows 1, 2 of the 259 x N column-major features
    xy[2 * j] = features[(size_t)259 * j + 1];
    xy[2 * j + 1] = features[(size_t)259 * j + 2];
  }
  const int cnt[2] = {n_lines, n_points};
  RSPL_HIP(hipMemcpyAsync(h->lines + set * L * 4, lines, sizeof(double) * 4 * n_lines, hipMemcpyHostToDevice, h->stream));
  RSPL_HIP(hipMemcpyAsync(h->pts + set * N * 2, xy.data(), sizeof(double) * xy.size(), hipMemcpyHostToDevice, h->stream));
  RSPL_HIP(hipMemcpyAsync(h->n_lines + set, &cnt[0], sizeof(int), hipMemcpyHostToDevice, h->stream));
  RSPL_HIP(hipMemcpyAsync(h->n_points + set, &cnt[1], sizeof(int), hipMemcpyHostToDevice, h->stream));
  RSPL_HIP(hipStreamSynchronize(h->stream));  // the host vectors above go out of scope
  return RSPL_OK;
}

int run_assign(rspl_lines* h, int B) {
  lines::AssignArgs a{};
  a.lines = h->lines; a.n_lines = h->n_lines; a.pts = h->pts; a.pt_batch = (size_t)h->cfg.max_points * 2;
  a.pt_stride = 2; a.pt_xoff = 0; a.n_points = h->n_points; a.offsets = h->offsets; a.idx = h->idx;
  a.dist = h->dist; a.max_lines = h->cfg.max_lines; a.cap = h->cap; a.status = h->status;
  RSPL_HIP(lines::assign(a, B, h->stream));
  int st[2] = {0, 0};
  RSPL_HIP(hipMemcpyAsync(st, h->status, sizeof(int) * B, hipMemcpyDeviceToHost, h->stream));
  RSPL_HIP(hipStreamSynchronize(h->stream));
  for (int b = 0; b < B; b++)
    if (st[b]) {
      set_error("point-line pairs exceed max_pairs %d", h->cap);
      return RSPL_E_CAPACITY;
    }
  return RSPL_OK;
}

int read_assignment(rspl_lines* h, int set, int n_lines, int* offsets, int* point_idx, double* dist, int capacity) {
  RSPL_HIP(hipMemcpy(offsets, h->offsets + (size_t)set * (h->cfg.max_lines + 1), sizeof(int) * (n_lines + 1),
                     hipMemcpyDeviceToHost));
  const int tot = offsets[n_lines];
  if (tot > capacity) {
    set_error("%d point-line pairs exceed capacity %d", tot, capacity);
    return RSPL_E_CAPACITY;
  }
  if (tot) {
    RSPL_HIP(hipMemcpy(point_idx, h->idx + (size_t)set * h->cap, sizeof(int) * tot, hipMemcpyDeviceToHost));
    RSPL_HIP(hipMemcpy(dist, h->dist + (size_t)set * h->cap, sizeof(double) * tot, hipMemcpyDeviceToHost));
  }
  return RSPL_OK;
}

int stage_assignment(rspl_lines* h, int set, const int* offsets, const int* idx, int n_lines, int n_points) {
  RSPL_CHECK_ARG(n_lines >= 0 && n_lines <= h->cfg.max_lines && n_points >= 0 && n_points <= h->cfg.max_points,
                 "assignment sizes outside the handle's limits");
  RSPL_CHECK_ARG(offsets && offsets[0] == 0, "offsets must start at 0");
  for (int l = 0; l < n_lines; l++) RSPL_CHECK_ARG(offsets[l + 1] >= offsets[l], "offsets must be non-decreasing");
  const int tot = offsets[n_lines];
  RSPL_CHECK_ARG(tot <= h->cap, "%d point-line pairs exceed max_pairs %d", tot, h->cap);
  for (int e = 0; e < tot; e++) RSPL_CHECK_ARG(idx[e] >= 0 && idx[e] < n_points, "point index %d outside [0, %d)", idx[e], n_points);
  const int cnt[2] = {n_lines, n_points};
  RSPL_HIP(hipMemcpy(h->offsets + (size_t)set * (h->cfg.max_lines + 1), offsets, sizeof(int) * (n_lines + 1),
                     hipMemcpyHostToDevice));
  if (tot) RSPL_HIP(hipMemcpy(h->idx + (size_t)set * h->cap, idx, sizeof(int) * tot, hipMemcpyHostToDevice));
  RSPL_HIP(hipMemcpy(h->n_lines + set, &cnt[0], sizeof(int), hipMemcpyHostToDevice));
  RSPL_HIP(hipMemcpy(h->n_points + set, &cnt[1], sizeof(int), hipMemcpyHostToDevice));
  return RSPL_OK;
}

int run_match(rspl_lines* h, int problem, int set0, int set1, const int* matches, int n_matches, int n_points0,
              int n_points1) {
  RSPL_CHECK_ARG(n_matches >= 0 && n_matches <= h->cfg.max_matches, "n_matches %d outside [0, %d]", n_matches,
                 h->cfg.max_matches);
  for (int m = 0; m < n_matches; m++)
    RSPL_CHECK_ARG(matches[2 * m] >= 0 && matches[2 * m] < n_points0 && matches[2 * m + 1] >= 0 &&
                       matches[2 * m + 1] < n_points1,
                   "match %d (%d, %d) outside the keypoint ranges", m, matches[2 * m], matches[2 * m + 1]);
  const size_t Mm = std::max(1, h->cfg.max_matches);
  if (n_matches)
    RSPL_HIP(hipMemcpy(h->matches + problem * Mm * 2, matches, sizeof(int) * 2 * n_matches, hipMemcpyHostToDevice));
  RSPL_HIP(hipMemcpy(h->n_matches + problem, &n_matches, sizeof(int), hipMemcpyHostToDevice));
  lines::MatchArgs a{};
  a.off0 = a.off1 = h->offsets; a.idx0 = a.idx1 = h->idx; a.n_lines0 = a.n_lines1 = h->n_lines;
  a.n_points0 = a.n_points1 = h->n_points; a.set0 = set0; a.set1 = set1; a.step0 = a.step1 = 0;
  a.matches = h->matches + problem * Mm * 2; a.n_matches = h->n_matches + problem; a.max_lines = h->cfg.max_lines;
  a.cap = h->cap; a.max_matches = (int)Mm; a.M = h->M + (size_t)problem * h->cfg.max_lines * h->cfg.max_lines;
  a.inv = h->inv + (size_t)problem * 2 * h->cap; a.out = h->out + (size_t)problem * h->cfg.max_lines;
  a.status = nullptr;  // host calls check the assignment status themselves
  RSPL_HIP(lines::match(a, 1, h->stream));
  RSPL_HIP(hipStreamSynchronize(h->stream));
  (void)n_points0;
  (void)n_points1;
  return RSPL_OK;
}

}  // namespace

extern "C" int rspl_lines_assign(rspl_lines* h, const double* lines, int n_lines, const double* features, int n_points,
                                 int* offsets, int* point_idx, double* dist, int capacity) {
  RSPL_CHECK_ARG(h && offsets && (capacity == 0 || (point_idx && dist)), "rspl_lines_assign: NULL argument");
  if (int rc = stage_image(h, 0, lines, n_lines, features, n_points)) return rc;
  if (int rc = run_assign(h, 1)) return rc;
  return read_assignment(h, 0, n_lines, offsets, point_idx, dist, capacity);
}

extern "C" int rspl_lines_match(rspl_lines* h, const int* offsets0, const int* idx0, int n_lines0, const int* offsets1,
                                const int* idx1, int n_lines1, const int* matches, int n_matches, int n_points0,
                                int n_points1, int* line_matches) {
  RSPL_CHECK_ARG(h && offsets0 && offsets1 && (n_matches == 0 || matches) && (n_lines0 == 0 || line_matches),
                 "rspl_lines_match: NULL argument");
  if (int rc = stage_assignment(h, 0, offsets0, idx0, n_lines0, n_points0)) return rc;
  if (int rc = stage_assignment(h, 1, offsets1, idx1, n_lines1, n_points1)) return rc;
  if (int rc = run_match(h, 0, 0, 1, matches, n_matches, n_points0, n_points1)) return rc;
  if (n_lines0) RSPL_HIP(hipMemcpy(line_matches, h->out, sizeof(int) * n_lines0, hipMemcpyDeviceToHost));
  return RSPL_OK;
}

extern "C" int rspl_lines_stereo(rspl_lines* h, const double* lines_left, int n_left, const double* features_left,
                                 int n_points_left, const double* lines_right, int n_right, const double* features_right,
                                 int n_points_right, const int* stereo_matches, int n_matches, const double* camera_limits,
                                 double* lines_right_out, uint8_t* lines_right_valid, int* n_kept_matches) {
  RSPL_CHECK_ARG(h && camera_limits && n_kept_matches && (n_left == 0 || (lines_right_out && lines_right_valid)),
                 "rspl_lines_stereo: NULL argument");
  RSPL_CHECK_ARG(n_matches >= 0 && (n_matches == 0 || stereo_matches), "bad stereo matches");
  // frame.cc:157-167: keep the stereo matches inside the disparity window
  const double min_x = camera_limits[0], max_x = camera_limits[1], max_y = camera_limits[2];
  std::vector<int> kept;
  kept.reserve((size_t)2 * n_matches);
  for (int m = 0; m < n_matches; m++) {
    const int q = stereo_matches[2 * m], t = stereo_matches[2 * m + 1];
    RSPL_CHECK_ARG(q >= 0 && q < n_points_left && t >= 0 && t < n_points_right, "stereo match %d out of range", m);
    const double dx = std::fabs(features_left[(size_t)259 * q + 1] - features_right[(size_t)259 * t + 1]);
    const double dy = std::fabs(features_left[(size_t)259 * q + 2] - features_right[(size_t)259 * t + 2]);
    if (dx > min_x && dx < max_x && dy <= max_y) {
      kept.push_back(q);
      kept.push_back(t);
    }
  }
  *n_kept_matches = (int)kept.size() / 2;
  // frame.cc:128, 181: both images' assignments in one launch; :188 MatchLines
  if (int rc = stage_image(h, 0, lines_left, n_left, features_left, n_points_left)) return rc;
  if (int rc = stage_image(h, 1, lines_right, n_right, features_right, n_points_right)) return rc;
  if (int rc = run_assign(h, 2)) return rc;
  if (int rc = run_match(h, 0, 0, 1, kept.data(), (int)kept.size() / 2, n_points_left, n_points_right)) return rc;
  std::vector<int> lm((size_t)n_left);
  if (n_left) RSPL_HIP(hipMemcpy(lm.data(), h->out, sizeof(int) * n_left, hipMemcpyDeviceToHost));
  // frame.cc:189-196 (a match to right line 0 counts as invalid, as in the reference)
  for (int i = 0; i < n_left; i++) {
    const bool ok = lm[i] > 0;
    lines_right_valid[i] = ok ? 1 : 0;
    for (int k = 0; k < 4; k++) lines_right_out[4 * i + k] = ok ? lines_right[4 * lm[i] + k] : 0.0;
  }
  return RSPL_OK;
}

// Device-resident form of rspl_lines_stereo for a GPU pipeline: SuperPoint's device features and
// counts (image 0 = left, 1 = right) and SuperGlue's device match index of each left keypoint go in,
// per left line the right line and its validity come out, all stream-ordered (no host copy, no
// synchronisation).  An assignment that overflows max_pairs leaves every left line unmatched;
// rspl_lines_status reports it after the stream has completed.
extern "C" int rspl_lines_stereo_device(rspl_lines* h, const double* d_lines_left, int n_left,
                                        const double* d_lines_right, int n_right, const double* d_features,
                                        int feat_cap, const int32_t* d_counts, const int32_t* d_match_idx,
                                        const double* camera_limits, double* d_lines_right_out,
                                        uint8_t* d_lines_right_valid, void* stream) {
  RSPL_CHECK_ARG(h && d_features && d_counts && d_match_idx && camera_limits && (n_left == 0 || d_lines_left) &&
                     (n_right == 0 || d_lines_right) && (n_left == 0 || (d_lines_right_out && d_lines_right_valid)),
                 "rspl_lines_stereo_device: NULL argument");
  RSPL_CHECK_ARG(n_left >= 0 && n_left <= h->cfg.max_lines && n_right >= 0 && n_right <= h->cfg.max_lines,
                 "line counts outside [0, %d]", h->cfg.max_lines);
  RSPL_CHECK_ARG(feat_cap > 0 && feat_cap <= h->cfg.max_points, "feat_cap outside [1, %d]", h->cfg.max_points);
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const size_t L = h->cfg.max_lines;
  if (n_left)
    RSPL_HIP(hipMemcpyAsync(h->lines, d_lines_left, sizeof(double) * 4 * n_left, hipMemcpyDeviceToDevice, st));
  if (n_right)
    RSPL_HIP(hipMemcpyAsync(h->lines + L * 4, d_lines_right, sizeof(double) * 4 * n_right, hipMemcpyDeviceToDevice, st));
  RSPL_HIP(lines::set_counts(h->n_lines, n_left, n_right, h->n_points, d_counts, h->n_matches, st));
  lines::AssignArgs a{};
  a.lines = h->lines; a.n_lines = h->n_lines; a.pts = d_features; a.pt_batch = (size_t)feat_cap * 259;
  a.pt_stride = 259; a.pt_xoff = 1; a.n_points = h->n_points; a.offsets = h->offsets; a.idx = h->idx;
  a.dist = h->dist; a.max_lines = h->cfg.max_lines; a.cap = h->cap; a.status = h->status;
  RSPL_HIP(lines::assign(a, 2, st));
  lines::StereoArgs sa{};
  sa.idx = d_match_idx; sa.n_points = h->n_points; sa.pts = d_features; sa.pt_batch = (size_t)feat_cap * 259;
  sa.stride = 259; sa.xoff = 1; sa.min_x = camera_limits[0]; sa.max_x = camera_limits[1]; sa.max_y = camera_limits[2];
  sa.matches = h->matches; sa.n_out = h->n_matches; sa.status = h->status + 2;
  sa.max_matches = std::max(1, h->cfg.max_matches);
  RSPL_HIP(lines::stereo_filter(sa, feat_cap, st));
  lines::MatchArgs m{};
  m.off0 = m.off1 = h->offsets; m.idx0 = m.idx1 = h->idx; m.n_lines0 = m.n_lines1 = h->n_lines;
  m.n_points0 = m.n_points1 = h->n_points; m.set0 = 0; m.set1 = 1; m.step0 = m.step1 = 0;
  m.matches = h->matches; m.n_matches = h->n_matches; m.max_lines = h->cfg.max_lines; m.cap = h->cap;
  m.max_matches = std::max(1, h->cfg.max_matches); m.M = h->M; m.inv = h->inv; m.out = h->out; m.status = h->status;
  RSPL_HIP(lines::match(m, 1, st));
  lines::RightArgs r{};
  r.line_matches = h->out; r.lines_right = h->lines + L * 4; r.n_lines = h->n_lines; r.out = d_lines_right_out;
  r.valid = d_lines_right_valid;
  RSPL_HIP(lines::right_lines(r, std::max(1, n_left), st));
  return RSPL_OK;
}

extern "C" int rspl_lines_status(rspl_lines* h, int* overflow) {
  RSPL_CHECK_ARG(h && overflow, "rspl_lines_status: NULL argument");
  int st[3] = {0, 0, 0};
  RSPL_HIP(hipMemcpy(st, h->status, sizeof(st), hipMemcpyDeviceToHost));
  *overflow = st[0] | st[1] | st[2];
  return RSPL_OK;
}
