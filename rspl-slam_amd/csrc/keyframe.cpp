// Keyframe-builder handle: C ABI (include/rspl.h, rspl_kf_*) over kf_kernels.hip.  Mirrors what the
// reference does on the host between SuperGlue's stereo pair and the map -- MapBuilder::InsertKeyframe
// (src/map_builder.cc:639-682), Frame::AddRightFeatures (src/frame.cc:150-177) and the map-point half of
// Map::InsertKeyframe (src/map.cc:40-55) -- for a batch of independent frames as one launch behind
// SuperGlue on the caller's stream, and Map::TriangulateMappoint (src/map.cc:292-339) as one batched call.
// All memory is host-mapped and allocated at create: the per-frame records and host arrays in, the results
// out; the kernels touch device memory only through the caller's pointers.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "kf_kernels.hpp"
#include "kf_triangulate.hpp"

using namespace rspl;

struct rspl_kf {
  rspl_kf_config cfg{};
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  PinnedArena pinned;
  kf::Args a{};
  // host-mapped (pieces of `pinned`): the per-frame records and the frames' host arrays in ...
  kf::Param* params = nullptr;
  int32_t *s_tid = nullptr, *s_slot = nullptr;
  double* s_points = nullptr;
  uint8_t* s_state = nullptr;
  int32_t *d_tid = nullptr, *d_slot = nullptr;  // their device addresses
  double* d_points = nullptr;
  uint8_t* d_state = nullptr;
  // ... the results out
  kf::Out* out = nullptr;
  double *u_right = nullptr, *depth = nullptr, *new_position = nullptr;
  int32_t* track_id = nullptr;
  uint8_t* new_point = nullptr;
  // triangulation staging (one area) and its device address
  char* tri = nullptr;
  char* tri_dev = nullptr;
  bool pending = false;
  int batch = 0;
};

namespace {

struct TriLayout {  // the triangulation staging for np poses, n points, m observations
  size_t poses, offsets, obs_pose, obs_xy, position, status, bytes;
  TriLayout(size_t np, size_t n, size_t m) {
    size_t o = 0;
    auto take = [&](size_t b) {
      const size_t at = o;
      o = al256(o + b);
      return at;
    };
    poses = take(16 * sizeof(double) * np);
    offsets = take(sizeof(int32_t) * (n + 1));
    obs_pose = take(sizeof(int32_t) * m);
    obs_xy = take(2 * sizeof(double) * m);
    position = take(3 * sizeof(double) * n);
    status = take(n);
    bytes = o;
  }
};

}  // namespace

extern "C" int rspl_kf_create(const rspl_kf_config* cfg, rspl_kf** out) {
  RSPL_CHECK_ARG(cfg && out, "rspl_kf_create: NULL argument");
  *out = nullptr;
  RSPL_CHECK_ARG(cfg->max_batch > 0 && cfg->max_keypoints > 0, "rspl_kf_create: max_batch %d, max_keypoints %d",
                 cfg->max_batch, cfg->max_keypoints);
  RSPL_CHECK_ARG(cfg->max_tri_points >= 0 && cfg->max_tri_observations >= 0,
                 "rspl_kf_create: max_tri_points %d, max_tri_observations %d", cfg->max_tri_points,
                 cfg->max_tri_observations);
  RSPL_CHECK_ARG((size_t)cfg->max_batch * cfg->max_keypoints <= (size_t)1 << 28 &&
                     cfg->max_tri_points <= 1 << 24 && cfg->max_tri_observations <= 1 << 26,
                 "rspl_kf_create: capacities too large");
  RSPL_HIP(hipSetDevice(cfg->device));
  auto* h = new rspl_kf();
  h->cfg = *cfg;
  const size_t B = cfg->max_batch, E = B * cfg->max_keypoints;
  // (a pose per observation is the most a triangulation batch can reference)
  const TriLayout lay(cfg->max_tri_observations, cfg->max_tri_points, cfg->max_tri_observations);
  kf::Args& a = h->a;
  auto carve = [&](auto& P) {
    h->params = P.template take<kf::Param>(B, &a.params);
    h->s_tid = P.template take<int32_t>(E, &h->d_tid);
    h->s_slot = P.template take<int32_t>(E, &h->d_slot);
    h->s_points = P.template take<double>(3 * E, &h->d_points);
    h->s_state = P.template take<uint8_t>(E, &h->d_state);
    h->out = P.template take<kf::Out>(B, &a.out);
    h->u_right = P.template take<double>(E, &a.u_right);
    h->depth = P.template take<double>(E, &a.depth);
    h->track_id = P.template take<int32_t>(E, &a.track_id);
    h->new_point = P.template take<uint8_t>(E, &a.new_point);
    h->new_position = P.template take<double>(3 * E, &a.new_position);
    h->tri = P.template take<char>(lay.bytes, &h->tri_dev);
  };
  Sizer psz;
  carve(psz);
  bool ok = h->pinned.reserve(psz.used + 256) == RSPL_OK;
  if (ok) carve(h->pinned);
  ok = ok && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
       hipEventCreateWithFlags(&h->done, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    set_error("rspl_kf_create: stream / event / pinned allocation failed");
    rspl_kf_destroy(h);
    return RSPL_E_DEVICE;
  }
  a.K = cfg->max_keypoints;
  *out = h;
  return RSPL_OK;
}

extern "C" void rspl_kf_destroy(rspl_kf* h) {
  if (!h) return;
  if (h->pending && h->done) (void)hipEventSynchronize(h->done);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->pinned.release();
  if (h->done) (void)hipEventDestroy(h->done);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int rspl_kf_enqueue(rspl_kf* h, int batch, const rspl_kf_frame* frames, void* stream) {
  RSPL_CHECK_ARG(h && (batch == 0 || frames), "rspl_kf_enqueue: NULL argument");
  RSPL_CHECK_ARG(batch >= 0 && batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
  RSPL_CHECK_ARG(!h->pending, "rspl_kf_enqueue: the previous enqueue has not been fetched");
  const size_t K = h->cfg.max_keypoints;
  for (int b = 0; b < batch; b++) {
    const rspl_kf_frame& fr = frames[b];
    RSPL_CHECK_ARG(fr.d_features_left && fr.d_features_right && fr.d_n_left && fr.d_n_right && fr.d_idx0 && fr.d_idx1,
                   "frame %d: NULL device pointer", b);
    RSPL_CHECK_ARG(fr.n >= 0 && (size_t)fr.n <= K, "frame %d: n %d exceeds max_keypoints %zu", b, fr.n, K);
    RSPL_CHECK_ARG(!fr.point_slot || fr.n == 0 || (fr.points && fr.state),
                   "frame %d: point_slot without points / state", b);
    bool finite = std::isfinite(fr.fx) && std::isfinite(fr.fy) && std::isfinite(fr.cx) && std::isfinite(fr.cy) &&
                  std::isfinite(fr.bf) && std::isfinite(fr.min_x_diff) && std::isfinite(fr.max_x_diff) &&
                  std::isfinite(fr.max_y_diff);
    for (int k = 0; k < 12; k++) finite = finite && std::isfinite(fr.Twc[k]);
    RSPL_CHECK_ARG(finite && fr.fx != 0 && fr.fy != 0, "frame %d: bad camera, window or pose", b);
    RSPL_CHECK_ARG(fr.next_track_id >= 0 && (fr.init == 0 || fr.init == 1), "frame %d: next_track_id %d, init %d", b,
                   fr.next_track_id, fr.init);
    const int nt = (fr.d_table_points != nullptr) + (fr.d_table_state != nullptr) + (fr.d_table_track_id != nullptr);
    RSPL_CHECK_ARG(nt == 0 || (nt == 3 && fr.table_capacity > 0),
                   "frame %d: the keyframe table needs its three arrays and a capacity", b);
  }
  if (batch == 0) return RSPL_OK;
  for (int b = 0; b < batch; b++) {
    const rspl_kf_frame& fr = frames[b];
    kf::Param& P = h->params[b];
    const size_t o = K * b, n = (size_t)fr.n;
    P.feat_l = fr.d_features_left;
    P.feat_r = fr.d_features_right;
    P.n_l = fr.d_n_left;
    P.n_r = fr.d_n_right;
    P.idx0 = fr.d_idx0;
    P.idx1 = fr.d_idx1;
    // the host arrays are copied before the call returns; the kernel reads them from the pinned staging
    P.track_id = P.point_slot = nullptr;
    P.points = nullptr;
    P.state = nullptr;
    if (fr.track_id && n) {
      memcpy(h->s_tid + o, fr.track_id, sizeof(int32_t) * n);
      P.track_id = h->d_tid + o;
    }
    if (fr.point_slot && n) {
      memcpy(h->s_slot + o, fr.point_slot, sizeof(int32_t) * n);
      memcpy(h->s_points + 3 * o, fr.points, 3 * sizeof(double) * n);
      memcpy(h->s_state + o, fr.state, n);
      P.point_slot = h->d_slot + o;
      P.points = h->d_points + 3 * o;
      P.state = h->d_state + o;
    }
    P.tbl_points = fr.d_table_points;
    P.tbl_state = fr.d_table_state;
    P.tbl_tid = fr.d_table_track_id;
    P.cam[0] = fr.fx; P.cam[1] = fr.fy; P.cam[2] = fr.cx; P.cam[3] = fr.cy; P.cam[4] = fr.bf;
    P.win[0] = fr.min_x_diff; P.win[1] = fr.max_x_diff; P.win[2] = fr.max_y_diff;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) P.Twc[3 * r + c] = fr.Twc[4 * r + c];
      P.Twc[9 + r] = fr.Twc[4 * r + 3];
    }
    P.next_track_id = fr.next_track_id;
    P.init = fr.init;
    P.n_host = fr.n;
    P.tbl_cap = fr.d_table_points ? fr.table_capacity : 0;
  }
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  RSPL_HIP(kf::stereo(h->a, batch, st));
  RSPL_HIP(hipEventRecord(h->done, st));
  h->pending = true;
  h->batch = batch;
  return RSPL_OK;
}

extern "C" int rspl_kf_fetch(rspl_kf* h, rspl_kf_result* res) {
  RSPL_CHECK_ARG(h && res, "rspl_kf_fetch: NULL argument");
  RSPL_CHECK_ARG(h->pending, "rspl_kf_fetch: nothing was enqueued");
  RSPL_HIP(hipEventSynchronize(h->done));
  h->pending = false;
  const size_t K = h->cfg.max_keypoints;
  for (int b = 0; b < h->batch; b++) {
    const kf::Out& o = h->out[b];
    rspl_kf_result& r = res[b];
    r.n_keypoints = o.n_keypoints;
    r.n_matches = o.n_matches;
    r.n_stereo_matches = o.n_stereo_matches;
    r.n_new_ids = o.n_new_ids;
    r.n_new_points = o.n_new_points;
    r.n_new_good = o.n_new_good;
    r.next_track_id = o.next_track_id;
    const size_t n = (size_t)std::min<int>(std::max(o.n_keypoints, 0), (int)K), at = K * b;
    if (r.u_right) memcpy(r.u_right, h->u_right + at, sizeof(double) * n);
    if (r.depth) memcpy(r.depth, h->depth + at, sizeof(double) * n);
    if (r.track_id) memcpy(r.track_id, h->track_id + at, sizeof(int32_t) * n);
    if (r.new_point) memcpy(r.new_point, h->new_point + at, n);
    if (r.new_position) memcpy(r.new_position, h->new_position + 3 * at, 3 * sizeof(double) * n);
  }
  return RSPL_OK;
}

extern "C" int rspl_kf_triangulate(rspl_kf* h, int n_poses, const double* Twc, const double* camera, int n_points,
                                   const int32_t* offsets, const int32_t* obs_pose, const double* obs_xy,
                                   double* position, uint8_t* status) {
  RSPL_CHECK_ARG(n_points >= 0 && n_poses >= 0, "rspl_kf_triangulate: negative sizes");
  if (n_points == 0) return RSPL_OK;
  RSPL_CHECK_ARG(camera && offsets && position && status, "rspl_kf_triangulate: NULL argument");
  RSPL_CHECK_ARG(std::isfinite(camera[0]) && std::isfinite(camera[1]) && camera[0] != 0 && camera[1] != 0,
                 "rspl_kf_triangulate: bad camera");
  RSPL_CHECK_ARG(offsets[0] == 0, "rspl_kf_triangulate: offsets[0] != 0");
  for (int i = 0; i < n_points; i++)
    RSPL_CHECK_ARG(offsets[i + 1] >= offsets[i], "rspl_kf_triangulate: offsets decrease at point %d", i);
  const int m = offsets[n_points];
  RSPL_CHECK_ARG(m == 0 || (obs_pose && obs_xy && (Twc || n_poses == 0)), "rspl_kf_triangulate: NULL observer arrays");
  for (int k = 0; k < m; k++)
    RSPL_CHECK_ARG(obs_pose[k] < n_poses, "rspl_kf_triangulate: observer %d names pose %d of %d", k, obs_pose[k], n_poses);
  if (!h) {  // the host instantiation of the same routine
    for (int i = 0; i < n_points; i++) {
      const int o = offsets[i];
      status[i] = (uint8_t)kf::triangulate_point(Twc, obs_pose + o, obs_xy + 2 * (size_t)o, offsets[i + 1] - o, camera,
                                                 position + 3 * (size_t)i, nullptr);
    }
    return RSPL_OK;
  }
  RSPL_CHECK_ARG(!h->pending, "rspl_kf_triangulate: an enqueue is in flight, fetch it first");
  if (n_points > h->cfg.max_tri_points || m > h->cfg.max_tri_observations || n_poses > h->cfg.max_tri_observations) {
    set_error("rspl_kf_triangulate: %d points / %d observations / %d poses, capacity %d / %d / %d", n_points, m, n_poses,
              h->cfg.max_tri_points, h->cfg.max_tri_observations, h->cfg.max_tri_observations);
    return RSPL_E_CAPACITY;
  }
  const TriLayout lay(n_poses, n_points, m);
  char* sg = h->tri;
  if (n_poses) memcpy(sg + lay.poses, Twc, 16 * sizeof(double) * n_poses);
  memcpy(sg + lay.offsets, offsets, sizeof(int32_t) * (n_points + 1));
  if (m) {
    memcpy(sg + lay.obs_pose, obs_pose, sizeof(int32_t) * m);
    memcpy(sg + lay.obs_xy, obs_xy, 2 * sizeof(double) * m);
  }
  kf::TriArgs t{};
  const char* dv = h->tri_dev;
  t.Twc = reinterpret_cast<const double*>(dv + lay.poses);
  t.offsets = reinterpret_cast<const int32_t*>(dv + lay.offsets);
  t.obs_pose = reinterpret_cast<const int32_t*>(dv + lay.obs_pose);
  t.obs_xy = reinterpret_cast<const double*>(dv + lay.obs_xy);
  for (int k = 0; k < 4; k++) t.cam[k] = camera[k];
  t.n = n_points;
  t.position = reinterpret_cast<double*>(h->tri_dev + lay.position);
  t.status = reinterpret_cast<uint8_t*>(h->tri_dev + lay.status);
  RSPL_HIP(kf::triangulate(t, h->stream));
  RSPL_HIP(hipStreamSynchronize(h->stream));
  memcpy(position, sg + lay.position, 3 * sizeof(double) * n_points);
  memcpy(status, sg + lay.status, n_points);
  return RSPL_OK;
}
