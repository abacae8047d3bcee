// Local map tracking handle: C ABI (include/rspl.h, rspl_lmap_*) over lmap_kernels.hip.  Mirrors
// Map::SearchByProjection (src/map.cc:952-1005) and MapBuilder::TrackLocalMap (src/map_builder.cc:753-785) -- code
// the reference keeps but never calls -- for a batch of independent frames: a descriptor bank keyed by map point
// id, the ordered local map resolved to bank rows on the host, and search | merge | the tracking chain of
// rspl_track_enqueue as one stream-ordered sequence with no host work in between.
// rspl_lmap_debug_search_host is the host instantiation of the search text (lmap_match.hpp).
// rspl_lmap_global_* (lmap_reloc.cpp) is the second reader of the bank; the handle is lmap_handle.hpp's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "lmap_handle.hpp"

using namespace rspl;

namespace {

bool good_frame(const rspl_lmap_frame& fr) {
  bool fin = std::isfinite(fr.fx) && std::isfinite(fr.fy) && std::isfinite(fr.cx) && std::isfinite(fr.cy) &&
             std::isfinite(fr.bf);
  for (int k = 0; k < 12; k++) fin = fin && std::isfinite(fr.Twc[k]);
  return fin && fr.width > 0 && fr.height > 0;
}

// rows for ids[0 .. n): existing ids keep theirs, new ones take the next free rows (`fresh`).  Nothing is committed
// here: the caller adds `fresh` to the bank's table once the rows have been filled (or their fill enqueued).
int assign_rows(rspl_lmap* h, const char* who, int n, const int32_t* ids, std::vector<int>& rows,
                std::unordered_map<int, int>& fresh) {
  rows.resize(n);
  int next = (int)h->row_of.size();
  for (int k = 0; k < n; k++) {
    RSPL_CHECK_ARG(ids[k] >= 0, "%s: map point id %d is negative", who, ids[k]);
    auto it = h->row_of.find(ids[k]);
    if (it != h->row_of.end()) {
      rows[k] = it->second;
      continue;
    }
    auto fr = fresh.find(ids[k]);
    if (fr == fresh.end()) fr = fresh.emplace(ids[k], next++).first;
    rows[k] = fr->second;
  }
  if (next > h->cfg.max_bank_points) {
    set_error("%s: the bank holds %d descriptors, %d more do not fit its %d rows", who, (int)h->row_of.size(),
              (int)fresh.size(), h->cfg.max_bank_points);
    return RSPL_E_CAPACITY;
  }
  return RSPL_OK;
}

// the per-frame parameters of an enqueue; slots: the tracker's tables (or null)
void fill_params(rspl_lmap* h, int batch, const rspl_lmap_frame* frames, double* const* kp, uint8_t* const* ks,
                 int32_t* const* kt) {
  for (int b = 0; b < batch; b++) {
    const rspl_lmap_frame& fr = frames[b];
    lmap::Param& P = h->params[b];
    P.feat = fr.d_features;
    P.n1 = fr.d_n1;
    P.u_right = fr.d_u_right;
    P.pid = fr.d_point_id;
    P.pxyz = fr.d_point_xyz;
    P.pgood = fr.d_point_good;
    P.kf_points = kp ? kp[b] : nullptr;
    P.kf_state = ks ? ks[b] : nullptr;
    P.kf_tid = kt ? kt[b] : nullptr;
    lmap::make_view(fr.Twc, fr.fx, fr.fy, fr.cx, fr.cy, fr.bf, fr.width, fr.height, h->cfg.radius, h->cfg.max_distance,
                    h->cfg.max_ratio, P.V);
  }
}

int check_enqueue(rspl_lmap* h, int batch, const rspl_lmap_frame* frames, const char* who) {
  RSPL_CHECK_ARG(h && (batch == 0 || frames), "%s: NULL argument", who);
  RSPL_CHECK_ARG(!h->host_only, "%s: a host-only handle (device < 0) has no device side", who);
  RSPL_CHECK_ARG(batch >= 0 && batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
  RSPL_CHECK_ARG(!h->pending, "%s: the previous enqueue has not been fetched", who);
  for (int b = 0; b < batch; b++) {
    const rspl_lmap_frame& fr = frames[b];
    RSPL_CHECK_ARG(fr.d_features && fr.d_n1 && fr.d_point_id && fr.d_point_xyz, "frame %d: NULL device pointer", b);
    RSPL_CHECK_ARG(good_frame(fr), "frame %d: bad camera, pose or image size", b);
  }
  return RSPL_OK;
}

}  // namespace

extern "C" int rspl_lmap_create(const rspl_lmap_config* cfg, rspl_lmap** out) {
  RSPL_CHECK_ARG(cfg && out, "rspl_lmap_create: NULL argument");
  *out = nullptr;
  RSPL_CHECK_ARG(cfg->max_bank_points > 0 && cfg->max_local_points > 0 && cfg->max_keypoints > 0 && cfg->max_batch > 0,
                 "rspl_lmap_create: max_bank_points %d, max_local_points %d, max_keypoints %d, max_batch %d",
                 cfg->max_bank_points, cfg->max_local_points, cfg->max_keypoints, cfg->max_batch);
  RSPL_CHECK_ARG(cfg->max_keypoints <= lmap::kMaxKeypoints, "rspl_lmap_create: max_keypoints %d exceeds the %d a merge workgroup holds",
                 cfg->max_keypoints, lmap::kMaxKeypoints);
  RSPL_CHECK_ARG((size_t)cfg->max_bank_points <= (size_t)1 << 22 && (size_t)cfg->max_batch * cfg->max_keypoints <= (size_t)1 << 26 &&
                     (size_t)cfg->max_batch * cfg->max_local_points <= (size_t)1 << 26,
                 "rspl_lmap_create: capacities too large");
  RSPL_CHECK_ARG(std::isfinite(cfg->radius) && cfg->radius > 0 && std::isfinite(cfg->max_distance) &&
                     std::isfinite(cfg->max_ratio),
                 "rspl_lmap_create: bad radius / thresholds");
  auto* h = new rspl_lmap();
  h->cfg = *cfg;
  h->host_only = cfg->device < 0;
  const size_t B = cfg->max_batch, K = cfg->max_keypoints, L = cfg->max_local_points, NB = cfg->max_bank_points;
  if (h->host_only) {
    h->host_bank.assign(NB * lmap::kDesc, 0.0);
    *out = h;
    return RSPL_OK;
  }
  if (hipSetDevice(cfg->device) != hipSuccess) {
    set_error("rspl_lmap_create: hipSetDevice(%d) failed", cfg->device);
    delete h;
    return RSPL_E_DEVICE;
  }
  lmap::Args& a = h->a;
  auto carve = [&](auto& A, auto& P) {
    h->params = P.template take<lmap::Param>(B, &a.host_params);
    h->out = P.template take<lmap::Out>(B, &a.out);
    h->o_good_kp = P.template take<int32_t>(B * L, &a.o_good_kp);
    h->o_good_point = P.template take<int32_t>(B * L, &a.o_good_point);
    h->o_assoc = P.template take<int32_t>(B * K, &a.o_assoc);
    h->s_local_row = P.template take<int32_t>(L, &h->s_local_row_dev);
    h->s_local_id = P.template take<int32_t>(L, &h->s_local_id_dev);
    h->s_local_pos = P.template take<double>(3 * L, &h->s_local_pos_dev);
    h->s_pairs = P.template take<int32_t>(2 * NB, &h->s_pairs_dev);
    h->bank = A.template take<double>(NB * lmap::kDesc);
    h->d_local_row = A.template take<int32_t>(L);
    h->d_local_id = A.template take<int32_t>(L);
    h->d_local_pos = A.template take<double>(3 * L);
    a.params = A.template take<lmap::Param>(B);
    a.kx = A.template take<double>(B * K);
    a.ky = A.template take<double>(B * K);
    a.kur = A.template take<double>(B * K);
    a.kkey = A.template take<int32_t>(B * K);
    a.n1c = A.template take<int32_t>(B);
    a.status = A.template take<int32_t>(B * L);
    a.best_idx = A.template take<int32_t>(B * L);
    a.best = A.template take<double>(B * L);
    a.second = A.template take<double>(B * L);
    a.good_kp = A.template take<int32_t>(B * L);
    a.good_point = A.template take<int32_t>(B * L);
    a.assoc = A.template take<int32_t>(B * K);
    a.idx0 = A.template take<int32_t>(B * K);
    a.idx1 = A.template take<int32_t>(B * K);
  };
  Sizer sz, psz;
  carve(sz, psz);
  int rc = h->arena.reserve(sz.used + 256);
  if (!rc) rc = h->pinned.reserve(psz.used + 256);
  if (rc) {
    rspl_lmap_destroy(h);
    return rc;
  }
  carve(h->arena, h->pinned);
  bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&h->done, kHostEventFlags) == hipSuccess &&
            hipEventCreateWithFlags(&h->store_ev, kOrderEventFlags) == hipSuccess &&
            hipEventCreateWithFlags(&h->local_ev, kOrderEventFlags) == hipSuccess;
  // (zeroed once so that a bank row never stored and a debug read-back of slots no kernel wrote are defined)
  ok = ok && hipMemset(h->arena.base, 0, h->arena.used) == hipSuccess;
  if (!ok) {
    set_error("rspl_lmap_create: stream / event allocation failed");
    rspl_lmap_destroy(h);
    return RSPL_E_DEVICE;
  }
  a.K = (int)K;
  a.L = (int)L;
  a.bank = h->bank;
  a.local_row = h->d_local_row;
  a.local_id = h->d_local_id;
  a.local_pos = h->d_local_pos;
  *out = h;
  return RSPL_OK;
}

extern "C" void rspl_lmap_destroy(rspl_lmap* h) {
  if (!h) return;
  if (h->pending && h->done) (void)hipEventSynchronize(h->done);
  if (h->store_ev) (void)hipEventSynchronize(h->store_ev);
  if (h->local_ev) (void)hipEventSynchronize(h->local_ev);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->arena.release();
  h->pinned.release();
  h->g_arena.release();
  h->g_pinned.release();
  for (hipEvent_t e : {h->done, h->store_ev, h->local_ev})
    if (e) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int rspl_lmap_store(rspl_lmap* h, int n, const int32_t* ids, const int32_t* keypoints,
                               const double* d_features, void* stream) {
  RSPL_CHECK_ARG(h && (n == 0 || (ids && keypoints && d_features)), "rspl_lmap_store: NULL argument");
  RSPL_CHECK_ARG(!h->host_only, "rspl_lmap_store: a host-only handle (device < 0) has no device side");
  RSPL_CHECK_ARG(n >= 0 && n <= h->cfg.max_bank_points, "rspl_lmap_store: n %d outside [0, %d]", n,
                 h->cfg.max_bank_points);
  for (int k = 0; k < n; k++) RSPL_CHECK_ARG(keypoints[k] >= 0, "rspl_lmap_store: keypoint %d is negative", keypoints[k]);
  if (n == 0) return RSPL_OK;
  std::vector<int> rows;
  std::unordered_map<int, int> fresh;
  const int rc = assign_rows(h, "rspl_lmap_store", n, ids, rows, fresh);
  if (rc) return rc;
  // the staging may still feed the previous store's kernel: that launch (only it) is waited for
  RSPL_HIP(hipEventSynchronize(h->store_ev));
  for (int k = 0; k < n; k++) {
    h->s_pairs[2 * k] = rows[k];
    h->s_pairs[2 * k + 1] = keypoints[k];
  }
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  RSPL_HIP(lmap::store(h->bank, d_features, h->s_pairs_dev, n, st));
  RSPL_HIP(hipEventRecord(h->store_ev, st));
  h->row_of.insert(fresh.begin(), fresh.end());
  return RSPL_OK;
}

extern "C" int rspl_lmap_store_host(rspl_lmap* h, int n, const int32_t* ids, const double* descriptors) {
  RSPL_CHECK_ARG(h && (n == 0 || (ids && descriptors)), "rspl_lmap_store_host: NULL argument");
  RSPL_CHECK_ARG(n >= 0, "rspl_lmap_store_host: n %d is negative", n);
  if (n == 0) return RSPL_OK;
  std::vector<int> rows;
  std::unordered_map<int, int> fresh;
  const int rc = assign_rows(h, "rspl_lmap_store_host", n, ids, rows, fresh);
  if (rc) return rc;
  const size_t row_bytes = sizeof(double) * lmap::kDesc;
  for (int k = 0; k < n;) {  // runs of consecutive rows are one copy
    int e = k + 1;
    while (e < n && rows[e] == rows[e - 1] + 1) e++;
    const double* src = descriptors + (size_t)lmap::kDesc * k;
    if (h->host_only)
      memcpy(h->host_bank.data() + (size_t)lmap::kDesc * rows[k], src, row_bytes * (e - k));
    else
      RSPL_HIP(hipMemcpy(h->bank + (size_t)lmap::kDesc * rows[k], src, row_bytes * (e - k), hipMemcpyHostToDevice));
    k = e;
  }
  h->row_of.insert(fresh.begin(), fresh.end());
  return RSPL_OK;
}

extern "C" int rspl_lmap_bank_size(const rspl_lmap* h, int* n) {
  RSPL_CHECK_ARG(h && n, "rspl_lmap_bank_size: NULL argument");
  *n = (int)h->row_of.size();
  return RSPL_OK;
}

extern "C" int rspl_lmap_set_local(rspl_lmap* h, int n, const int32_t* ids, const double* positions, void* stream) {
  RSPL_CHECK_ARG(h && (n == 0 || (ids && positions)), "rspl_lmap_set_local: NULL argument");
  RSPL_CHECK_ARG(n >= 0 && n <= h->cfg.max_local_points, "rspl_lmap_set_local: n %d outside [0, %d]", n,
                 h->cfg.max_local_points);
  RSPL_CHECK_ARG(!h->pending, "rspl_lmap_set_local: an enqueue is in flight, fetch it first");
  std::vector<int32_t> rows(n);
  for (int k = 0; k < n; k++) {
    auto it = h->row_of.find(ids[k]);
    RSPL_CHECK_ARG(it != h->row_of.end(), "rspl_lmap_set_local: map point %d has no descriptor in the bank", ids[k]);
    rows[k] = it->second;
    for (int c = 0; c < 3; c++)
      RSPL_CHECK_ARG(std::isfinite(positions[3 * (size_t)k + c]), "rspl_lmap_set_local: map point %d: bad position",
                     ids[k]);
  }
  if (!h->host_only && n) {
    // the staging may still feed the previous upload: that copy (only it) is waited for
    RSPL_HIP(hipEventSynchronize(h->local_ev));
    memcpy(h->s_local_row, rows.data(), sizeof(int32_t) * n);
    memcpy(h->s_local_id, ids, sizeof(int32_t) * n);
    memcpy(h->s_local_pos, positions, sizeof(double) * 3 * n);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    RSPL_HIP(upload_mapped(h->d_local_row, h->s_local_row_dev, sizeof(int32_t) * n, st));
    RSPL_HIP(upload_mapped(h->d_local_id, h->s_local_id_dev, sizeof(int32_t) * n, st));
    RSPL_HIP(upload_mapped(h->d_local_pos, h->s_local_pos_dev, sizeof(double) * 3 * n, st));
    RSPL_HIP(hipEventRecord(h->local_ev, st));
  }
  h->local_ids.assign(ids, ids + n);
  h->n_local = n;
  return RSPL_OK;
}

extern "C" int rspl_lmap_enqueue(rspl_lmap* h, int batch, const rspl_lmap_frame* frames, void* stream) {
  const int rc = check_enqueue(h, batch, frames, "rspl_lmap_enqueue");
  if (rc) return rc;
  h->batch = batch;
  h->batch_local = h->n_local;
  if (batch == 0) return RSPL_OK;
  fill_params(h, batch, frames, nullptr, nullptr, nullptr);
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  RSPL_HIP(lmap::wait_uploads(h, st));
  RSPL_HIP(lmap::search(h->a, batch, h->n_local, st));
  RSPL_HIP(hipEventRecord(h->done, st));
  h->pending = true;
  return RSPL_OK;
}

extern "C" int rspl_lmap_track_enqueue(rspl_lmap* h, rspl_track* t, int batch, const rspl_lmap_frame* frames,
                                       const rspl_track_frame* tf, void* stream) {
  const int rc = check_enqueue(h, batch, frames, "rspl_lmap_track_enqueue");
  if (rc) return rc;
  RSPL_CHECK_ARG(t && (batch == 0 || tf), "rspl_lmap_track_enqueue: NULL argument");
  const int K = h->cfg.max_keypoints;
  std::vector<double*> kp(batch);
  std::vector<uint8_t*> ks(batch);
  std::vector<int32_t*> kt(batch);
  std::vector<rspl_track_frame> tfs(tf, tf + batch);
  for (int b = 0; b < batch; b++) {
    for (int c = 0; c < b; c++)
      RSPL_CHECK_ARG(tf[c].slot != tf[b].slot, "frames %d and %d share keyframe slot %d", c, b, tf[b].slot);
    // (checks the slot, the tracker's capacity against K and that no enqueue of the tracker is in flight)
    const int r = rspl_track_keyframe_table(t, tf[b].slot, K, &kp[b], &ks[b], &kt[b]);
    if (r) return r;
    tfs[b].d_idx0 = h->a.idx0 + (size_t)K * b;
    tfs[b].d_idx1 = h->a.idx1 + (size_t)K * b;
    // the count the search used (clamped to K by the prep kernel): the index slices above hold K entries, and the
    // tracker, whose capacity may be larger, would clamp the caller's count to its own
    tfs[b].d_n1 = h->a.n1c + b;
  }
  h->batch = batch;
  h->batch_local = h->n_local;
  if (batch == 0) return rspl_track_enqueue(t, 0, tf, stream);
  fill_params(h, batch, frames, kp.data(), ks.data(), kt.data());
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  RSPL_HIP(lmap::wait_uploads(h, st));
  RSPL_HIP(lmap::search(h->a, batch, h->n_local, st));
  RSPL_HIP(hipEventRecord(h->done, st));
  h->pending = true;
  return rspl_track_enqueue(t, batch, tfs.data(), st);
}

extern "C" int rspl_lmap_fetch(rspl_lmap* h, rspl_lmap_result* res) {
  RSPL_CHECK_ARG(h && (res || h->batch == 0), "rspl_lmap_fetch: NULL argument");
  RSPL_CHECK_ARG(!(h->pending && h->pending_global), "rspl_lmap_fetch: the enqueue in flight is a global one");
  if (h->pending) {
    RSPL_HIP(hipEventSynchronize(h->done));
    h->pending = false;
  }
  const size_t K = h->cfg.max_keypoints, L = h->cfg.max_local_points;
  for (int b = 0; b < h->batch; b++) {
    const lmap::Out& o = h->out[b];
    rspl_lmap_result& r = res[b];
    r.n_keypoints = o.n1;
    r.n_selected = o.n_selected;
    r.n_projected = o.n_projected;
    r.n_with_candidates = o.n_cand;
    r.n_good = o.n_good;
    const size_t ng = (size_t)std::min<int>(std::max(o.n_good, 0), (int)L);
    const size_t n1 = (size_t)std::min<int>(std::max(o.n1, 0), (int)K);
    if (r.good_kp) memcpy(r.good_kp, h->o_good_kp + L * b, sizeof(int32_t) * ng);
    if (r.good_point) memcpy(r.good_point, h->o_good_point + L * b, sizeof(int32_t) * ng);
    if (r.assoc_id) memcpy(r.assoc_id, h->o_assoc + K * b, sizeof(int32_t) * n1);
  }
  return RSPL_OK;
}

extern "C" int rspl_lmap_debug_points(rspl_lmap* h, int frame, int32_t* status, int32_t* best_idx, double* best,
                                      double* second) {
  RSPL_CHECK_ARG(h, "rspl_lmap_debug_points: NULL handle");
  RSPL_CHECK_ARG(!h->host_only, "rspl_lmap_debug_points: a host-only handle (device < 0) has no device side");
  RSPL_CHECK_ARG(!h->pending, "rspl_lmap_debug_points: fetch the enqueue first");
  RSPL_CHECK_ARG(frame >= 0 && frame < h->batch, "frame %d not in the last batch", frame);
  const size_t n = h->batch_local, o = (size_t)h->cfg.max_local_points * frame;
  auto get = [](void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  };
  RSPL_HIP(get(status, h->a.status + o, sizeof(int32_t) * n));
  RSPL_HIP(get(best_idx, h->a.best_idx + o, sizeof(int32_t) * n));
  RSPL_HIP(get(best, h->a.best + o, sizeof(double) * n));
  RSPL_HIP(get(second, h->a.second + o, sizeof(double) * n));
  return RSPL_OK;
}

extern "C" int rspl_lmap_debug_search_host(const rspl_lmap_host_problem* p, int32_t* status, int32_t* best_idx,
                                           double* best, double* second) {
  RSPL_CHECK_ARG(p && status && best_idx && best && second, "rspl_lmap_debug_search_host: NULL argument");
  RSPL_CHECK_ARG(p->n_keypoints >= 0 && p->n_local >= 0 && p->width > 0 && p->height > 0,
                 "rspl_lmap_debug_search_host: bad sizes");
  RSPL_CHECK_ARG((p->n_keypoints == 0 || (p->features && p->point_id)) &&
                     (p->n_local == 0 || (p->local_ids && p->local_pos && p->local_desc)),
                 "rspl_lmap_debug_search_host: NULL array");
  lmap::View V;
  lmap::make_view(p->Twc, p->fx, p->fy, p->cx, p->cy, p->bf, p->width, p->height, p->radius, p->max_distance,
                  p->max_ratio, V);
  const int n1 = p->n_keypoints;
  // the prep kernel's arrays
  std::vector<double> kx(n1), ky(n1), kur(n1);
  std::vector<int> key(n1);
  for (int i = 0; i < n1; i++) {
    const double* r = p->features + RSPL_FEATURE_ROWS * (size_t)i;
    key[i] = p->point_id[i] < 0 ? lmap::cell_key(r[1], r[2], V.inv_w, V.inv_h) : -1;
    kx[i] = lmap::to_float(r[1]);
    ky[i] = lmap::to_float(r[2]);
    kur[i] = p->u_right ? p->u_right[i] : -1.0;
  }
  for (int q = 0; q < p->n_local; q++) {
    lmap::Best b;
    int st = RSPL_LMAP_GOOD;
    bool held = false;
    for (int i = 0; i < n1; i++) held |= p->point_id[i] == p->local_ids[q];
    double u = 0, v = 0, xr = 0;
    if (held)
      st = RSPL_LMAP_NOT_SELECTED;
    else
      st = lmap::project(V, p->local_pos + 3 * (size_t)q, u, v, xr);
    if (st == RSPL_LMAP_GOOD) {
      bool any = false;
      const double* d = p->local_desc + (size_t)lmap::kDesc * q;
      for (int i = 0; i < n1; i++) {
        if (key[i] < 0 || !lmap::in_box(kx[i], ky[i], kur[i], p->u_right != nullptr, u, v, xr, V.radius)) continue;
        any = true;
        b.visit(lmap::distance_host(d, p->features + RSPL_FEATURE_ROWS * (size_t)i + 3), key[i], i);
      }
      st = !any ? RSPL_LMAP_NO_CANDIDATE : (b.idx >= 0 && b.good(V) ? RSPL_LMAP_GOOD : RSPL_LMAP_FAILED);
    }
    status[q] = st;
    best_idx[q] = b.idx;
    best[q] = b.best;
    second[q] = b.second;
  }
  return RSPL_OK;
}
