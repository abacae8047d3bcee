// The global descriptor search of the local table (relocalisation): C ABI rspl_lmap_global_* over
// lmap_global.hip, on the handle of lmap.cpp.  The reference has no such stage; rspl_lmap_debug_global_host is the
// contract (lmap_global.hpp) on host arrays, with the distances of lmap_match.hpp's fixed summation order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "lmap_handle.hpp"

using namespace rspl;

namespace {

// the global search's device and host-mapped arrays, once
int global_setup(rspl_lmap* h) {
  if (h->g_ready) return RSPL_OK;
  const size_t B = h->cfg.max_batch, K = h->cfg.max_keypoints, L = h->cfg.max_local_points;
  lmap::GArgs& g = h->g;
  int qtile = 0, slab = 0;
  lmap::global_plan((int)K, (int)L, &g.chunk_rows, &qtile, &slab);
  g.K = (int)K;
  g.L = (int)L;
  g.n_qtiles = (int)((K + qtile - 1) / qtile);
  g.Kpad = g.n_qtiles * qtile;
  g.max_chunks = (int)((L + g.chunk_rows - 1) / g.chunk_rows);
  g.Lpad = g.max_chunks * g.chunk_rows;
  const size_t KP = g.Kpad, LP = g.Lpad, NC = g.max_chunks, NQ = g.n_qtiles;
  auto carve = [&](auto& A, auto& P) {
    h->g_params = P.template take<lmap::GParam>(B, &g.host_params);
    h->g_out = P.template take<lmap::GOut>(B, &g.out);
    h->go_arg = P.template take<int32_t>(B * K, &g.o_arg);
    h->go_best = P.template take<double>(B * K, &g.o_best);
    h->go_second = P.template take<double>(B * K, &g.o_second);
    h->go_match = P.template take<int32_t>(B * K, &g.o_match);
    h->go_kbest = P.template take<int32_t>(B * L, &g.o_kbest);
    h->go_m_kp = P.template take<int32_t>(B * K, &g.o_m_kp);
    h->go_m_local = P.template take<int32_t>(B * K, &g.o_m_local);
    h->go_m_id = P.template take<int32_t>(B * K, &g.o_m_id);
    h->go_m_pos = P.template take<double>(3 * B * K, &g.o_m_pos);
    h->go_m_xy = P.template take<double>(2 * B * K, &g.o_m_xy);
    g.params = A.template take<lmap::GParam>(B);
    g.qpack = A.template take<double>(B * KP * lmap::kDesc);
    g.n1c = A.template take<int32_t>(B);
    g.pk_best = A.template take<double>(B * NC * KP);
    g.pk_second = A.template take<double>(B * NC * KP);
    g.pk_arg = A.template take<int32_t>(B * NC * KP);
    g.pp_min = A.template take<double>(B * NQ * LP);
    g.pp_arg = A.template take<int32_t>(B * NQ * LP);
    g.arg = A.template take<int32_t>(B * K);
    g.best = A.template take<double>(B * K);
    g.second = A.template take<double>(B * K);
    g.match = A.template take<int32_t>(B * K);
    g.kbest = A.template take<int32_t>(B * L);
    g.m_kp = A.template take<int32_t>(B * K);
  };
  Sizer sz, psz;
  carve(sz, psz);
  RSPL_HIP(hipSetDevice(h->cfg.device));
  int rc = h->g_arena.reserve(sz.used + 256);
  if (!rc) rc = h->g_pinned.reserve(psz.used + 256);
  if (rc) {
    h->g_arena.release();
    h->g_pinned.release();
    return rc;
  }
  carve(h->g_arena, h->g_pinned);
  g.bank = h->bank;
  g.local_row = h->d_local_row;
  g.local_id = h->d_local_id;
  g.local_pos = h->d_local_pos;
  h->g_ready = true;
  return RSPL_OK;
}

// one keypoint set against one table on host arrays: the ascending walk of the contract (lmap_global.hpp)
void global_host(int n1, const double* feat, int nl, const int32_t* ids, const double* pos, const double* desc,
                 const rspl_lmap_global_params& gp, rspl_lmap_global_result* r) {
  std::vector<lmap::GBest> kb(n1);
  std::vector<lmap::GMin> pm(nl);
  for (int i = 0; i < n1; i++) {
    const double* q = feat + RSPL_FEATURE_ROWS * (size_t)i + 3;
    for (int p = 0; p < nl; p++) {
      const double d = lmap::distance_host(q, desc + (size_t)lmap::kDesc * p);
      kb[i].visit(d, p);
      pm[p].visit(d, i);
    }
  }
  int n_pass = 0, n_matched = 0;
  for (int i = 0; i < n1; i++) {
    const int ar = kb[i].idx == INT_MAX ? -1 : kb[i].idx;
    const bool pass = ar >= 0 && lmap::global_pass(kb[i].best, kb[i].second, gp.max_distance, gp.max_ratio);
    const int mt = pass && (!gp.mutual || pm[ar].idx == i) ? ar : -1;
    n_pass += pass;
    if (r->arg) r->arg[i] = ar;
    if (r->best) r->best[i] = kb[i].best;
    if (r->second) r->second[i] = kb[i].second;
    if (r->match) r->match[i] = mt;
    if (mt < 0) continue;
    const size_t j = n_matched++;
    if (r->match_kp) r->match_kp[j] = i;
    if (r->match_local) r->match_local[j] = mt;
    if (r->match_id) r->match_id[j] = ids[mt];
    if (r->match_pos) memcpy(r->match_pos + 3 * j, pos + 3 * (size_t)mt, sizeof(double) * 3);
    if (r->match_xy) memcpy(r->match_xy + 2 * j, feat + RSPL_FEATURE_ROWS * (size_t)i + 1, sizeof(double) * 2);
  }
  if (r->kbest)
    for (int p = 0; p < nl; p++) r->kbest[p] = pm[p].idx == INT_MAX ? -1 : pm[p].idx;
  r->n_keypoints = n1;
  r->n_local = nl;
  r->n_pass = n_pass;
  r->n_matched = n_matched;
}

bool good_global_params(const rspl_lmap_global_params* p) {
  return p && std::isfinite(p->max_distance) && std::isfinite(p->max_ratio);
}

}  // namespace

// ---- the global search (relocalisation) ----------------------------------------------------------------------
extern "C" int rspl_lmap_global_enqueue(rspl_lmap* h, int batch, const rspl_lmap_frame* frames,
                                        const rspl_lmap_global_params* params, void* stream) {
  RSPL_CHECK_ARG(h && (batch == 0 || frames), "rspl_lmap_global_enqueue: NULL argument");
  RSPL_CHECK_ARG(!h->host_only, "rspl_lmap_global_enqueue: a host-only handle (device < 0) has no device side");
  RSPL_CHECK_ARG(good_global_params(params), "rspl_lmap_global_enqueue: bad parameters");
  RSPL_CHECK_ARG(batch >= 0 && batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
  RSPL_CHECK_ARG(!h->pending, "rspl_lmap_global_enqueue: the previous enqueue has not been fetched");
  for (int b = 0; b < batch; b++)
    RSPL_CHECK_ARG(frames[b].d_features && frames[b].d_n1, "frame %d: NULL device pointer", b);
  h->g_batch = batch;
  if (batch == 0) return RSPL_OK;
  const int rc = global_setup(h);
  if (rc) return rc;
  for (int b = 0; b < batch; b++) {
    h->g_params[b].feat = frames[b].d_features;
    h->g_params[b].n1 = frames[b].d_n1;
  }
  h->g.max_distance = params->max_distance;
  h->g.max_ratio = params->max_ratio;
  h->g.mutual = params->mutual != 0;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  RSPL_HIP(lmap::wait_uploads(h, st));
  RSPL_HIP(lmap::global_search(h->g, batch, h->n_local, st));
  RSPL_HIP(hipEventRecord(h->done, st));
  h->pending = true;
  h->pending_global = true;
  return RSPL_OK;
}

extern "C" int rspl_lmap_global_fetch(rspl_lmap* h, rspl_lmap_global_result* res) {
  RSPL_CHECK_ARG(h && (res || h->g_batch == 0), "rspl_lmap_global_fetch: NULL argument");
  RSPL_CHECK_ARG(!(h->pending && !h->pending_global), "rspl_lmap_global_fetch: the enqueue in flight is not a global one");
  if (h->pending) {
    RSPL_HIP(hipEventSynchronize(h->done));
    h->pending = false;
    h->pending_global = false;
  }
  const size_t K = h->cfg.max_keypoints, L = h->cfg.max_local_points;
  for (int b = 0; b < h->g_batch; b++) {
    const lmap::GOut& o = h->g_out[b];
    rspl_lmap_global_result& r = res[b];
    r.n_keypoints = o.n1;
    r.n_local = o.n_local;
    r.n_pass = o.n_pass;
    r.n_matched = o.n_matched;
    const size_t n1 = (size_t)std::min<int>(std::max(o.n1, 0), (int)K);
    const size_t nl = (size_t)std::min<int>(std::max(o.n_local, 0), (int)L);
    const size_t nm = (size_t)std::min<int>(std::max(o.n_matched, 0), (int)n1);
    if (r.arg) memcpy(r.arg, h->go_arg + K * b, sizeof(int32_t) * n1);
    if (r.best) memcpy(r.best, h->go_best + K * b, sizeof(double) * n1);
    if (r.second) memcpy(r.second, h->go_second + K * b, sizeof(double) * n1);
    if (r.match) memcpy(r.match, h->go_match + K * b, sizeof(int32_t) * n1);
    if (r.kbest) memcpy(r.kbest, h->go_kbest + L * b, sizeof(int32_t) * nl);
    if (r.match_kp) memcpy(r.match_kp, h->go_m_kp + K * b, sizeof(int32_t) * nm);
    if (r.match_local) memcpy(r.match_local, h->go_m_local + K * b, sizeof(int32_t) * nm);
    if (r.match_id) memcpy(r.match_id, h->go_m_id + K * b, sizeof(int32_t) * nm);
    if (r.match_pos) memcpy(r.match_pos, h->go_m_pos + 3 * K * b, sizeof(double) * 3 * nm);
    if (r.match_xy) memcpy(r.match_xy, h->go_m_xy + 2 * K * b, sizeof(double) * 2 * nm);
  }
  return RSPL_OK;
}

extern "C" int rspl_lmap_debug_global_host(const rspl_lmap_global_host_problem* p, const rspl_lmap_global_params* params,
                                           rspl_lmap_global_result* result) {
  RSPL_CHECK_ARG(p && result, "rspl_lmap_debug_global_host: NULL argument");
  RSPL_CHECK_ARG(good_global_params(params), "rspl_lmap_debug_global_host: bad parameters");
  RSPL_CHECK_ARG(p->n_keypoints >= 0 && p->n_local >= 0, "rspl_lmap_debug_global_host: bad sizes");
  RSPL_CHECK_ARG((p->n_keypoints == 0 || p->features) && (p->n_local == 0 || (p->local_ids && p->local_pos && p->local_desc)),
                 "rspl_lmap_debug_global_host: NULL array");
  global_host(p->n_keypoints, p->features, p->n_local, p->local_ids, p->local_pos, p->local_desc, *params, result);
  return RSPL_OK;
}

extern "C" int rspl_lmap_debug_global_plan(int max_keypoints, int max_local_points, int* chunk_rows, int* qtile_rows,
                                           int* k_slab) {
  RSPL_CHECK_ARG(max_keypoints > 0 && max_local_points > 0, "rspl_lmap_debug_global_plan: capacities %d, %d",
                 max_keypoints, max_local_points);
  lmap::global_plan(max_keypoints, max_local_points, chunk_rows, qtile_rows, k_slab);
  return RSPL_OK;
}
