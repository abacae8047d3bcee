// Local BA, host-only geometry: the Schur chunk plan of a window, the chunk capacity of a handle, the window
// geometry of an Active (plan_window) and the test hooks that expose them.  No device call.
#include "ba_handle.hpp"

using namespace rspl;

namespace rspl {
namespace ba {
// Schur chunks: ranges of kLmChunk landmarks per pose pair while the chunk waves fit one dispatch round (C3: 45 pairs
// x 16 ranges); with many pose pairs (C5: K = 29, 435 pairs) fewer, wider ranges -- each wave then walks more
// passes, but the chip runs them in one round instead of ~17.
// Wide windows (K > the single-wave solve's, fewer than 8 ranges per pair): a diagonal pose pair walks about
// (K - 1) / (obs - 1) times an off-diagonal pair's edge pairs (C5: ~970 vs ~170 per range) and set the chunk phase
// alone -- its ranges are cut into kDiagSub sub-chunks (the off-diagonal pairs keep theirs).  On the single-wave
// windows the diagonal pairs' ranges stay whole and their chunks are launched first (chunk_at).
ChunkPlan chunk_plan(int nL, int K, size_t chunk_slots) {
  constexpr int kDiagSub = 8;
  const int npairs = K * (K + 1) / 2;
  ChunkPlan p{};
  p.nchk = std::max(1, std::min((nL + kLmChunk - 1) / kLmChunk, kChunkWaves / std::max(npairs, 1)));
  p.lmchunk = std::max(kLmChunk, ((nL + p.nchk - 1) / p.nchk + 63) / 64 * 64);
  p.nchk = std::max((nL + p.lmchunk - 1) / p.lmchunk, 1);
  p.dsub = 1;
  p.lmsub = p.lmchunk;
  if (!wave_path(K) && p.nchk < 8 && (size_t)p.nchk * (npairs + (kDiagSub - 1) * K) <= chunk_slots) {
    p.dsub = kDiagSub;
    p.lmsub = ((p.lmchunk + kDiagSub - 1) / kDiagSub + 63) / 64 * 64;
  }
  return p;
}

// chunks a handle of these capacities holds: ranges of kLmChunk for every pose pair (a window's plan without
// diagonal sub-chunks never has more; the sub-chunks are taken only where they fit)
size_t chunk_slots_for(int max_landmarks, int max_poses) {
  const size_t NL = std::max(max_landmarks, 0), K = std::max(max_poses, 0);
  return K * (K + 1) / 2 * std::max<size_t>((NL + kLmChunk - 1) / kLmChunk, 1);
}

void plan_window(Active& A, int nL, int K, size_t chunk_slots, bool update_geometry) {
  const ChunkPlan cp = chunk_plan(nL, K, chunk_slots);
  A.nchk = cp.nchk;
  A.lmchunk = cp.lmchunk;
  A.dsub = cp.dsub;
  A.lmsub = cp.lmsub;
  A.K = K;
  A.npairs = K * (K + 1) / 2;
  A.nL = nL;
  if (update_geometry) set_update_geometry(A);
}
}  // namespace ba
}  // namespace rspl

namespace {
// the hooks' window: its sizes checked, planned in a handle of the given capacities
int debug_window(int n_landmarks, int n_poses, int max_landmarks, int max_poses, bool update_geometry, ba::Active& A,
                 size_t& slots) {
  RSPL_CHECK_ARG(n_landmarks >= 0 && n_poses >= 0 && max_landmarks >= n_landmarks && max_poses >= n_poses,
                 "rspl_ba_debug_chunk_plan: bad sizes");
  slots = ba::chunk_slots_for(max_landmarks, max_poses);
  ba::plan_window(A, n_landmarks, n_poses, slots, update_geometry);
  return RSPL_OK;
}
}  // namespace

extern "C" int rspl_ba_debug_chunk_plan(int n_landmarks, int n_poses, int max_landmarks, int max_poses,
                                        rspl_ba_chunk_plan* out) {
  RSPL_CHECK_ARG(out, "rspl_ba_debug_chunk_plan: NULL argument");
  ba::Active A{};
  size_t slots = 0;
  if (const int rc = debug_window(n_landmarks, n_poses, max_landmarks, max_poses, true, A, slots)) return rc;
  *out = rspl_ba_chunk_plan{A.nchk, A.lmchunk, A.dsub, A.lmsub, ba::chunk_count(A), ba::chunk_grid(A), A.ue_bpr,
                            (int64_t)slots};
  return RSPL_OK;
}

extern "C" int rspl_ba_debug_chunk_geometry(int n_landmarks, int n_poses, int max_landmarks, int max_poses,
                                            int32_t* chunks, int32_t* order) {
  RSPL_CHECK_ARG(chunks && order, "rspl_ba_debug_chunk_geometry: NULL argument");
  ba::Active A{};
  size_t slots = 0;
  if (const int rc = debug_window(n_landmarks, n_poses, max_landmarks, max_poses, false, A, slots)) return rc;
  const int nc = ba::chunk_count(A), grid = ba::chunk_grid(A);
  for (int c = 0; c < nc; c++) {  // the geometry the pair lists are built from (pair_scan)
    const ba::ChunkGeo q = ba::chunk_geo(A, c);
    const int32_t row[6] = {q.pr, q.g0, q.g1, q.c0, q.c1, q.gend};
    std::copy(row, row + 6, chunks + 6 * c);
  }
  for (int vb = 0; vb < grid; vb++) {  // the launch order (pair_chunk); the chunk's own geometry must agree
    int c = -1;
    ba::ChunkGeo q;
    order[vb] = -1;
    if (!ba::chunk_at(A, vb, c, q)) continue;
    const ba::ChunkGeo r = ba::chunk_geo(A, c);
    const bool same = q.pr == r.pr && q.lb == r.lb && q.g0 == r.g0 && q.g1 == r.g1 && q.gend == r.gend &&
                      q.c0 == r.c0 && q.c1 == r.c1;
    order[vb] = same ? c : -2;
  }
  return RSPL_OK;
}
