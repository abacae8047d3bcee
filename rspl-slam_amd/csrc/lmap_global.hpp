// Global descriptor search of the local table (relocalisation): what lmap_global.hip and the
// host (lmap_reloc.cpp: rspl_lmap_global_*, rspl_lmap_debug_global_host) share.
//
//   D[i][p] = 2 (1 - q_i . d_p)           keypoint i of the frame against local point p (its bank row)
//   per keypoint  best / arg / second     lmap::Best's rule with a constant key over p ascending: a tie keeps the
//                                         lowest p, second is the second smallest value, 4.0 where nothing is below
//   per point     kbest                   the lowest i that attains min_i D[i][p]
//   pass          best < max_distance and best < max_ratio * second
//   match         pass and (mutual == 0 or kbest[arg] == i)
//
// Both folds are order-free -- (distance, index) is compared lexicographically and the second best of a union is
// min(max(b1, b2), s1, s2) -- so the device's tiles, partials and merge give the decisions of the ascending walk.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "lmap_match.hpp"

namespace rspl {
namespace lmap {

constexpr int kGQTile = 64;    // keypoints per workgroup (4 waves x 16 rows)
constexpr int kGGroup = 64;    // bank rows per accumulator pass (4 column tiles of 16 per wave)
constexpr int kGSlab = 64;     // descriptor entries staged per LDS slab
constexpr int kGMaxGroups = 8; // accumulator passes per workgroup at most
constexpr int kGTargetBlocks = 2048;

// chunk_rows: bank rows per workgroup = kGGroup * m, m the smallest power of two (at most kGMaxGroups) that brings
// the grid of a full table down to kGTargetBlocks workgroups: small tables keep every CU busy, a full bank keeps
// the per-keypoint partials few
inline void global_plan(int max_keypoints, int max_local_points, int* chunk_rows, int* qtile_rows, int* k_slab) {
  const long long nq = (max_keypoints + kGQTile - 1) / kGQTile;
  const long long ng = (max_local_points + kGGroup - 1) / kGGroup;
  int m = 1;
  while (m < kGMaxGroups && (ng + m - 1) / m * nq > kGTargetBlocks) m *= 2;
  if (chunk_rows) *chunk_rows = kGGroup * m;
  if (qtile_rows) *qtile_rows = kGQTile;
  if (k_slab) *k_slab = kGSlab;
}

struct GBest {  // per keypoint: idx INT_MAX = none (best 4.0)
  double best = 4.0, second = 4.0;
  int idx = INT_MAX;
  RSPL_LMAP_HD void visit(double d, int i) {  // a candidate not below 4.0 (or NaN) is no candidate, as in Best
    if (!(d < 4.0)) return;
    if (d < best || (d == best && i < idx)) {
      second = best;
      best = d;
      idx = i;
    } else if (d < second) {
      second = d;
    }
  }
  RSPL_LMAP_HD void merge(double b, double s, int i) {
    const double hi = b < best ? best : b;  // max(b1, b2)
    const double lo = s < second ? s : second;
    if (b < best || (b == best && i < idx)) {
      best = b;
      idx = i;
    }
    second = hi < lo ? hi : lo;
  }
};

struct GMin {  // per local point: idx INT_MAX = none
  double v = INFINITY;
  int idx = INT_MAX;
  RSPL_LMAP_HD void visit(double d, int i) {
    if (d < v || (d == v && i < idx)) {
      v = d;
      idx = i;
    }
  }
};

RSPL_LMAP_HD bool global_pass(double best, double second, double max_distance, double max_ratio) {
#pragma clang fp contract(off)
  return best < max_distance && best < max_ratio * second;
}

struct GParam {  // one frame of a global enqueue, written by the host into host-mapped memory
  const double* feat;  // [cap][259]
  const int32_t* n1;
};

struct GOut {  // per-frame counts, host-mapped
  int n1, n_local, n_pass, n_matched;
};

struct GArgs {
  const GParam* host_params;  // host-mapped, read by the pack kernel only
  GParam* params;             // its device copy
  int K, L;                   // the handle's capacities (strides of the host-mapped results)
  int Kpad, Lpad;             // K rounded up to the query tile, L to the chunk
  int chunk_rows, max_chunks, n_qtiles;
  double max_distance, max_ratio;
  int mutual;
  const double* bank;
  const int32_t* local_row;
  const int32_t* local_id;
  const double* local_pos;
  double* qpack;              // [B][Kpad][256] the frame's descriptors, dense, zero rows past n1
  int32_t* n1c;               // [B]
  // partials: per keypoint and chunk, per local point and query tile
  double* pk_best;            // [B][max_chunks][Kpad]
  double* pk_second;
  int32_t* pk_arg;
  double* pp_min;             // [B][n_qtiles][Lpad]
  int32_t* pp_arg;
  // merged, device side
  int32_t* arg;               // [B][K]
  double* best;
  double* second;
  int32_t* match;
  int32_t* kbest;             // [B][L]
  int32_t* m_kp;              // [B][K] the compacted matches
  // results (host-mapped)
  GOut* out;
  int32_t* o_arg;             // [B][K]
  double* o_best;
  double* o_second;
  int32_t* o_match;
  int32_t* o_kbest;           // [B][L]
  int32_t* o_m_kp;            // [B][K]
  int32_t* o_m_local;
  int32_t* o_m_id;
  double* o_m_pos;            // [B][K][3]
  double* o_m_xy;             // [B][K][2]
};

// pack | search | fold | merge for `batch` frames against the first n_local points of the local table
hipError_t global_search(const GArgs& a, int batch, int n_local, hipStream_t s);

}  // namespace lmap
}  // namespace rspl
