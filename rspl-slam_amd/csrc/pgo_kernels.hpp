// Device side of the pose-graph optimiser: what pgo.cpp hands to pgo_kernels.hip.
#pragma once
#include "common.hpp"
#include "pgo_solve.hpp"

namespace rspl {
namespace pgo {

// what the host reads after one synchronisation (host-mapped)
struct Scalars {
  double cost;      // sum of the edges' costs, fixed tree
  double pred;      // delta^T (lambda delta + b)
  double max_step;  // max |delta|
  double max_diag;  // max diag H
  int32_t bad_pivot, pad;
};

struct DArgs {
  int n_poses, n_edges, n_free, nt;  // nt: tiles per side
  // poses: current and trial (pgo.cpp swaps them after an accepted step)
  double *q, *p, *tq, *tp;
  const int32_t* pose_free;  // [n_poses] free index or -1
  const int32_t *edge_i, *edge_j;
  const double *edge_q, *edge_p, *edge_w;
  // per edge: Hii | Hij | Hjj (108), gi | gj (12), cost, residual (6)
  double *eblk, *eg, *ecost, *eres;
  // the filled tiles in column-major tile order, kTileElems each, and the vectors of nt * kTile entries
  double *tiles, *b, *hdiag, *y, *delta;
  // the plan's tables (pgo.cpp: struct Plan)
  const int32_t *tile_row, *tile_col;  // [n_filled]
  const int32_t* tile_map;             // [nt][nt], -1 where nothing is stored
  const int32_t *tile_blk_off, *blk_pos, *blk_off, *blk_contrib;
  const int32_t *pose_off, *pose_contrib;
  const int32_t *col_diag, *col_off, *col_tile, *col_row;
  int32_t* flag;  // a non-positive pivot in this trial: every later kernel of the trial returns at once
  Scalars* out;
};

hipError_t launch_linearise(const DArgs& a, hipStream_t s);                                // edges, gradient, reduce
hipError_t launch_assemble(const DArgs& a, int n_filled, double lambda, hipStream_t s);    // tiles of H + lambda I
hipError_t launch_factor(const DArgs& a, const int32_t* host_col_off, hipStream_t s);      // three kernels per column
hipError_t launch_substitute(const DArgs& a, hipStream_t s);                               // delta
hipError_t launch_trial(const DArgs& a, double lambda, hipStream_t s);                     // trial poses, cost, reduce

}  // namespace pgo
}  // namespace rspl
