// Host staging of one LocalmapOptimization call (rspl_ba_local): the caller's edge arrays (the
// reference's per-type constraint vectors, g2o_optimization.cc:81-167) validated, counted per landmark
// and placed in landmark-CSR order -- point landmarks first, each landmark's edges contiguous, input
// order within a landmark (the order every per-landmark reduction of the kernels follows).  Large
// unsharded calls run on a few persistent host workers (HostPool); the result is identical to the
// serial passes (rspl_ba_debug_stage: tests/test_ba_stage.py).
#pragma once

#include <memory>
#include <vector>

#include "ba_kernels.hpp"
#include "common.hpp"
#include "host_pool.hpp"

namespace rspl {
namespace ba {

struct Stager {
  // pass 1: validate the edges, count the local edges per landmark, mark the poses with edges.
  // sharded: keep the edges of landmarks g % nranks == rank.  par_edges: stage on the workers from
  // this many edges (unsharded only; <= 0: never).  Sets E (local edges), Ep (local point edges) and
  // pose_has_edge; RSPL_E_ARG (message set) on invalid input.
  int count(const rspl_ba_problem* pr, bool sharded, int rank, int nranks, int par_edges);
  // pass 2: lm_off [nL + 1] and, per CSR position k < E, the edge's type, pose, landmark, camera,
  // caller id (gmap), reduced pose (pidx of its pose) and observation (points: 4 doubles each from
  // eobs; lines: 8 doubles each from eobs + 4 Ep); ginv (or null): the CSR position of every caller id
  struct Out {
    int* lm_off;
    int8_t* etype;
    int* epose;
    int* elm;
    int* ecam;
    int* gmap;
    int* lpose;
    double* eobs;
    const int* pidx;
    int* ginv = nullptr;
  };
  void place(const rspl_ba_problem* pr, const Out& o);
  // after count(): the reduced numbering of the poses -- pidx[p] (pidx may be null) = the pose's index among the
  // optimised ones (it has a local edge and is not fixed), else -1; returns their number K
  int number_poses(const rspl_ba_problem* pr, int* pidx) const {
    int K = 0;
    for (int p = 0; p < pr->n_poses; p++) {
      const int k = (pose_has_edge[p] && !pr->pose_fixed[p]) ? K++ : -1;
      if (pidx) pidx[p] = k;
    }
    return K;
  }

  int E = 0, Ep = 0;
  std::vector<uint8_t> pose_has_edge;  // [np]

 private:
  bool sh_ = false, par_ = false;
  int rank_ = 0, nranks_ = 1, NP_ = 1;
  std::vector<int> lm_cnt_;                  // serial: per-landmark counts (shifted by one), then cursors
  std::unique_ptr<HostPool> pool_;
  std::vector<std::vector<int2>> bkt_;       // parallel: [part][landmark range] {caller edge id, landmark}
  std::vector<std::vector<int>> pcnt_;       // parallel: [range] per-landmark counts, then CSR cursors
  std::vector<std::vector<uint8_t>> ppact_;  // parallel: [part] poses with edges
  std::vector<int> pcut_, gcut_, rstart_;    // part p: caller edges [pcut[p], pcut[p+1]); range q:
                                             //   landmarks [gcut[q], gcut[q+1]), CSR [rstart[q], rstart[q+1])
};

// Segment offsets of the Schur chunks' edge-pair lists, counted on the host from the staged CSR: chunk c of
// pose pair (a <= b) and a landmark range owns sum over its active landmarks of cnt_g[a] * cnt_g[b] pairs
// (cnt_g[p]: the landmark's edges on reduced pose p; -1 entries of lm_pose are on no reduced pose), exactly what
// pair_scan counts on the device.  G: nchk / lmchunk / dsub / lmsub / K / npairs / nL set (chunk_geo's fields).
// pp_off [chunk_count(G) + 1]: the exclusive scan; returns the total.
size_t pair_offsets(const Active& G, const int* lm_off, const int* lm_pose, const uint8_t* lm_act, int* pp_off);

// Line workgroups (Active::ltab) of the line landmarks [nq, nL) of the staged CSR: consecutive line landmarks
// packed whole into <= kLineBlk edges (and <= kLineBlk landmarks), so a workgroup sums their blocks itself; a
// landmark with more edges gets workgroups of its own, flagged split (1 << 8: per-edge records + last-edge
// ticket).  Entry {first CSR position, edges | split << 8, first landmark, end landmark}; returns their number.
int pack_line_blocks(const int* lm_off, int nq, int nL, int4* ltab);
// entries ltab must hold for nl line landmarks with line_edges edges: at most one per line landmark plus one per
// kLineBlk line edges (a landmark with more edges is split)
inline size_t line_blocks_bound(size_t nl, size_t line_edges) { return nl + line_edges / kLineBlk + 2; }

}  // namespace ba
}  // namespace rspl
