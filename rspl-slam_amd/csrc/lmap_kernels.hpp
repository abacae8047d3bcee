#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lmap_match.hpp"

namespace rspl {
namespace lmap {

struct Param {  // one frame of the batch, written by the host into host-mapped memory
  const double* feat;     // [cap][259]
  const int32_t* n1;
  const double* u_right;  // or null: no dxr term
  const int32_t* pid;     // [n1] the map point the keypoint holds, or -1
  const double* pxyz;     // [n1][3]
  const uint8_t* pgood;   // [n1] or null: every held point is Good
  double* kf_points;      // the tracker slot the merge fills, or null (search only)
  uint8_t* kf_state;
  int32_t* kf_tid;
  View V;
};

struct Out {  // per-frame counts, written into host-mapped memory
  int n1, n_selected, n_projected, n_cand, n_good, pad[3];
};

struct Args {
  const Param* host_params;  // host-mapped, read by the prep kernel only
  Param* params;             // its device copy, read by the search and merge kernels
  int K, L;                  // per-frame capacity of the per-keypoint / per-local-point arrays
  // bank and local map
  const double* bank;        // [max_bank_points][256], rows 16-byte aligned
  const int32_t* local_row;  // [L] bank row of local point p
  const int32_t* local_id;   // [L]
  const double* local_pos;   // [L][3]
  // the frame's keypoints as the search reads them (prep kernel)
  double* kx;                // [B][K] float-rounded x
  double* ky;
  double* kur;               // [B][K] u_right (-1 without the array)
  int32_t* kkey;             // [B][K] grid cell key, -1: not a candidate (holds a point, or past n1)
  int32_t* n1c;              // [B] clamped keypoint count
  // per local point (search kernel)
  int32_t* status;           // [B][L]
  int32_t* best_idx;
  double* best;
  double* second;
  // the merge kernel's lists before they are copied out
  int32_t* good_kp;          // [B][L]
  int32_t* good_point;
  int32_t* assoc;            // [B][K]
  // identity indices of the chained tracking step (merge kernel)
  int32_t* idx0;             // [B][K]
  int32_t* idx1;
  // results (host-mapped)
  Out* out;
  int32_t* o_good_kp;        // [B][L]
  int32_t* o_good_point;
  int32_t* o_assoc;          // [B][K]
};

// rows 3..258 of record pairs[2k + 1] of feat -> bank row pairs[2k]; pairs: host-mapped
hipError_t store(double* bank, const double* feat, const int32_t* pairs, int n, hipStream_t s);
// prep | search | merge for `batch` frames against the first n_local points of the local map
hipError_t search(const Args& a, int batch, int n_local, hipStream_t s);

}  // namespace lmap
}  // namespace rspl
