#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "frame_kernels.hpp"
#include "pnp_kernels.hpp"

namespace rspl {
namespace track {

constexpr int kDrawCap = 2048;  // raw RNG draws the gather kernel can index (its LDS run-length table)

struct Param {  // one frame of the batch, written by the host into host-mapped memory
  const double* feat;      // [cap][259]
  const int32_t* n1;
  const int32_t* idx0;
  const int32_t* idx1;
  const double* u_right;   // or null
  const double* kf_points; // the slot's table
  const uint8_t* kf_state;
  const int32_t* kf_tid;
  int n0, min_match, iters, pad;
  double cam[5];           // fx fy cx cy bf
  double thr2, confidence; // PnP
  double delta[2], th[2];  // FrameOptimization
  double last[12];         // last T_wc: R row-major | t
};

struct Out {  // per-frame result, written into host-mapped memory
  double q[4];  // T_wc (x y z w)
  double p[3];
  double chi2[4];
  int iters[4];
  int pose_set, n_inliers, n_pnp, pnp_used;
  int n1, n_matches, n_kept, n_mono, n_stereo, rounds;
};

struct Seed {  // the seed kernel's record (debug read-back)
  double q[4];  // T_wc (x y z w)
  double p[3];
  int pnp_used, pad;
};

struct Args {
  const Param* host_params;  // host-mapped, read once by the gather kernel
  Param* params;             // its device copy, read by the later kernels
  int K;                     // per-frame capacity of every per-keypoint / per-slot array
  const uint32_t* draws;     // [n_draws] raw multiply-with-carry draws
  int n_draws;
  // gather outputs
  pnp::Desc* pnp_desc;
  double* pts;               // [B][K][3]
  double* kps;               // [B][K][2]
  int32_t* subsets;          // [B][kMaxIters][5]
  frame::Desc* frame_desc;
  frame::Edge* edges;        // [B][K]
  uint8_t* inl_in;           // [B][K]
  int32_t* corr_kp;          // [B][K] correspondence slot -> keypoint
  int32_t* edge_kp;          // [B][K] edge slot -> keypoint
  int32_t* kp_edge;          // [B][K] keypoint -> edge slot, -1: none
  int32_t* match_kf;         // [B][K]
  int32_t* inl_tid;          // [B][K] TrackFrame's `inliers`
  int32_t* counts;           // [B][4] n1, matches, mono, stereo
  // solver outputs
  const pnp::Out* pnp_out;
  const frame::Out* frame_out;
  const uint8_t* edge_inl;   // [B][K] FrameOptimization's inl_out
  Seed* seed;
  // results (host-mapped)
  Out* out;
  int32_t* o_match_kf;
  int32_t* o_track_id;
  uint8_t* o_kept;
};

hipError_t gather(const Args& a, int batch, hipStream_t s);
hipError_t seed(const Args& a, int batch, hipStream_t s);
hipError_t write_back(const Args& a, int batch, hipStream_t s);

}  // namespace track
}  // namespace rspl
