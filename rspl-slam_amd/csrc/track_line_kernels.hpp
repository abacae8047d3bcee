#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "track_kernels.hpp"

namespace rspl {
namespace track {

// The line half of MapBuilder::TrackFrame (src/map_builder.cc:450-455, 490-501) and MapBuilder::AddKeyframe's
// decision (:616-636) behind the tracking chain.  Two kernels, one 1024-thread workgroup per keyframe slot /
// per frame:
//   kf_lines     AssignPointsToLines for a keyframe slot's lines, once per keyframe: the slot's CSR and its
//                keypoint -> lines inverse incidence, kept for every frame tracked against the slot
//   frame_lines  after track_write_kernel: AssignPointsToLines for the frame's lines, MatchLines against the
//                slot from match_kf as the gather kernel left it, the line track id copy, and the keyframe
//                decision on the pose and inlier count track_write_kernel has just written

struct LineParam {  // one frame of the batch, written by the host into host-mapped memory
  const double* lines;  // device [n_lines][4]
  int n_lines;          // 0: no line work for this frame
  int slot;
  int kf_n_lines;       // the slot's line count, 0 when its lines were never set
  int kf_frame_id, frame_id;
  int max_num_match, max_num_passed_frame, pad;
  double kf_R[9], kf_t[3];  // the last keyframe's T_wc: R row-major | t
  double max_angle, max_distance;
};

struct LineOut {  // per-frame result, written into host-mapped memory
  int n_lines, n_matches, n_tracks, overflow;
  int tracked_well, add_keyframe, passed_frames, pad;
  double delta_angle, delta_distance;
};

struct LineArgs {
  int K;          // = Args::K
  int max_lines;  // lines per frame and per keyframe slot, <= 1024
  int cap;        // point-line pairs per frame and per slot
  // keyframe slots [S]
  int* kf_off;         // [S][max_lines + 1] CSR of AssignPointsToLines
  int* kf_idx;         // [S][cap]
  double* kf_dist;     // [S][cap]
  int* kf_kstart;      // [S][K + 1] inverse incidence: keypoint q's lines are kf_kline[kstart[q] .. kstart[q + 1])
  int* kf_kline;       // [S][cap]
  int* kf_status;      // [S] 1: the slot's assignment overflowed cap
  int32_t* kf_ltid;    // [S][max_lines] Frame::GetLineTrackId
  int32_t* kf_lslot;   // [S][max_lines] the map line held, or -1
  // frames [B]
  const LineParam* lparams;  // host-mapped
  int* off;            // [B][max_lines + 1]
  int* idx;            // [B][cap]
  double* dist;        // [B][cap]
  int* kline;          // [B][cap] the frame's inverse incidence (its starts live in LDS)
  int* M;              // [B][max_lines * max_lines] shared-match counts
  int32_t* line_match; // [B][max_lines] device results, for a device consumer
  int32_t* line_tid;
  int32_t* line_slot;
  // results (host-mapped)
  LineOut* out;
  int32_t* o_line_match;  // [B][max_lines]
  int32_t* o_line_tid;
  int32_t* o_line_slot;
};

hipError_t kf_lines(const LineArgs& g, int slot, const double* d_lines, int n_lines, const double* d_features,
                    const int32_t* d_n0, hipStream_t s);
hipError_t frame_lines(const Args& a, const LineArgs& g, int batch, hipStream_t s);

}  // namespace track
}  // namespace rspl
