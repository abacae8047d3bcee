#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rspl {
namespace kf {

struct Param {  // one frame of the batch, written by the host into host-mapped memory
  const double* feat_l;       // [cap][259] left records (x, y = rows 1, 2)
  const double* feat_r;
  const int32_t* n_l;
  const int32_t* n_r;
  const int32_t* idx0;        // left -> right
  const int32_t* idx1;        // right -> left
  // the frame's host arrays in the handle's pinned staging (device addresses); each may be null
  const int32_t* track_id;    // null: all -1
  const int32_t* point_slot;  // null: all -1
  const double* points;       // [n][3] of the held points
  const uint8_t* state;       // RSPL_TRACK_* of the held points
  // the tracker's keyframe table (all three or none)
  double* tbl_points;
  uint8_t* tbl_state;
  int32_t* tbl_tid;
  double cam[5];              // fx fy cx cy bf
  double win[3];              // min_x_diff max_x_diff max_y_diff
  double Twc[12];             // R row-major | t
  int next_track_id, init;
  int n_host;                 // entries of the four staged host arrays
  int tbl_cap;                // entries the table arrays hold: keypoints past it are not written
};

struct Out {  // per-frame counts, host-mapped
  int n_keypoints, n_matches, n_stereo_matches, n_new_ids, n_new_points, n_new_good, next_track_id, pad;
};

struct Args {
  const Param* params;  // host-mapped
  int K;                // per-frame capacity of every per-keypoint array
  // results (host-mapped), [B][K] each
  Out* out;
  double* u_right;
  double* depth;
  int32_t* track_id;
  uint8_t* new_point;   // 0 none, 1 Good, 2 UnTriangulated
  double* new_position; // [B][K][3]
};

struct TriArgs {  // everything host-mapped
  const double* Twc;        // [np][16]
  const int32_t* offsets;   // [n + 1]
  const int32_t* obs_pose;
  const double* obs_xy;
  double cam[4];            // fx fy cx cy
  int n;
  double* position;         // [n][3]
  uint8_t* status;          // [n] kTri*
};

hipError_t stereo(const Args& a, int batch, hipStream_t s);
hipError_t triangulate(const TriArgs& a, hipStream_t s);

}  // namespace kf
}  // namespace rspl
