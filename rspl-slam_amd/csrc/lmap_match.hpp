// Map::SearchByProjection's per-point arithmetic (src/map.cc:952-1005, Camera::StereoProject include/camera.h:59-70,
// Frame::FindGrid / FindNeighborKeypoints src/frame.cc:70-78, :324-349, DescriptorDistance src/utils.cc:14-16) as
// ONE source compiled for the host and for the device: lmap_search_kernel runs it one wave per local map point,
// rspl_lmap_debug_search_host and the CPU tests run the host instantiation.
//
//   project      pc = Rwc^T (pw - twc), z <= 0 is behind; u = x z_inv fx + cx, v = y z_inv fy + cy,
//                xr = u - bf z_inv; strictly inside (0, W) x (0, H)
//   in_box       |kx - u| < r, |ky - v| < r with the keypoint rounded to float (cv::KeyPoint::pt), and
//                |u_right - xr| < r when xr > 0 and the frame has a u_right array
//   cell_key     the 64 x 48 grid cell the keypoint was binned into (round half away from zero of the unrounded
//                coordinate, clamped), as gx * 48 + gy: the grid walk visits cells in ascending key and the
//                keypoints of a cell in ascending index, which decides an exact tie in the distance
//   partial4     a lane's share of the descriptor dot product: entries 4l..4l+3, ((a0 b0 + a1 b1) + a2 b2) + a3 b3
//   Best         best / second-best bookkeeping in index order: argmin over (dist, key, idx); `second` is the
//                second smallest value (4.0 where nothing is below it), which is what the reference's visiting
//                order leaves whatever that order is
//
// The 64 partials are summed by the xor butterfly 32, 16, 8, 4, 2, 1 (wave::xsum64 on the device, xsum64_host here:
// step o adds partial l ^ o to partial l, so after the last step every slot holds the same bits).  Contraction is
// off on both sides, so the bits do not depend on what the optimiser fuses.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/rspl.h"

namespace rspl {
namespace lmap {

constexpr int kGridCols = 64, kGridRows = 48;  // FRAME_GRID_COLS / FRAME_GRID_ROWS
constexpr int kDesc = 256;
constexpr int kMaxKeypoints = 8192;  // the merge kernel's per-keypoint claims live in LDS: 32 KB

#define RSPL_LMAP_HD __host__ __device__ __forceinline__

struct View {  // what one frame's search needs besides the keypoints
  double R[9], t[3];  // T_wc: rotation row-major | translation
  double fx, fy, cx, cy, bf;
  double W, H;
  double inv_w, inv_h;  // _grid_width_inv / _grid_height_inv
  double radius, max_distance, max_ratio;
};

inline void make_view(const double* Twc, double fx, double fy, double cx, double cy, double bf, int width, int height,
                      double radius, double max_distance, double max_ratio, View& V) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) V.R[3 * r + c] = Twc[4 * r + c];
    V.t[r] = Twc[4 * r + 3];
  }
  V.fx = fx; V.fy = fy; V.cx = cx; V.cy = cy; V.bf = bf;
  V.W = (double)width;
  V.H = (double)height;
  V.inv_w = (double)kGridCols / (double)width;
  V.inv_h = (double)kGridRows / (double)height;
  V.radius = radius; V.max_distance = max_distance; V.max_ratio = max_ratio;
}

// RSPL_LMAP_GOOD: projected (u, v, xr set); RSPL_LMAP_BEHIND / RSPL_LMAP_OFF_IMAGE otherwise
RSPL_LMAP_HD int project(const View& V, const double* pw, double& u, double& v, double& xr) {
#pragma clang fp contract(off)
  const double d0 = pw[0] - V.t[0], d1 = pw[1] - V.t[1], d2 = pw[2] - V.t[2];
  const double x = (V.R[0] * d0 + V.R[3] * d1) + V.R[6] * d2;
  const double y = (V.R[1] * d0 + V.R[4] * d1) + V.R[7] * d2;
  const double z = (V.R[2] * d0 + V.R[5] * d1) + V.R[8] * d2;
  if (!(z > 0)) return RSPL_LMAP_BEHIND;  // pc(2) <= 0 (a NaN is behind as well)
  const double z_inv = 1.0 / z;
  u = x * z_inv * V.fx + V.cx;
  v = y * z_inv * V.fy + V.cy;
  xr = u - V.bf * z_inv;
  if (!(u > 0 && u < V.W && v > 0 && v < V.H)) return RSPL_LMAP_OFF_IMAGE;
  return RSPL_LMAP_GOOD;
}

// kxf, kyf: the keypoint as cv::KeyPoint holds it (float-rounded); ur: its u_right; has_ur: the frame has the array
RSPL_LMAP_HD bool in_box(double kxf, double kyf, double ur, bool has_ur, double u, double v, double xr, double r) {
#pragma clang fp contract(off)
  const double dx = kxf - u, dy = kyf - v;
  const double dxr = (has_ur && xr > 0) ? ur - xr : 0.0;
  return fabs(dx) < r && fabs(dy) < r && fabs(dxr) < r;
}

RSPL_LMAP_HD double to_float(double x) { return (double)(float)x; }

// std::round: half away from zero
RSPL_LMAP_HD int cell_key(double kx, double ky, double inv_w, double inv_h) {
#pragma clang fp contract(off)
  const double rx = round(kx * inv_w), ry = round(ky * inv_h);
  // (the comparisons are made on the doubles: a coordinate far outside never overflows the int, a NaN gives 0)
  const int gx = !(rx > 0) ? 0 : (rx > kGridCols - 1 ? kGridCols - 1 : (int)rx);
  const int gy = !(ry > 0) ? 0 : (ry > kGridRows - 1 ? kGridRows - 1 : (int)ry);
  return gx * kGridRows + gy;
}

RSPL_LMAP_HD double partial4(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3) {
#pragma clang fp contract(off)
  return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
}

RSPL_LMAP_HD double distance_of(double dot) {
#pragma clang fp contract(off)
  return 2.0 * (1.0 - dot);
}

struct Best {
  double best = 4.0, second = 4.0;
  int idx = -1, key = 0;
  // candidates arrive in ascending idx
  RSPL_LMAP_HD void visit(double d, int k, int i) {
    if (d < best || (d == best && idx >= 0 && k < key)) {
      second = best;
      best = d;
      idx = i;
      key = k;
    } else if (d < second) {
      second = d;
    }
  }
  RSPL_LMAP_HD bool good(const View& V) const {
#pragma clang fp contract(off)
    return best < V.max_distance && best < V.max_ratio * second;
  }
};

// the host's walk of the device's reduction tree over 64 emulated lane partials
inline double xsum64_host(double* p) {
#pragma clang fp contract(off)
  for (int o = 32; o >= 1; o >>= 1)
    for (int l = 0; l < o; l++) p[l] = p[l] + p[l + o];
  return p[0];
}

inline double distance_host(const double* a, const double* b) {
  double p[64];
  for (int l = 0; l < 64; l++)
    p[l] = partial4(a[4 * l], a[4 * l + 1], a[4 * l + 2], a[4 * l + 3], b[4 * l], b[4 * l + 1], b[4 * l + 2], b[4 * l + 3]);
  return distance_of(xsum64_host(p));
}

}  // namespace lmap
}  // namespace rspl
