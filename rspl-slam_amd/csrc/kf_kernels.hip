// The device side of keyframe insertion: what the reference does on the host between SuperGlue's stereo
// pair and the map (MapBuilder::InsertKeyframe, map_builder.cc:639-682; Frame::AddRightFeatures,
// frame.cc:150-177; the map-point half of Map::InsertKeyframe, map.cc:40-55; MapBuilder::Init's ids,
// map_builder.cc:390-403).
//   kf_stereo_kernel       one 256-thread workgroup per frame: mutual check, disparity window, u_right and
//                          depth, new track ids, new map points, the tracker's keyframe table
//   kf_triangulate_kernel  Map::TriangulateMappoint (map.cc:292-339), one lane per map point
// Ordering: the id ranks are a ballot + lane-count prefix inside a wave, wave totals through LDS and a
// running base over chunks of 256 keypoints -- no atomics, ids ascend with the keypoint index as the
// reference's loops assign them.
#include "kf_kernels.hpp"
#include "kf_triangulate.hpp"
#include "line_kernels.hpp"
#include "ransac.hpp"
#include "wave_reduce.hpp"

namespace rspl {
namespace kf {
namespace {

constexpr int T = 256, NW = 4;
using wave::lanes_below;

// keypoint i of the left image: its mutual partner inside the disparity window (frame.cc:157-177).
// Returns 1 for a mutual match, 3 for one the window keeps; u_right / depth are -1 unless kept.
__device__ __forceinline__ int stereo_at(const Param& P, int i, int nl, int nr, double& xl, double& yl, double& ur,
                                         double& depth) {
  #pragma clang fp contract(off)
  ur = -1.0;
  depth = -1.0;
  const double* l = P.feat_l + 259 * (size_t)i;
  xl = l[1];
  yl = l[2];
  const int j = ransac::mutual_partner(P.idx0, P.idx1, i, nr);
  if (j < 0) return 0;
  const double* r = P.feat_r + 259 * (size_t)j;
  const double xr = r[1], yr = r[2];
  if (!lines::in_disparity_window(xl, yl, xr, yr, P.win[0], P.win[1], P.win[2])) return 1;
  ur = xr;
  depth = P.cam[4] / (xl - xr);  // the signed difference: a partner to the right gives a negative depth
  return 3;
}

// Rwf * (BackProjectStereo) + twf (map.cc:49-51, camera.cc:150-161)
__device__ __forceinline__ void back_project(const Param& P, double x, double y, double ur, double fx_inv,
                                             double fy_inv, double* pw) {
  #pragma clang fp contract(off)
  const double d = P.cam[4] / (x - ur);
  const double pf0 = ((x - P.cam[2]) * fx_inv) * d, pf1 = ((y - P.cam[3]) * fy_inv) * d, pf2 = 1.0 * d;
#pragma unroll
  for (int r = 0; r < 3; r++) pw[r] = (P.Twc[3 * r] * pf0 + P.Twc[3 * r + 1] * pf1 + P.Twc[3 * r + 2] * pf2) + P.Twc[9 + r];
}

__global__ __launch_bounds__(T) void kf_stereo_kernel(Args a) {
  #pragma clang fp contract(off)
  __shared__ int wtot[NW][2];
  const int f = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const Param P = a.params[f];
  const int K = a.K;
  const size_t o = (size_t)f * K;
  int nl = *P.n_l, nr = *P.n_r;
  nl = nl < 0 ? 0 : (nl > K ? K : nl);
  nr = nr < 0 ? 0 : (nr > K ? K : nr);
  const double fx_inv = 1.0 / P.cam[0], fy_inv = 1.0 / P.cam[1];

  // pass 1: the counts; with init, the keypoints with a depth take their ids before all the others
  int nmatch = 0, nkept = 0, npos = 0;
  for (int i = tid; i < nl; i += T) {
    double xl, yl, ur, dp;
    const int s = stereo_at(P, i, nl, nr, xl, yl, ur, dp);
    nmatch += s & 1;
    nkept += s >> 1;
    npos += dp > 0.0;
  }
  nmatch = wave::block_sum_int<NW>(nmatch);
  nkept = wave::block_sum_int<NW>(nkept);
  npos = wave::block_sum_int<NW>(npos);

  // pass 2: ids in ascending keypoint order.  Class A: keypoints without an id (init: with a depth);
  // class B (init only): the keypoints without a depth, numbered after all of class A.
  int baseA = 0, baseB = P.init ? npos : 0, npts = 0, ngood = 0;
  for (int c = 0; c < nl; c += T) {
    const int i = c + tid;
    const bool in = i < nl;
    double xl = 0, yl = 0, ur = -1.0, dp = -1.0;
    int tin = -1, slot = -1;
    if (in) {
      stereo_at(P, i, nl, nr, xl, yl, ur, dp);
      if (!P.init && P.track_id && i < P.n_host) tin = P.track_id[i];
      if (P.point_slot && i < P.n_host) slot = P.point_slot[i];
    }
    const bool pos = dp > 0.0;
    const bool A = in && (P.init ? pos : tin < 0), B = in && P.init && !pos;
    const unsigned long long mA = __ballot(A), mB = __ballot(B);
    if (lane == 0) {
      wtot[wv][0] = __popcll(mA);
      wtot[wv][1] = __popcll(mB);
    }
    __syncthreads();
    int oA = 0, oB = 0, tA = 0, tB = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const int x = wtot[w][0], y = wtot[w][1];
      if (w < wv) {
        oA += x;
        oB += y;
      }
      tA += x;
      tB += y;
    }
    if (in) {
      int t = tin;
      if (A) t = P.next_track_id + baseA + oA + lanes_below(mA);
      else if (B) t = P.next_track_id + baseB + oB + lanes_below(mB);
      // a new map point for a keypoint that holds none (map.cc:42-55); Init creates none without a depth
      int np = 0;
      double pw[3] = {0.0, 0.0, 0.0};
      if (slot < 0 && t >= 0) np = pos ? 1 : (P.init ? 0 : 2);
      if (np == 1) back_project(P, xl, yl, ur, fx_inv, fy_inv, pw);
      a.u_right[o + i] = ur;
      a.depth[o + i] = dp;
      a.track_id[o + i] = t;
      a.new_point[o + i] = (uint8_t)np;
      double* q = a.new_position + 3 * (o + i);
      q[0] = pw[0]; q[1] = pw[1]; q[2] = pw[2];
      npts += np != 0;
      ngood += np == 1;
      if (P.tbl_points && i < P.tbl_cap) {
        uint8_t st = np == 1 ? 1 : (np == 2 ? 2 : 0);  // RSPL_TRACK_GOOD / NOT_GOOD / NO_MAPPOINT
        if (slot >= 0) {
          st = P.state[i];
          pw[0] = P.points[3 * (size_t)i]; pw[1] = P.points[3 * (size_t)i + 1]; pw[2] = P.points[3 * (size_t)i + 2];
        }
        double* tp = P.tbl_points + 3 * (size_t)i;
        tp[0] = pw[0]; tp[1] = pw[1]; tp[2] = pw[2];
        P.tbl_state[i] = st;
        P.tbl_tid[i] = t;
      }
    }
    baseA += tA;
    baseB += tB;
    __syncthreads();  // wtot is rewritten by the next chunk
  }
  npts = wave::block_sum_int<NW>(npts);
  ngood = wave::block_sum_int<NW>(ngood);
  if (tid == 0) {
    const int nnew = baseA + baseB - (P.init ? npos : 0);
    Out r;
    r.n_keypoints = nl;
    r.n_matches = nmatch;
    r.n_stereo_matches = nkept;
    r.n_new_ids = nnew;
    r.n_new_points = npts;
    r.n_new_good = ngood;
    r.next_track_id = P.next_track_id + nnew;
    r.pad = 0;
    a.out[f] = r;
  }
}

__global__ __launch_bounds__(64) void kf_triangulate_kernel(TriArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  const int o = a.offsets[i], n = a.offsets[i + 1] - o;
  double p[3];
  const int rc = triangulate_point(a.Twc, a.obs_pose + o, a.obs_xy + 2 * (size_t)o, n, a.cam, p, nullptr);
  a.position[3 * (size_t)i] = p[0];
  a.position[3 * (size_t)i + 1] = p[1];
  a.position[3 * (size_t)i + 2] = p[2];
  a.status[i] = (uint8_t)rc;
}

}  // namespace

hipError_t stereo(const Args& a, int batch, hipStream_t s) {
  kf_stereo_kernel<<<batch, T, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t triangulate(const TriArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  kf_triangulate_kernel<<<(a.n + 63) / 64, 64, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace kf
}  // namespace rspl
