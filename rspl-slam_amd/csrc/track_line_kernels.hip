// Line tracking and the keyframe decision of the tracking step (track_line_kernels.hpp): the line half of
// MapBuilder::TrackFrame (src/map_builder.cc:450-455, 490-501) and MapBuilder::AddKeyframe (:616-636) as one
// launch per batch behind track_write_kernel, plus one launch per keyframe for the slot's tables.
//
// The on-line test, the CSR scan and the first-maximum argmax are line_kernels.hip's (line_device.hpp), and
// MatchLines follows match_kernel phase by phase.  What differs is where the operands live: the point matches
// are the gather kernel's match_kf (the pairs (match_kf[i], i) before the removal of :472-488), the keyframe
// side's CSR and inverse incidence were computed once per keyframe and stay in the slot, so a frame's
// workgroup carries only the frame's own keypoint tables in LDS (~45 KB against match_kernel's ~70 KB).
// Integer work in a fixed order (ballot compaction; counts): bitwise reproducible.
#include "../../include/rspl.h"
#include "line_device.hpp"
#include "line_kernels.hpp"
#include "se3_device.hpp"
#include "track_line_kernels.hpp"
#include "wave_reduce.hpp"

namespace rspl {
namespace track {
namespace {

constexpr int T = 1024, NW = 16;
constexpr int kMaxLines = 1024;
using lines::kMaxPointsLds;

// AddKeyframe (:616-636) on the pose rspl_track_result reports.  delta_angle = Eigen::AngleAxisd(R_kf^T R)
// .angle(): rotation matrix -> quaternion (Eigen's Quaterniond(Matrix3d) = R_to_q), then 2 atan2(|vec|, |w|).
__device__ void decide(const LineParam& LP, const Out* r, int min_match, LineOut& o) {
#pragma clang fp contract(off)
  const double q[4] = {r->q[3], r->q[0], r->q[1], r->q[2]};  // w x y z
  double R[9], D[9], dq[4];
  ba::q_to_R(q, R);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) D[3 * i + j] = LP.kf_R[i] * R[j] + LP.kf_R[3 + i] * R[3 + j] + LP.kf_R[6 + i] * R[6 + j];
  ba::R_to_q(D, dq);
  const double n = sqrt(dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
  const double angle = n != 0 ? 2 * atan2(n, fabs(dq[0])) : 0.0;
  const double dx = r->p[0] - LP.kf_t[0], dy = r->p[1] - LP.kf_t[1], dz = r->p[2] - LP.kf_t[2];
  const double dist = sqrt(dx * dx + dy * dy + dz * dz);
  const int passed = LP.frame_id - LP.kf_frame_id;
  const int num_match = r->n_inliers;
  o.tracked_well = num_match >= min_match;  // _last_frame_track_well (:240)
  o.add_keyframe = (num_match < LP.max_num_match ? RSPL_TRACK_KF_NOT_ENOUGH_MATCH : 0) |
                   (angle > LP.max_angle ? RSPL_TRACK_KF_LARGE_DELTA_ANGLE : 0) |
                   (dist > LP.max_distance ? RSPL_TRACK_KF_LARGE_DISTANCE : 0) |
                   (passed > LP.max_num_passed_frame ? RSPL_TRACK_KF_ENOUGH_PASSED_FRAME : 0);
  o.passed_frames = passed;
  o.pad = 0;
  o.delta_angle = angle;
  o.delta_distance = dist;
}

// keypoint -> lines inverse incidence of a CSR (offs in LDS, idx in global): c[0 .. np] = starts (LDS),
// kline = the lines, fill = np ints of LDS scratch.  Order within a keypoint is irrelevant: only counts follow.
__device__ void inverse_incidence(const int* offs, const int* idx, int nl, int np, int* c, int* fill, int* kline,
                                  int* part) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tot = offs[nl];
  for (int i = tid; i < np; i += T) c[i] = fill[i] = 0;
  __syncthreads();
  for (int e = tid; e < tot; e += T) atomicAdd(&c[idx[e]], 1);
  __syncthreads();
  lines::block_excl_scan(c, np, part);
  if (tid == 0) c[np] = tot;
  __syncthreads();
  for (int l = wv; l < nl; l += NW)
    for (int e = offs[l] + lane; e < offs[l + 1]; e += 64) {
      const int t = idx[e];
      kline[c[t] + atomicAdd(&fill[t], 1)] = l;
    }
  __syncthreads();
}

__global__ __launch_bounds__(T) void track_kf_lines_kernel(LineArgs g, int slot, const double* L, int nl,
                                                           const double* feat, const int32_t* d_n0) {
  __shared__ int c0[kMaxPointsLds + 1], f0[kMaxPointsLds];
  __shared__ int cnt[kMaxLines + 1];
  __shared__ int part[16];
  const int tid = threadIdx.x, K = g.K;
  int np = *d_n0;
  np = np < 0 ? 0 : (np > K ? K : np);
  int* off = g.kf_off + (size_t)slot * (g.max_lines + 1);
  int* idx = g.kf_idx + (size_t)slot * g.cap;
  int* kstart = g.kf_kstart + (size_t)slot * (K + 1);
  const int tot = lines::assign_lines(L, nl, feat + 1, 259, np, off, idx, g.kf_dist + (size_t)slot * g.cap, g.cap, cnt, part);
  const bool over = tot > g.cap;  // uniform
  if (tid == 0) g.kf_status[slot] = over;
  // The starts cover all K keypoints, whatever count the slot's point table is given later: a match index
  // below K always finds a (possibly empty) range.  An overflowed slot keeps no incidence.
  if (over) {
    for (int i = tid; i <= K; i += T) kstart[i] = 0;
    return;
  }
  inverse_incidence(cnt, idx, nl, K, c0, f0, g.kf_kline + (size_t)slot * g.cap, part);
  for (int i = tid; i <= K; i += T) kstart[i] = c0[i];
}

// MatchLines' phases as match_kernel numbers them; phase 7 is the id copy of :490-501.
__global__ __launch_bounds__(T) void track_lines_kernel(Args a, LineArgs g) {
  __shared__ int c1[kMaxPointsLds + 1], f1[kMaxPointsLds];
  __shared__ int cnt[kMaxLines + 1];
  __shared__ int part[16];
  __shared__ int rowloc[kMaxLines], lmatch[kMaxLines];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const LineParam LP = g.lparams[f];
  const Param& P = a.params[f];
  const int K = a.K, ML = g.max_lines;
  const int n1 = a.counts[4 * f], np0 = P.n0, nl0 = LP.kf_n_lines, nl1 = LP.n_lines;
  LineOut o;
  if (tid == 0) decide(LP, a.out + f, P.min_match, o);  // (kept in thread 0's registers until the last store)
  for (int j = tid; j < nl1; j += T) lmatch[j] = -1;
  bool over = false;
  if (nl1 > 0) {
    int* idx1 = g.idx + (size_t)f * g.cap;
    const int tot1 = lines::assign_lines(LP.lines, nl1, P.feat + 1, 259, n1, g.off + (size_t)f * (ML + 1), idx1,
                                         g.dist + (size_t)f * g.cap, g.cap, cnt, part);
    over = tot1 > g.cap || (nl0 > 0 && g.kf_status[LP.slot]);
    if (!over && np0 > 0 && n1 > 0 && nl0 > 0) {  // (:231; uniform)
      const int* off0 = g.kf_off + (size_t)LP.slot * (ML + 1);
      const int* k0 = g.kf_kstart + (size_t)LP.slot * (K + 1);
      const int* kline0 = g.kf_kline + (size_t)LP.slot * g.cap;
      int* kline1 = g.kline + (size_t)f * g.cap;
      int* M = g.M + (size_t)f * ML * ML;
      for (int i = tid; i < nl0 * nl1; i += T) M[i] = 0;
      inverse_incidence(cnt, idx1, nl1, n1, c1, f1, kline1, part);  // phases 1-3 for the frame's side
      const int32_t* mk = a.match_kf + (size_t)f * K;
      for (int i = tid; i < n1; i += T) {  // phase 4: the match (q, i)
        const int q = mk[i];
        if (q < 0 || q >= K) continue;
        for (int u = k0[q]; u < k0[q + 1]; u++) {
          int* row = M + (size_t)kline0[u] * nl1;
          for (int v = c1[i]; v < c1[i + 1]; v++) atomicAdd(&row[kline1[v]], 1);
        }
      }
      __syncthreads();
      for (int r = wv; r < nl0; r += NW) {  // phase 5
        int best = -1, bi = 0;
        for (int j = lane; j < nl1; j += 64) {
          const int v = M[(size_t)r * nl1 + j];
          if (v > best) {
            best = v;
            bi = j;
          }
        }
        lines::wave_first_max(best, bi);
        if (lane == 0) rowloc[r] = bi;
      }
      __syncthreads();
      for (int j = wv; j < nl1; j += NW) {  // phase 6
        int best = -1, bi = 0;
        for (int r = lane; r < nl0; r += 64) {
          const int v = M[(size_t)r * nl1 + j];
          if (v > best) {
            best = v;
            bi = r;
          }
        }
        lines::wave_first_max(best, bi);
        if (lane == 0) {
          if (best < 2 || rowloc[bi] != j) continue;
          const int sz0 = off0[bi + 1] - off0[bi], sz1 = cnt[j + 1] - cnt[j];
          const float score = (float)(best * best) / (float)(sz0 < sz1 ? sz0 : sz1);
          if (score < 0.8f) continue;
          lmatch[j] = bi;  // line_matches[bi] = j; injective by the mutual test
        }
      }
    }
  }
  __syncthreads();
  // phase 7: the keyframe line's track id and map line go to its matched line; id 0 is a track (>= 0, :497)
  const int32_t* ktid = g.kf_ltid + (size_t)LP.slot * ML;
  const int32_t* kslot = g.kf_lslot + (size_t)LP.slot * ML;
  int nm = 0, nt = 0;
  for (int j = tid; j < nl1; j += T) {
    const int i = lmatch[j];
    int t = -1, s = -1;
    if (i >= 0 && ktid[i] >= 0) {
      t = ktid[i];
      s = kslot[i];
    }
    const size_t w = (size_t)f * ML + j;
    g.line_match[w] = g.o_line_match[w] = i;
    g.line_tid[w] = g.o_line_tid[w] = t;
    g.line_slot[w] = g.o_line_slot[w] = s;
    nm += i >= 0;
    nt += t >= 0;
  }
  nm = wave::block_sum_int<NW>(nm);
  nt = wave::block_sum_int<NW>(nt);
  if (tid == 0) {
    o.n_lines = nl1;
    o.n_matches = nm;
    o.n_tracks = nt;
    o.overflow = over;
    g.out[f] = o;
  }
}

}  // namespace

hipError_t kf_lines(const LineArgs& g, int slot, const double* d_lines, int n_lines, const double* d_features,
                    const int32_t* d_n0, hipStream_t s) {
  track_kf_lines_kernel<<<1, T, 0, s>>>(g, slot, d_lines, n_lines, d_features, d_n0);
  return hipGetLastError();
}

hipError_t frame_lines(const Args& a, const LineArgs& g, int batch, hipStream_t s) {
  track_lines_kernel<<<batch, T, 0, s>>>(a, g);
  return hipGetLastError();
}

}  // namespace track
}  // namespace rspl
