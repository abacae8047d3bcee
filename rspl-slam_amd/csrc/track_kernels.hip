// The device-side glue of the tracking step (MapBuilder::TrackFrame + FramePoseOptimization,
// src/map_builder.cc:448-611) around the PnP and FrameOptimization kernels: what the reference does on
// the host between SuperGlue and the two solvers, and after them, as three small kernels so that the
// whole step is one stream-ordered chain.
//   track_gather_kernel  matches -> ordered correspondences / edges, the solvers' descriptors, RANSAC subsets
//   track_seed_kernel    PnP's result -> the gate of :517-521 -> FrameOptimization's initial T_cw
//   track_write_kernel   FrameOptimization's flags -> track ids, kept matches, the pose
// Ordering: every compaction is a ballot + lane-count prefix inside a wave, wave totals through LDS and a
// running base over chunks of 256 keypoints -- no atomics, so slot order is ascending keypoint index, the
// reference's loop order, by construction.
#include "ransac.hpp"
#include "se3_device.hpp"
#include "track_kernels.hpp"
#include "wave_reduce.hpp"

namespace rspl {
namespace track {
namespace {

constexpr int T = 256, NW = 4;

using ransac::mutual_partner;
using ransac::subset_at;
using wave::lanes_below;

// SE3Quat::inverse as frame.cpp's host code spells it
__device__ __forceinline__ ba::SE3 se3_inverse(const ba::SE3& X) {
  #pragma clang fp contract(off)  // the bits of the conversion do not depend on what the optimiser fuses
  ba::SE3 r;
  r.q[0] = X.q[0]; r.q[1] = -X.q[1]; r.q[2] = -X.q[2]; r.q[3] = -X.q[3];
  double R[9], t[3];
  ba::q_to_R(r.q, R);
  ba::mat3_vec(R, X.t, t);
  for (int i = 0; i < 3; i++) r.t[i] = -t[i];
  ba::se3_normalize(r);
  return r;
}

// rotation matrix (row-major) | translation -> SE3Quat, normalised (Eigen's Quaterniond(Matrix3d), then
// SE3Quat::normalizeRotation as rspl_frame_optimize applies it to the caller's pose)
__device__ __forceinline__ ba::SE3 se3_from_Rt(const double* R, const double* t) {
  ba::SE3 X;
  ba::R_to_q(R, X.q);
  for (int i = 0; i < 3; i++) X.t[i] = t[i];
  ba::se3_normalize(X);
  return X;
}

__global__ __launch_bounds__(T) void track_gather_kernel(Args a) {
  __shared__ int wtot[NW][2];
  __shared__ int dv[kDrawCap];            // draws % count
  __shared__ unsigned short run[kDrawCap];  // draws a subset started at k consumes
  __shared__ int start[pnp::kMaxIters];
  const int f = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const Param P = a.host_params[f];
  if (tid == 0) a.params[f] = P;
  const int K = a.K;
  const size_t o = (size_t)f * K;
  int n1 = *P.n1;
  n1 = n1 < 0 ? 0 : (n1 > K ? K : n1);

  // pass 1: the mutual check (point_matching.cc:24-31), `inliers` (map_builder.cc:457-466), the counts
  int nmatch = 0, nmono = 0, nstereo = 0;
  for (int i = tid; i < K; i += T) {
    int j = -1, t = -1;
    bool keep = false, st = false;
    if (i < n1) {
      const int jj = mutual_partner(P.idx1, P.idx0, i, P.n0);
      if (jj >= 0) {
        j = jj;
        t = P.kf_tid[jj];
        keep = P.kf_state[jj] == 1;
        st = keep && P.u_right && P.u_right[i] > 0;
      }
    }
    a.match_kf[o + i] = j;
    a.inl_tid[o + i] = t;
    a.kp_edge[o + i] = -1;
    nmatch += j >= 0;
    nmono += keep && !st;
    nstereo += st;
  }
  nmatch = wave::block_sum_int<NW>(nmatch);
  nmono = wave::block_sum_int<NW>(nmono);
  nstereo = wave::block_sum_int<NW>(nstereo);
  const int count = nmono + nstereo;  // <= min(n0, n1) <= K: a keyframe keypoint has one mutual partner

  // pass 2: placement.  Correspondence slot = kept keypoints before i; edge slot = mono edges before i, or
  // all mono edges + stereo edges before i (the order rspl_frame_optimize packs).
  int bc = 0, bm = 0, bs = nmono;
  for (int c = 0; c < n1; c += T) {
    const int i = c + tid;
    int j = -1;
    bool keep = false, st = false;
    if (i < n1) {
      j = a.match_kf[o + i];  // this thread's own store of pass 1
      keep = j >= 0 && P.kf_state[j] == 1;
      st = keep && P.u_right && P.u_right[i] > 0;
    }
    const unsigned long long mk = __ballot(keep), ms = __ballot(st);
    if (lane == 0) {
      wtot[wv][0] = __popcll(mk);
      wtot[wv][1] = __popcll(ms);
    }
    __syncthreads();
    int ok = 0, os = 0, tk = 0, ts = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const int k = wtot[w][0], s = wtot[w][1];
      if (w < wv) {
        ok += k;
        os += s;
      }
      tk += k;
      ts += s;
    }
    if (keep) {
      const int kb = ok + lanes_below(mk), sb = os + lanes_below(ms);  // kept / stereo keypoints of the chunk before i
      const int cs = bc + kb;
      const int e = st ? bs + sb : bm + (kb - sb);
      const double* X = P.kf_points + 3 * (size_t)j;
      const double* fr = P.feat + 259 * (size_t)i;
      const double x0 = X[0], x1 = X[1], x2 = X[2], u = fr[1], v = fr[2];
      a.corr_kp[o + cs] = i;
      double* pp = a.pts + 3 * (o + cs);
      pp[0] = (double)(float)x0;  // cv::Point3f / cv::Point2f (g2o_optimization.cc:425-426)
      pp[1] = (double)(float)x1;
      pp[2] = (double)(float)x2;
      double* pk = a.kps + 2 * (o + cs);
      pk[0] = (double)(float)u;
      pk[1] = (double)(float)v;
      static_assert(sizeof(frame::Edge) == 96, "six 16-byte stores per edge record");
      double2* E = reinterpret_cast<double2*>(a.edges + o + e);
      E[0] = make_double2(x0, x1);
      E[1] = make_double2(x2, u);
      E[2] = make_double2(v, st ? P.u_right[i] : 0.0);
      E[3] = make_double2(P.cam[0], P.cam[1]);
      E[4] = make_double2(P.cam[2], P.cam[3]);
      E[5] = make_double2(P.cam[4], st ? 1.0 : 0.0);
      a.inl_in[o + e] = 1;  // constraint->inlier = true (map_builder.cc:563, 573)
      a.edge_kp[o + e] = i;
      a.kp_edge[o + i] = e;
    }
    bc += tk;
    bs += ts;
    bm += tk - ts;
    __syncthreads();  // wtot is rewritten by the next chunk
  }

  const int iters = count >= 8 ? P.iters : 0;  // < 8 correspondences: SolvePnPWithCV returns 0 (:433)
  if (tid == 0) {
    pnp::Desc d;
    d.p0 = (int)o;
    d.n = count;
    d.s0 = f * pnp::kMaxIters;
    d.iters = iters;
    for (int k = 0; k < 4; k++) d.K[k] = P.cam[k];
    d.thr2 = P.thr2;
    d.confidence = P.confidence;
    a.pnp_desc[f] = d;
    frame::Desc* fd = a.frame_desc + f;  // T0 is the seed kernel's
    fd->e0 = (int)o;
    fd->n = count;
    fd->pad[0] = fd->pad[1] = 0;
    fd->delta[0] = P.delta[0]; fd->delta[1] = P.delta[1];
    fd->th[0] = P.th[0]; fd->th[1] = P.th[1];
    int* cn = a.counts + 4 * f;
    cn[0] = n1; cn[1] = nmatch; cn[2] = nmono; cn[3] = nstereo;
  }
  if (iters == 0) return;  // uniform

  // RANSAC's subsets for `count` (csrc/pnp.cpp subsets()).  The raw draws do not depend on the count; which
  // draw a subset starts at does (a duplicate draws again).  run[k] = the draws a subset started at k would
  // consume, for every k side by side; the starts are then a chain of `iters` LDS look-ups.
  const int nd = a.n_draws < kDrawCap ? a.n_draws : kDrawCap;
  for (int k = tid; k < nd; k += T) dv[k] = (int)(a.draws[k] % (unsigned)count);
  __syncthreads();
  for (int k = tid; k < nd; k += T) {
    int v[5];
    run[k] = (unsigned short)subset_at(dv, nd, k, v);
  }
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int h = 0; h < iters; h++) {
      start[h] = s;
      const int L = s < nd ? run[s] : 0;
      s = L ? s + L : nd;
    }
  }
  __syncthreads();
  if (tid < iters) {
    int v[5];
    // (the table is sized at create for every count this handle can see, so a start is always inside it;
    // an out-of-table start still yields in-range indices)
    if (start[tid] >= nd || !subset_at(dv, nd, start[tid], v))
      for (int k = 0; k < 5; k++) v[k] = k;
    int32_t* sub = a.subsets + 5 * ((size_t)f * pnp::kMaxIters + tid);
#pragma unroll
    for (int k = 0; k < 5; k++) sub[k] = v[k];
  }
}

// one thread per frame
__global__ __launch_bounds__(64) void track_seed_kernel(Args a, int batch) {
  #pragma clang fp contract(off)
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= batch) return;
  const Param& P = a.params[f];
  const pnp::Out* O = a.pnp_out + f;
  const int ninl = O->n_inliers;
  bool use = ninl > 0 && !(ninl < P.min_match);
  double R[9], t[3];
  if (use) {  // (Rwc | twc are written only when PnP found a model)
    for (int k = 0; k < 9; k++) R[k] = O->Rwc[k];
    for (int k = 0; k < 3; k++) t[k] = O->twc[k];
    const double dx = t[0] - P.last[9], dy = t[1] - P.last[10], dz = t[2] - P.last[11];
    use = !(sqrt(dx * dx + dy * dy + dz * dz) > 0.5);  // check_dp.norm() > 0.5 (map_builder.cc:517-518)
  }
  if (!use) {
    for (int k = 0; k < 9; k++) R[k] = P.last[k];
    for (int k = 0; k < 3; k++) t[k] = P.last[9 + k];
  }
  const ba::SE3 Twc = se3_from_Rt(R, t);
  const ba::SE3 Tcw = se3_inverse(Twc);  // VertexSE3Expmap estimate = SE3Quat(q, p).inverse() (g2o_optimization.cc:265)
  frame::Desc* fd = a.frame_desc + f;
  for (int k = 0; k < 4; k++) fd->T0[k] = Tcw.q[k];
  for (int k = 0; k < 3; k++) fd->T0[4 + k] = Tcw.t[k];
  fd->T0[7] = 0;
  Seed* sd = a.seed + f;
  sd->q[0] = Twc.q[1]; sd->q[1] = Twc.q[2]; sd->q[2] = Twc.q[3]; sd->q[3] = Twc.q[0];
  for (int k = 0; k < 3; k++) sd->p[k] = Twc.t[k];
  sd->pnp_used = use;
  sd->pad = 0;
}

__global__ __launch_bounds__(T) void track_write_kernel(Args a) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const Param& P = a.params[f];
  const frame::Out* FO = a.frame_out + f;
  const size_t o = (size_t)f * a.K;
  const int* cn = a.counts + 4 * f;
  const int n1 = cn[0];
  const int ninl = FO->n_inliers;
  const bool pose_set = ninl > P.min_match;  // (map_builder.cc:586, :472)
  int nk = 0;
  for (int i = tid; i < n1; i += T) {
    const int j = a.match_kf[o + i];
    int t = a.inl_tid[o + i];
    if (pose_set) {  // an edge FrameOptimization flagged: inliers[idx] = -1 (:594-606)
      const int e = a.kp_edge[o + i];
      if (e >= 0 && !a.edge_inl[o + e]) t = -1;
    }
    int tid_out = -1;
    uint8_t kept = 0;
    if (j >= 0) {
      if (!pose_set) kept = 1;   // no track id is assigned and no match removed
      else if (t > 0) {          // inliers[idx1] > 0, strictly: track id 0 is dropped as in the reference (:476-486)
        tid_out = t;
        kept = 1;
      }
    }
    a.o_match_kf[o + i] = j;
    a.o_track_id[o + i] = tid_out;
    a.o_kept[o + i] = kept;
    nk += kept;
  }
  nk = wave::block_sum_int<NW>(nk);
  if (tid == 0) {
    ba::SE3 Twc;
    if (pose_set) {  // pose = estimate().inverse() (g2o_optimization.cc:394-396)
      ba::SE3 Tcw;
      for (int k = 0; k < 4; k++) Tcw.q[k] = FO->T[k];
      for (int k = 0; k < 3; k++) Tcw.t[k] = FO->T[4 + k];
      Twc = se3_inverse(Tcw);
    } else {
      Twc = se3_from_Rt(P.last, P.last + 9);
    }
    Out* r = a.out + f;
    r->q[0] = Twc.q[1]; r->q[1] = Twc.q[2]; r->q[2] = Twc.q[3]; r->q[3] = Twc.q[0];
    for (int k = 0; k < 3; k++) r->p[k] = Twc.t[k];
    for (int k = 0; k < 4; k++) {
      r->chi2[k] = FO->chi2[k];
      r->iters[k] = FO->iters[k];
    }
    r->pose_set = pose_set;
    r->n_inliers = ninl;
    r->n_pnp = a.pnp_out[f].n_inliers;
    r->pnp_used = a.seed[f].pnp_used;
    r->n1 = n1;
    r->n_matches = cn[1];
    r->n_kept = nk;
    r->n_mono = cn[2];
    r->n_stereo = cn[3];
    r->rounds = FO->rounds;
  }
}

}  // namespace

hipError_t gather(const Args& a, int batch, hipStream_t s) {
  track_gather_kernel<<<batch, T, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t seed(const Args& a, int batch, hipStream_t s) {
  track_seed_kernel<<<(batch + 63) / 64, 64, 0, s>>>(a, batch);
  return hipGetLastError();
}

hipError_t write_back(const Args& a, int batch, hipStream_t s) {
  track_write_kernel<<<batch, T, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace track
}  // namespace rspl
