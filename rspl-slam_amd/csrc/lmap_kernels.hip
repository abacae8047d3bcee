// Local map tracking on the device: Map::SearchByProjection (src/map.cc:952-1005) and the merge loop of
// MapBuilder::TrackLocalMap (src/map_builder.cc:763-768) for a batch of frames.
//   lmap_store_kernel   Mappoint::SetDescriptor at creation: record rows 3..258 -> a bank row
//   lmap_prep_kernel    the frame's keypoints as every wave of the search reads them -- x, y (float-rounded),
//                       u_right, grid cell key / candidate flag -- 28 bytes per keypoint instead of the records'
//                       2 KB stride
//   lmap_search_kernel  one wave per local map point: its descriptor in registers (4 doubles per lane), the
//                       projection, then the keypoints 64 at a time: each lane tests its keypoint, the ballot's
//                       set bits are walked wave-uniformly with one wave-wide dot product per candidate
//   lmap_merge_kernel   one block per frame: the good list compacted in local order (a contiguous quarter per
//                       wave, ballot + prefix, no atomics in the order), "last wins" as an integer atomicMax of
//                       the local index per keypoint, the merged table into the tracker's keyframe slot
// The arithmetic is csrc/lmap_match.hpp's, shared with the host; the dot product's tree is wave::xsum64.
#include "lmap_kernels.hpp"
#include "wave_reduce.hpp"

namespace rspl {
namespace lmap {
namespace {

constexpr int T = 256, NW = 4;

__global__ __launch_bounds__(64) void lmap_store_kernel(double* bank, const double* feat, const int32_t* pairs) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const int row = pairs[2 * k], kp = pairs[2 * k + 1];
  const double* src = feat + RSPL_FEATURE_ROWS * (size_t)kp + 3 + 4 * lane;  // 8-byte aligned only
  const double s0 = src[0], s1 = src[1], s2 = src[2], s3 = src[3];
  double2* dst = reinterpret_cast<double2*>(bank + kDesc * (size_t)row) + 2 * lane;
  dst[0] = make_double2(s0, s1);
  dst[1] = make_double2(s2, s3);
}

__global__ __launch_bounds__(T) void lmap_prep_kernel(Args a) {
  const int f = blockIdx.y, i = blockIdx.x * T + threadIdx.x;
  const Param& P = a.host_params[f];
  const int K = a.K;
  int n1 = *P.n1;
  n1 = n1 < 0 ? 0 : (n1 > K ? K : n1);
  if (i == 0) {
    a.params[f] = P;
    a.n1c[f] = n1;
  }
  if (i >= K) return;
  const size_t o = (size_t)f * K + i;
  double x = 0, y = 0, ur = -1.0;
  int key = -1;
  if (i < n1) {
    const double* r = P.feat + RSPL_FEATURE_ROWS * (size_t)i;
    const double rx = r[1], ry = r[2];
    if (P.pid[i] < 0) key = cell_key(rx, ry, P.V.inv_w, P.V.inv_h);  // filter: a keypoint holding a point is skipped
    x = to_float(rx);
    y = to_float(ry);
    if (P.u_right) ur = P.u_right[i];
  }
  a.kx[o] = x;
  a.ky[o] = y;
  a.kur[o] = ur;
  a.kkey[o] = key;
}

__global__ __launch_bounds__(T) void lmap_search_kernel(Args a, int n_local) {
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int p = blockIdx.x * NW + (threadIdx.x >> 6);
  if (p >= n_local) return;  // wave-uniform; the kernel has no block barrier
  const Param& P = a.params[f];
  const View& V = P.V;
  const int K = a.K, n1 = a.n1c[f];
  const size_t ok = (size_t)f * K, op = (size_t)f * a.L + p;
  const int id = a.local_id[p];

  int status = RSPL_LMAP_GOOD;
  Best b;
  // SearchLocalPoints: a local point the frame already holds is not selected
  bool held = false;
  for (int i = lane; i < n1; i += 64) held |= P.pid[i] == id;
  double u = 0, v = 0, xr = 0;
  if (__ballot(held)) {
    status = RSPL_LMAP_NOT_SELECTED;
  } else {
    const double* pw = a.local_pos + 3 * (size_t)p;
    const double w[3] = {pw[0], pw[1], pw[2]};
    status = project(V, w, u, v, xr);
  }
  if (status == RSPL_LMAP_GOOD) {
    const double2* dp = reinterpret_cast<const double2*>(a.bank + kDesc * (size_t)a.local_row[p]) + 2 * lane;
    const double2 d01 = dp[0], d23 = dp[1];
    const bool has_ur = P.u_right != nullptr;
    bool any = false;
    for (int c = 0; c < n1; c += 64) {
      const int i = c + lane;
      int key = -1;
      bool cand = false;
      if (i < n1) {
        key = a.kkey[ok + i];
        cand = key >= 0 && in_box(a.kx[ok + i], a.ky[ok + i], a.kur[ok + i], has_ur, u, v, xr, V.radius);
      }
      unsigned long long m = __ballot(cand);
      any |= m != 0;
      while (m) {  // wave-uniform: ascending keypoint index
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const int ki = c + j;
        const double* q = P.feat + RSPL_FEATURE_ROWS * (size_t)ki + 3 + 4 * lane;  // 8-byte aligned only
        const double dot = wave::xsum64(partial4(d01.x, d01.y, d23.x, d23.y, q[0], q[1], q[2], q[3]));
        b.visit(distance_of(dot), __builtin_amdgcn_readlane(key, j), ki);
      }
    }
    status = !any ? RSPL_LMAP_NO_CANDIDATE : (b.idx >= 0 && b.good(V) ? RSPL_LMAP_GOOD : RSPL_LMAP_FAILED);
  }
  if (lane == 0) {
    a.status[op] = status;
    a.best_idx[op] = b.idx;
    a.best[op] = b.best;
    a.second[op] = b.second;
  }
}

__global__ __launch_bounds__(T) void lmap_merge_kernel(Args a, int n_local) {
  extern __shared__ int claim[];  // [K] largest local index among the good projections onto the keypoint, -1: none
  __shared__ int wtot[NW];
  const int f = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const Param& P = a.params[f];
  const int K = a.K, n1 = a.n1c[f];
  const size_t ok = (size_t)f * K, ol = (size_t)f * a.L;
  for (int j = tid; j < K; j += T) claim[j] = -1;

  // The good projections in local order (SearchByProjection's emplace_back order), the claims, the counts.  Wave w
  // owns the w-th contiguous quarter of the local map: a counting pass, one barrier for the quarters' totals, a
  // placement pass.
  const int span = (n_local + NW * 64 - 1) / (NW * 64) * 64;
  const int w0 = wv * span < n_local ? wv * span : n_local;
  const int w1 = w0 + span < n_local ? w0 + span : n_local;
  int nsel = 0, nproj = 0, ncand = 0, mine = 0;
  for (int c = w0; c < w1; c += 64) {
    const int p = c + lane;
    const int st = p < w1 ? a.status[ol + p] : RSPL_LMAP_NOT_SELECTED;
    nsel += st != RSPL_LMAP_NOT_SELECTED;
    nproj += st >= RSPL_LMAP_NO_CANDIDATE;
    ncand += st >= RSPL_LMAP_FAILED;
    mine += __popcll(__ballot(st == RSPL_LMAP_GOOD));
  }
  if (lane == 0) wtot[wv] = mine;
  __syncthreads();
  int base = 0, n_good = 0;
#pragma unroll
  for (int w = 0; w < NW; w++) {
    if (w < wv) base += wtot[w];
    n_good += wtot[w];
  }
  for (int c = w0; c < w1; c += 64) {
    const int p = c + lane;
    const bool good = p < w1 && a.status[ol + p] == RSPL_LMAP_GOOD;
    const unsigned long long m = __ballot(good);
    if (good) {
      const int kp = a.best_idx[ol + p], s = base + wave::lanes_below(m);
      a.good_kp[ol + s] = kp;
      a.good_point[ol + s] = p;
      atomicMax(claim + kp, p);  // kp < n1 <= K: the search only proposes keypoints it visited
    }
    base += __popcll(m);
  }
  nsel = wave::block_sum_int<NW>(nsel);
  nproj = wave::block_sum_int<NW>(nproj);
  ncand = wave::block_sum_int<NW>(ncand);  // (its barriers also order the claims before the reads below)

  // the merged table: the frame's own point, else the last good projection onto the keypoint
  for (int j = tid; j < K; j += T) {
    int id = -1, self = -1;
    uint8_t state = RSPL_TRACK_NO_MAPPOINT;
    double x = 0, y = 0, z = 0;
    if (j < n1) {
      const int own = P.pid[j];
      const int c = claim[j];
      if (own >= 0) {
        id = own;
        state = (!P.pgood || P.pgood[j]) ? RSPL_TRACK_GOOD : RSPL_TRACK_NOT_GOOD;
        x = P.pxyz[3 * (size_t)j]; y = P.pxyz[3 * (size_t)j + 1]; z = P.pxyz[3 * (size_t)j + 2];
      } else if (c >= 0) {
        id = a.local_id[c];
        state = RSPL_TRACK_GOOD;
        x = a.local_pos[3 * (size_t)c]; y = a.local_pos[3 * (size_t)c + 1]; z = a.local_pos[3 * (size_t)c + 2];
      }
      if (state != RSPL_TRACK_NO_MAPPOINT) self = j;
    }
    if (P.kf_points) {
      double* X = P.kf_points + 3 * (size_t)j;
      X[0] = x; X[1] = y; X[2] = z;
      P.kf_state[j] = state;
      P.kf_tid[j] = id;
    }
    a.idx0[ok + j] = self;
    a.idx1[ok + j] = self;
    a.assoc[ok + j] = id;
  }
  // the results go to host-mapped memory last, in bulk
  __syncthreads();
#pragma unroll 4
  for (int i = tid; i < n_good; i += T) {
    a.o_good_kp[ol + i] = a.good_kp[ol + i];
    a.o_good_point[ol + i] = a.good_point[ol + i];
  }
#pragma unroll 4
  for (int j = tid; j < K; j += T) a.o_assoc[ok + j] = a.assoc[ok + j];
  if (tid == 0) {
    Out* r = a.out + f;
    r->n1 = n1;
    r->n_selected = nsel;
    r->n_projected = nproj;
    r->n_cand = ncand;
    r->n_good = n_good;
    r->pad[0] = r->pad[1] = r->pad[2] = 0;
  }
}

}  // namespace

hipError_t store(double* bank, const double* feat, const int32_t* pairs, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  lmap_store_kernel<<<n, 64, 0, s>>>(bank, feat, pairs);
  return hipGetLastError();
}

hipError_t search(const Args& a, int batch, int n_local, hipStream_t s) {
  lmap_prep_kernel<<<dim3((a.K + T - 1) / T, batch), T, 0, s>>>(a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (n_local > 0) {
    lmap_search_kernel<<<dim3((n_local + NW - 1) / NW, batch), T, 0, s>>>(a, n_local);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  lmap_merge_kernel<<<batch, T, sizeof(int) * a.K, s>>>(a, n_local);
  return hipGetLastError();
}

}  // namespace lmap
}  // namespace rspl
