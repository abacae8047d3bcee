// cv::findFundamentalMat(points0, points1, FM_RANSAC, 3, 0.99, mask) (src/point_matching.cc:34-45) for a batch
// of independent frames, as one stream-ordered chain with no host work in between:
//   fm_gather_kernel  (device-resident path) SuperGlue's indices -> the mutual matches in DMatch order, their
//                     float-rounded pixel pairs, RANSAC's subsets from the handle's table of raw draws
//   fm_hyp_kernel     a lane per RANSAC iteration: the 7-point solver (fm_solve.hpp), up to three models
//   fm_count_kernel   a wave per iteration: each model's inlier count over all n correspondences by ballots
//   fm_accept_kernel  the sequential acceptance replayed over the stored counts (RANSACUpdateNumIters
//                     included), the winning model's mask, and on the device-resident path the filtered
//                     copies of SuperGlue's indices (the write-back)
// All iterations the handle allows are solved side by side; the acceptance decides afterwards how many the
// sequential loop would have evaluated, so the result is the sequential one for every n.
#include "fm_kernels.hpp"
#include "fm_solve.hpp"
#include "ransac.hpp"
#include "wave_reduce.hpp"

namespace rspl {
namespace fm {
namespace {

constexpr int T = 256, NW = 4;
constexpr int kCountWaves = 4;  // iterations (one wave each) per workgroup of fm_count_kernel

using ransac::subset_at;
using wave::lanes_below;

__device__ __forceinline__ void load_subset_points(const double* p, const int (&o)[7], double (&s)[14]) {
#pragma unroll
  for (int i = 0; i < 7; i++) {
    const double2 v = *reinterpret_cast<const double2*>(p + 2 * (size_t)o[i]);
    s[2 * i] = v.x;
    s[2 * i + 1] = v.y;
  }
}

__global__ __launch_bounds__(T) void fm_gather_kernel(Args a) {
  __shared__ int wtot[NW];
  __shared__ unsigned short dv[kDrawCap];     // draws % count
  __shared__ unsigned short run[kDrawCap];    // draws a subset started at k consumes | 0x8000: it passes checkSubset
  __shared__ unsigned short start[kMaxIters]; // where iteration h's accepted subset starts
  __shared__ int found_s;
  const int f = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const Param P = a.host_params[f];
  if (tid == 0) a.params[f] = P;
  const int K = a.K;
  const size_t o = (size_t)f * K;
  int n0 = *P.n0, n1 = *P.n1;
  n0 = n0 < 0 ? 0 : (n0 > K ? K : n0);
  n1 = n1 < 0 ? 0 : (n1 > K ? K : n1);
  double* q0 = a.p0 + 2 * o;
  double* q1 = a.p1 + 2 * o;

  // the mutual matches (point_matching.cc:24-31) in ascending i: slot = matches before i, by ballots
  int base = 0;
  for (int c = 0; c < n0; c += T) {
    const int i = c + tid;
    const int j = i < n0 ? ransac::mutual_partner(P.idx0, P.idx1, i, n1) : -1;
    const unsigned long long mk = __ballot(j >= 0);
    if (lane == 0) wtot[wv] = __popcll(mk);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const int k = wtot[w];
      if (w < wv) before += k;
      total += k;
    }
    if (j >= 0) {
      const int s = base + before + lanes_below(mk);  // < min(n0, n1) <= K: a keypoint has one mutual partner
      const double* r0 = P.feat0 + 259 * (size_t)i;
      const double* r1 = P.feat1 + 259 * (size_t)j;
      *reinterpret_cast<double2*>(q0 + 2 * s) = make_double2((double)(float)r0[1], (double)(float)r0[2]);  // cv::Point2f
      *reinterpret_cast<double2*>(q1 + 2 * s) = make_double2((double)(float)r1[1], (double)(float)r1[2]);
      a.match0[o + s] = i;
      a.match1[o + s] = j;
    }
    base += total;
    __syncthreads();  // wtot is rewritten by the next chunk
  }
  const int count = base;
  if (count <= kModelPoints) {  // no RANSAC: nothing (n < 7) or the direct solve of subset 0 .. 6 (n == 7)
    if (tid < kModelPoints) a.subsets[(size_t)f * kMaxIters * 7 + tid] = tid;
    if (tid == 0) {
      Desc d;
      d.n = count;
      d.iters = count == kModelPoints ? 1 : 0;
      d.thr = (float)(P.threshold * P.threshold);
      d.pad = 0;
      d.confidence = P.confidence;
      a.frames[f] = d;
    }
    return;  // uniform
  }

  // RANSAC's subsets for `count`.  The raw draws do not depend on the count; which draw a subset starts at
  // does (a duplicate draws again, a subset failing checkSubset is drawn again as a whole).  run[k] = the draws
  // a subset started at k would consume and whether it passes, for every k side by side; the starts are then
  // one chain of LDS look-ups in which a failed subset simply leads to the next start.
  int nd = a.need[count];
  nd = nd < a.n_draws ? nd : a.n_draws;
  nd = nd < kDrawCap ? nd : kDrawCap;
  for (int k = tid; k < nd; k += T) dv[k] = (unsigned short)(a.draws[k] % (unsigned)count);
  __syncthreads();  // (also orders the point pairs written above before the reads below)
  for (int k = tid; k < nd; k += T) {
    int v[7];
    int r = subset_at(dv, nd, k, v);
    if (r) {
      double s0[14], s1[14];
      load_subset_points(q0, v, s0);
      load_subset_points(q1, v, s1);
      if (check_subset(s0, s1)) r |= 0x8000;
    }
    run[k] = (unsigned short)r;
  }
  __syncthreads();
  if (tid == 0) {
    int pos = 0, found = 0;
    while (found < a.max_iters && pos < nd) {
      const int r = run[pos];
      if (r == 0) break;  // the table ends inside this subset: the sequence of subsets ends here
      if (r & 0x8000) start[found++] = (unsigned short)pos;
      pos += r & 0x7fff;
    }
    found_s = found;
    Desc d;
    d.n = count;
    d.iters = found;
    d.thr = (float)(P.threshold * P.threshold);
    d.pad = 0;
    d.confidence = P.confidence;
    a.frames[f] = d;
  }
  __syncthreads();
  const int found = found_s;
  for (int h = tid; h < found; h += T) {
    int v[7];
    subset_at(dv, nd, start[h], v);
    int32_t* dst = a.subsets + ((size_t)f * kMaxIters + h) * 7;
#pragma unroll
    for (int i = 0; i < 7; i++) dst[i] = v[i];
  }
}

// lane l of workgroup (bx, frame) solves iteration 64 bx + l
__global__ __launch_bounds__(64) void fm_hyp_kernel(Args a) {
  __shared__ double w[kWork * 64];
  const int f = blockIdx.y, lane = threadIdx.x;
  const int h = blockIdx.x * 64 + lane;
  const Desc D = a.frames[f];
  if (h >= D.iters) return;
  const size_t o = (size_t)f * a.K;
  const int32_t* sub = a.subsets + ((size_t)f * kMaxIters + h) * 7;
  int v[7];
#pragma unroll
  for (int i = 0; i < 7; i++) v[i] = sub[i];
  double s0[14], s1[14];
  load_subset_points(a.p0 + 2 * o, v, s0);
  load_subset_points(a.p1 + 2 * o, v, s1);
  const size_t hi = (size_t)f * kMaxIters + h;
  a.nmodels[hi] = seven_point<64>(s0, s1, w + lane, a.models + hi * 27);
}

// wave w of workgroup (bx, frame) counts the inliers of iteration 4 bx + w's models
__global__ __launch_bounds__(64 * kCountWaves) void fm_count_kernel(Args a) {
  const int f = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int h = blockIdx.x * kCountWaves + wv;
  const Desc D = a.frames[f];
  if (h >= D.iters) return;  // wave-uniform
  const size_t o = (size_t)f * a.K, hi = (size_t)f * kMaxIters + h;
  const double2* p0 = reinterpret_cast<const double2*>(a.p0 + 2 * o);
  const double2* p1 = reinterpret_cast<const double2*>(a.p1 + 2 * o);
  const int nm = a.nmodels[hi];
  for (int m = 0; m < nm; m++) {
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = a.models[hi * 27 + 9 * m + k];
    int cnt = 0;
    for (int c = 0; c < D.n; c += 64) {
      const int i = c + lane;
      bool in = false;
      if (i < D.n) {
        const double2 x0 = p0[i], x1 = p1[i];
        in = sampson_max(F, x0.x, x0.y, x1.x, x1.y) <= D.thr;
      }
      cnt += __popcll(__ballot(in));
    }
    if (lane == 0) a.counts[hi * 3 + m] = cnt;
  }
}

// one workgroup per frame: RANSAC's acceptance in iteration order (replayed by every thread, the counts read as
// broadcasts), the mask of the winning model, the filtered indices
__global__ __launch_bounds__(T) void fm_accept_kernel(Args a, int write_back) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const Desc D = a.frames[f];
  const int n = D.n;
  const size_t o = (size_t)f * a.K, h0 = (size_t)f * kMaxIters;
  int best = -1, best_m = 0, used = 0;
  if (n == kModelPoints) {  // the direct solve: its first model, every point kept
    used = 1;
    if (a.nmodels[h0] > 0) best = 0;
  } else if (n > kModelPoints) {
    int best_cnt = 0, niters = a.max_iters, h = 0;
    for (h = 0; h < niters; h++) {
      if (h >= D.iters) break;  // getSubset found no further subset
      const int nm = a.nmodels[h0 + h];
      for (int m = 0; m < nm; m++) {
        const int c = a.counts[(h0 + h) * 3 + m];
        if (c > (best_cnt > kModelPoints - 1 ? best_cnt : kModelPoints - 1)) {
          best = h;
          best_m = m;
          best_cnt = c;
          niters = ransac::update_num_iters(D.confidence, (double)(n - c) / n, (double)kModelPoints, niters);
        }
      }
    }
    used = h;
  }
  // (device-resident path) SuperGlue's indices are copied first; the mask loop below then sets both ends of
  // every rejected match to -1, everything else stays as it came
  Param P{};
  if (write_back) {
    P = a.params[f];
    int n0 = *P.n0, n1 = *P.n1;
    n0 = n0 < 0 ? 0 : n0;
    n1 = n1 < 0 ? 0 : n1;
    for (int i = tid; i < n0; i += T) P.idx0_out[i] = P.idx0[i];
    for (int j = tid; j < n1; j += T) P.idx1_out[j] = P.idx1[j];
    __syncthreads();  // the copies before the -1s
  }
  Out* out = a.out + f;
  uint8_t* inl = a.inl + o;
  int ninl = -1;
  if (best < 0 || n == kModelPoints) {  // no model (nothing rejected) or the direct solve
    for (int i = tid; i < n; i += T) inl[i] = 1;
    if (best >= 0) ninl = n;
  } else {
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = a.models[(h0 + best) * 27 + 9 * best_m + k];
    const double2* p0 = reinterpret_cast<const double2*>(a.p0 + 2 * o);
    const double2* p1 = reinterpret_cast<const double2*>(a.p1 + 2 * o);
    int c = 0;
    for (int i = tid; i < n; i += T) {
      const double2 x0 = p0[i], x1 = p1[i];
      const bool in = sampson_max(F, x0.x, x0.y, x1.x, x1.y) <= D.thr;
      inl[i] = in;
      c += in;
      if (write_back && !in) {
        P.idx0_out[a.match0[o + i]] = -1;
        P.idx1_out[a.match1[o + i]] = -1;
      }
    }
    ninl = wave::block_sum_int<NW>(c);
  }
  if (tid == 0) {
    for (int k = 0; k < 9; k++) out->F[k] = best >= 0 ? a.models[(h0 + best) * 27 + 9 * best_m + k] : 0.0;
    out->n = n;
    out->n_inliers = ninl;
    out->hyps = used;
    out->pad = 0;
  }
}

}  // namespace

hipError_t gather(const Args& a, int batch, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  fm_gather_kernel<<<batch, T, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t solve(const Args& a, int batch, bool write_back, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  fm_hyp_kernel<<<dim3((a.max_iters + 63) / 64, batch), 64, 0, s>>>(a);
  fm_count_kernel<<<dim3((a.max_iters + kCountWaves - 1) / kCountWaves, batch), 64 * kCountWaves, 0, s>>>(a);
  fm_accept_kernel<<<batch, T, 0, s>>>(a, write_back ? 1 : 0);
  return hipGetLastError();
}

}  // namespace fm
}  // namespace rspl
