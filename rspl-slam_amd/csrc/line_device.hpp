// Device pieces shared by the line kernels (line_kernels.hip: AssignPointsToLines / MatchLines per image)
// and the tracking step's line kernel (track_line_kernels.hip): the on-line test of
// line_processor.cc:201-212, the workgroup scan behind the CSR offsets and the first-maximum wave argmax
// of MatchLines (:265-270).  One source, so both units decide "is this keypoint on this line" with the
// same arithmetic: doubles, the distance through a float, contraction off so every product is rounded
// as the reference's non-FMA x86 build rounds it.
#pragma once
#include <hip/hip_runtime.h>

namespace rspl {
namespace lines {

// wave-wide exclusive prefix of a per-lane count
__device__ __forceinline__ int wave_excl(int v, int lane) {
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  return x - v;
}

// exclusive scan of data[0..n) in LDS by a 1024-thread workgroup (n <= 4 * 1024 per pass, then
// carried); returns the total.  `part` is 16 ints of LDS.
__device__ inline int block_excl_scan(int* data, int n, int* part) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += 4096) {
    int v[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = base + 4 * tid + q;
      v[q] = i < n ? data[i] : 0;
      s += v[q];
    }
    const int ex = wave_excl(s, lane);
    if (lane == 63) part[wv] = ex + s;
    __syncthreads();
    int wbase = carry;
    for (int w = 0; w < wv; w++) wbase += part[w];
    int run = wbase + ex;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = base + 4 * tid + q;
      if (i < n) data[i] = run;
      run += v[q];
    }
    int tot = 0;
    for (int w = 0; w < 16; w++) tot += part[w];
    __syncthreads();
    carry += tot;
  }
  return carry;
}

struct LineEq {
  double x1, y1, x2, y2, A, B, C, D, lox, hix, loy, hiy;
};

__device__ __forceinline__ LineEq line_eq(const double* l) {
#pragma clang fp contract(off)
  LineEq q;
  q.x1 = l[0];
  q.y1 = l[1];
  q.x2 = l[2];
  q.y2 = l[3];
  q.A = q.y2 - q.y1;
  q.B = q.x1 - q.x2;
  q.C = q.x2 * q.y1 - q.x1 * q.y2;
  q.D = sqrt(q.A * q.A + q.B * q.B);
  q.lox = q.x1 > q.x2 ? q.x2 : q.x1;
  q.hix = q.x1 > q.x2 ? q.x1 : q.x2;
  q.loy = q.y1 > q.y2 ? q.y2 : q.y1;
  q.hiy = q.y1 > q.y2 ? q.y1 : q.y2;
  return q;
}

// line_processor.cc:201-212: inside the 3-px-padded box, <= 6 px from the infinite line, and
// within 3 px of an endpoint or projecting between the endpoints
__device__ __forceinline__ bool on_line(const LineEq& q, double px, double py, float& d) {
#pragma clang fp contract(off)
  if (px < q.lox - 3 || px > q.hix + 3 || py < q.loy - 3 || py > q.hiy + 3) return false;
  d = (float)(fabs(q.A * px + q.B * py + q.C) / q.D);
  if (d > 6) return false;
  const double s1 = (q.x1 - px) * (q.x1 - px) + (q.y1 - py) * (q.y1 - py);
  const double s2 = (q.x2 - px) * (q.x2 - px) + (q.y2 - py) * (q.y2 - py);
  const double ls = q.D * q.D;
  return s1 <= 9 || s2 <= 9 || ((s1 < ls + s2) && (s2 < ls + s1));
}

// AssignPointsToLines (line_processor.cc:163-216) for one image by one 1024-thread workgroup: line l's
// keypoints (x at pts[j * stride], y right after it, j < np) compacted in keypoint order -- a wave per
// line, 64 keypoints per ballot -- into the CSR offs[nl + 1] / idx / dist.  cnt: nl + 1 ints of LDS that
// hold the offsets afterwards, part: 16.  Returns the pair count; past `cap` only the offsets are written.
// Ends on a barrier.
__device__ inline int assign_lines(const double* L, int nl, const double* pts, int stride, int np, int* offs,
                                   int* idx, double* dist, int cap, int* cnt, int* part) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // pass 1: pairs per line
  for (int l = wv; l < nl; l += 16) {
    const LineEq q = line_eq(L + 4 * l);
    int c = 0;
    for (int j0 = 0; j0 < np; j0 += 64) {
      const int j = j0 + lane;
      float d;
      const bool in = j < np && on_line(q, pts[(size_t)j * stride], pts[(size_t)j * stride + 1], d);
      c += __popcll(__ballot(in));
    }
    if (lane == 0) cnt[l] = c;
  }
  __syncthreads();
  const int tot = block_excl_scan(cnt, nl, part);
  for (int l = tid; l < nl; l += 1024) offs[l] = cnt[l];
  if (tid == 0) offs[nl] = cnt[nl] = tot;  // (cnt = the offsets, for a caller that goes on in the same launch)
  if (tot <= cap) {  // uniform
    // pass 2: the same tests, written compacted in keypoint order
    const unsigned long long below = (1ull << lane) - 1;
    for (int l = wv; l < nl; l += 16) {
      const LineEq q = line_eq(L + 4 * l);
      int base = cnt[l];
      for (int j0 = 0; j0 < np; j0 += 64) {
        const int j = j0 + lane;
        float d = 0.f;
        const bool in = j < np && on_line(q, pts[(size_t)j * stride], pts[(size_t)j * stride + 1], d);
        const unsigned long long m = __ballot(in);
        if (in) {
          const int pos = base + __popcll(m & below);
          idx[pos] = j;
          dist[pos] = (double)d;
        }
        base += __popcll(m);
      }
    }
  }
  __syncthreads();
  return tot;
}

// the first maximum across a wave: every lane holds a candidate (value, index), `best` = -1 for none;
// afterwards every lane holds the largest value and, among equals, the smallest index (Eigen's
// maxCoeff(&index) order)
__device__ __forceinline__ void wave_first_max(int& best, int& bi) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int ov = __shfl_xor(best, o), oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
}

}  // namespace lines
}  // namespace rspl
