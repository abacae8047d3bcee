#pragma once
// The line detector's per-pixel and per-chain arithmetic: FastLineDetector after Canny's classes, restating
// oracle/fld_ref.py.  This header is the text: the device kernels (fld_kernels.hip) and the host detector
// (fld_host.hpp, behind rspl_lines_detect and the two rspl_lines_debug_fld_* hooks) both compile it, and no rule
// below is written anywhere else under csrc.  It holds getPointChain's step, the line through two points,
// cv::fitLine DIST_L2 from running sums, extractSegments, the float cast with the length and border filters, and
// the brighter-side-left orientation.  Double / float types and operation order are the restatement's, with FP
// contraction off in every function, so both sides equal it bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace rspl {
namespace fld {

constexpr int kMaxBatch = 2;          // images per rspl_lines_detect_device call
constexpr int kMaxEdge = 32768;       // edge pixels per image: the component sort packs (label, index) as 15 + 15 bits
constexpr int kMaxSeg = kMaxEdge / 2; // runs are disjoint and hold >= 2 points each
constexpr int kMaskLdsBytes = 147456; // both half-image bitmasks (strong and candidate) in LDS: rows * ceil(w / 32) * 8
constexpr int kMetaInts = 16;         // per image: see Meta
enum Meta { kNEdge = 0, kNComp, kNChain, kNSeg, kPasses, kMaxComp, kWalkIters, kStatus };
enum Status { kStEdgePixels = 1, kStSegments = 2, kStLogic = 4 };

__host__ __device__ inline int words_per_row(int hw) { return (hw + 31) >> 5; }
__host__ __device__ inline uint32_t pack_pt(int x, int y) { return (uint32_t)x | ((uint32_t)y << 16); }
__host__ __device__ inline int pt_x(uint32_t p) { return (int)(p & 0xffffu); }
__host__ __device__ inline int pt_y(uint32_t p) { return (int)(p >> 16); }

// one bit per half-image pixel, rows padded to whole 32-bit words
struct BitView {
  const volatile uint32_t* w;
  int wpr;
  __host__ __device__ bool operator()(int x, int y) const { return (w[y * wpr + (x >> 5)] >> (x & 31)) & 1u; }
};

// getPointChain: the neighbours in index order (dr, dc) = (1,1) (1,0) (1,-1) (0,-1) (-1,-1) (-1,0) (-1,1) (0,1);
// step 0 takes the first edge neighbour, later steps the most direction-consistent one (ties to the later
// index) if within 2.  `edge(x, y)` tests a pixel.
__host__ __device__ inline int nb_dr(int i) { return (int)((0x406Au >> (2 * i)) & 3u) - 1; }
__host__ __device__ inline int nb_dc(int i) { return (int)((0xA406u >> (2 * i)) & 3u) - 1; }
__host__ __device__ inline int nb_dir(int i) { return i > 4 ? i - 8 : i; }

// bit i: neighbour i is inside the image and an edge.  No branch between the eight tests (an outside neighbour
// reads the pixel itself and is masked), so that on the device the reads are in flight together.
template <class Edge>
__host__ __device__ inline unsigned neighbour_mask(const Edge& edge, int h, int w, int x, int y) {
  unsigned nb = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int ci = x + nb_dc(i), ri = y + nb_dr(i);
    const bool in = !(ri < 0 || ri == h || ci < 0 || ci == w);
    const bool set = edge(in ? ci : x, in ? ri : y);
    nb |= (unsigned)(in & set) << i;
  }
  return nb;
}

// the direction-consistency rule of the later steps: the edge neighbours are offered in index order, the
// difference to the chain's direction wraps at 4, `<=` gives a tie to the later index, and the winner is taken
// if it is within 2
struct Pick {
  float best = 7.0f;
  int i = -1;
  __host__ __device__ void offer(int k, int direction) {
#pragma clang fp contract(off)
    float diff = fabsf((float)nb_dir(k) - (float)direction);
    diff = diff > 4.0f ? 8.0f - diff : diff;
    if (diff <= best) {
      best = diff;
      i = k;
    }
  }
  __host__ __device__ void first(int k) {  // step 0: the first edge neighbour, whatever its direction
    best = 0.0f;
    i = k;
  }
  __host__ __device__ int taken() const { return i >= 0 && best < 2.0f ? i : -1; }
};

// the neighbour getPointChain takes for a mask, or -1: a function of (mask, direction, step == 0) alone, which
// the walk kernel tabulates in LDS once per launch
__host__ __device__ inline int chain_pick(unsigned nb, int direction, int step) {
  Pick p;
  for (int i = 0; i < 8; i++) {
    if (!((nb >> i) & 1u)) continue;
    if (step == 0) return i;  // Pick::first, spelt out: the kernels' code stays what it was
    p.offer(i, direction);
  }
  return p.taken();
}

// one step of a sequential walk (the host detector): tests and rule fused in one loop, which skips a neighbour
// outside the image or not an edge and leaves at the first one at step 0.  Always inlined: it runs once per edge
// pixel, and as a call from the walk's loop it costs the host detector 5 to 10 % (measured: DESIGN.md).
template <class Edge>
__host__ __device__ inline __attribute__((always_inline)) bool chain_step(const Edge& edge, int h, int w, int& x,
                                                                          int& y, int& direction, int step) {
  Pick p;
  for (int k = 0; k < 8; k++) {
    const int ci = x + nb_dc(k), ri = y + nb_dr(k);
    if (ri < 0 || ri == h || ci < 0 || ci == w || !edge(ci, ri)) continue;
    if (step == 0) {
      p.first(k);
      break;
    }
    p.offer(k, direction);
  }
  const int i = p.taken();
  if (i < 0) return false;
  x += nb_dc(i);
  y += nb_dr(i);
  direction = nb_dir(i);
  return true;
}

struct HLine {
  double a, b, c;
};

__host__ __device__ inline HLine line_through(double px, double py, double qx, double qy) {
#pragma clang fp contract(off)
  const double a = py - qy, b = qx - px, c = px * qy - py * qx;
  const double n = sqrt(a * a + b * b);
  return {a / n, b / n, c / n};
}

// fit_line's five sums over a run that only grows at its end: exact integers in fp64, so adding a point to the
// running sums gives what the restatement's recomputation over the whole run gives
struct Sums {
  double sx, sy, sxx, syy, sxy;
  int n;
  __host__ __device__ void clear() {
    sx = sy = sxx = syy = sxy = 0.0;
    n = 0;
  }
  __host__ __device__ void add(uint32_t p) {
#pragma clang fp contract(off)
    const int x = pt_x(p), y = pt_y(p);
    sx += (double)x;
    sy += (double)y;
    sxx += (double)((long long)x * x);
    syy += (double)((long long)y * y);
    sxy += (double)((long long)x * y);
    n++;
  }
};

__host__ __device__ inline HLine fit_line(const Sums& s) {
#pragma clang fp contract(off)
  const double cnt = (double)s.n, cx = s.sx / cnt, cy = s.sy / cnt;
  const double dxx = s.sxx / cnt - cx * cx, dyy = s.syy / cnt - cy * cy, dxy = s.sxy / cnt - cx * cy;
  const double t = atan2(2.0 * dxy, dxx - dyy) / 2.0;
  const double vx = cos(t), vy = sin(t);
  return line_through(cx, cy, cx + vx, cy + vy);
}

__host__ __device__ inline double ldist(const HLine& l, double x, double y) {
#pragma clang fp contract(off)
  return fabs(l.a * x + l.b * y + l.c);
}

// extractSegments over one chain's points: emit(k, x1, y1, x2, y2) per straight run, k counting the runs
template <class Emit>
__host__ __device__ inline void extract_segments(const uint32_t* pts, int total, int len_thr, double dist_thr,
                                                 Emit&& emit) {
#pragma clang fp contract(off)
  int i = 0, k = 0;
  while (i + len_thr < total) {
    const uint32_t ps = pts[i], pe = pts[i + len_thr];
    HLine l = line_through(pt_x(ps), pt_y(ps), pt_x(pe), pt_y(pe));
    bool is_line = true;
    for (int j = 1; j < len_thr && is_line; j++) is_line = ldist(l, pt_x(pts[i + j]), pt_y(pts[i + j])) <= dist_thr;
    if (!is_line) {
      i++;
      continue;
    }
    Sums s;
    s.clear();
    for (int j = 0; j <= len_thr; j++) s.add(pts[i + j]);
    l = fit_line(s);
    int j = i + len_thr + 1;
    for (; j < total; j++) {
      const double x = pt_x(pts[j]), y = pt_y(pts[j]);
      if (ldist(l, x, y) > dist_thr) {
        l = fit_line(s);
        if (ldist(l, x, y) > dist_thr) break;
      }
      s.add(pts[j]);
    }
    l = fit_line(s);
    const uint32_t pf = pts[i], pb = pts[j - 1];
    const double df = l.a * pt_x(pf) + l.b * pt_y(pf) + l.c, db = l.a * pt_x(pb) + l.b * pt_y(pb) + l.c;
    emit(k, pt_x(pf) - df * l.a, pt_y(pf) - df * l.b, pt_x(pb) - db * l.a, pt_y(pb) - db * l.b);
    k++;
    i = j;  // the rejected point (or the end) starts the next search
  }
}

// the float cast, the float length filter, the border filter and the orientation (brighter side on the left:
// the intensity difference at +-1.5 px along the normal, one sample per pixel of length); false = dropped
__host__ __device__ inline bool finish_segment(const uint8_t* img, int h, int w, int len_thr, double sx1, double sy1,
                                               double sx2, double sy2, float* out) {
#pragma clang fp contract(off)
  const float fx1 = (float)sx1, fy1 = (float)sy1, fx2 = (float)sx2, fy2 = (float)sy2;
  const float ddx = fx1 - fx2, ddy = fy1 - fy2;
  const float length = sqrtf(ddx * ddx + ddy * ddy);
  if (length < (float)len_thr) return false;
  if ((fx1 <= 5.0f && fx2 <= 5.0f) || (fy1 <= 5.0f && fy2 <= 5.0f) || (fx1 >= w - 5.0f && fx2 >= w - 5.0f) ||
      (fy1 >= h - 5.0f && fy2 >= h - 5.0f))
    return false;
  const double x1 = fx1, y1 = fy1, x2 = fx2, y2 = fy2;
  const double dx = x2 - x1, dy = y2 - y1;
  const double L = sqrt(dx * dx + dy * dy);
  const double nx = -dy / L, ny = dx / L;
  const int n = (int)L > 1 ? (int)L : 1;
  long long acc = 0;
  for (int k = 0; k < n; k++) {
    const double t = (k + 0.5) / n;
    const double px = x1 + t * dx, py = y1 + t * dy;
    const int lx = (int)floor(px + 1.5 * nx + 0.5), ly = (int)floor(py + 1.5 * ny + 0.5);
    const int rx = (int)floor(px - 1.5 * nx + 0.5), ry = (int)floor(py - 1.5 * ny + 0.5);
    if (lx >= 0 && lx < w && ly >= 0 && ly < h && rx >= 0 && rx < w && ry >= 0 && ry < h)
      acc += (int)img[(size_t)ly * w + lx] - (int)img[(size_t)ry * w + rx];
  }
  if (acc < 0) {
    out[0] = fx2; out[1] = fy2; out[2] = fx1; out[3] = fy1;
  } else {
    out[0] = fx1; out[1] = fy1; out[2] = fx2; out[3] = fy2;
  }
  return true;
}

}  // namespace fld
}  // namespace rspl
