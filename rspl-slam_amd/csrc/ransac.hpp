// cv::RANSACPointSetRegistrator as the PnP (5 points) and F-matrix (7 points) stages restate it, once: cv::RNG's
// generator, getSubset's draw of M distinct indices, RANSACUpdateNumIters, and the mutual match check both
// stages start from.  ONE source for the host and the device (and for a plain host compiler: tests/c), so the
// host samplers, the handles' draw-table sizing and the gather kernels' walk over the draw table cannot drift.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RSPL_RANSAC_HD __host__ __device__ __forceinline__
#else
#define RSPL_RANSAC_HD inline
#endif

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

namespace rspl {
namespace ransac {

// cv::RNG::next (multiply-with-carry), the generator RANSACPointSetRegistrator::run seeds with (uint64)-1
RSPL_RANSAC_HD unsigned rng_next(uint64_t& s) {
  s = (uint64_t)(unsigned)s * 4164903690u + (unsigned)(s >> 32);
  return (unsigned)s;
}

// getSubset's inner loop over the live generator: M distinct values of [0, count), a duplicate draws again.
// False (nothing drawn) when count < M.
template <int M>
RSPL_RANSAC_HD bool draw_subset(uint64_t& s, int count, int32_t* o) {
  if (count < M) return false;
  for (int i = 0; i < M; i++) {
    int v;
    for (;;) {
      v = (int)(rng_next(s) % (unsigned)count);
      bool dup = false;
      for (int j = 0; j < i; j++) dup |= o[j] == v;
      if (!dup) break;
    }
    o[i] = v;
  }
  return true;
}

// getSubset started at draw k of the (already reduced % count) stream dv[0, nd): M distinct values, a
// duplicate draws again.  Returns the draws consumed, 0 when the table ends first.
template <int M, class D>
RSPL_RANSAC_HD int subset_at(const D* dv, int nd, int k, int (&o)[M]) {
  int pos = k;
#pragma unroll
  for (int i = 0; i < M; i++) o[i] = -1;
#pragma unroll
  for (int i = 0; i < M; i++) {
    for (;;) {
      if (pos >= nd) return 0;
      const int v = dv[pos++];
      bool dup = false;
#pragma unroll
      for (int j = 0; j < M; j++) dup |= j < i && o[j] == v;
      if (!dup) {
        o[i] = v;
        break;
      }
    }
  }
  return pos - k;
}

// RANSACUpdateNumIters.  E is the type the exponent reaches pow() with: solvePnPRansac's restatement passes an
// int, findFundamentalMat's a double, and on the device those are different math routines -- each caller keeps
// the one its results were pinned with.
template <class E>
RSPL_RANSAC_HD int update_num_iters(double p, double ep, E model_points, int max_iters) {
#pragma clang fp contract(off)
  p = fmin(fmax(p, 0.), 1.);
  ep = fmin(fmax(ep, 0.), 1.);
  double num = fmax(1. - p, DBL_MIN);
  double denom = 1. - pow(1. - ep, model_points);
  if (denom < DBL_MIN) return 0;
  num = log(num);
  denom = log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

// The mutual check of point_matching.cc:24-31 from one side: keypoint i's partner on the other side
// (n_other keypoints), or -1.  fwd = this side's indices (i -> partner), back = the other side's.
RSPL_RANSAC_HD int mutual_partner(const int32_t* fwd, const int32_t* back, int i, int n_other) {
  const int j = fwd[i];
  return (j >= 0 && j < n_other && back[j] == i) ? j : -1;
}

// the first n raw draws of the generator, which do not depend on the correspondence count (host)
inline std::vector<uint32_t> raw_draws(int n) {
  std::vector<uint32_t> d(n);
  uint64_t s = (uint64_t)-1;
  for (uint32_t& v : d) v = rng_next(s);
  return d;
}

// The draws the first `want` subsets of M out of `count` consume, or -1 when the table d ends first; *fit =
// the subsets that do fit, *fit_draws their draws (either may be null).  Host; getSubset's own loop rather than
// subset_at over a reduced copy (a third of the time at create, which runs it for every count), and
// tests/c/ransac_check.cpp holds the two to each other.
template <int M>
inline int draws_needed(const std::vector<uint32_t>& d, int count, int want, int* fit = nullptr,
                        int* fit_draws = nullptr) {
  size_t pos = 0, done = 0;  // done: the draws of the subsets that fit
  int h = 0, o[M];
  for (; h < want; h++) {
    for (int i = 0; i < M; i++) {
      for (;;) {
        if (pos >= d.size()) goto out;
        const int v = (int)(d[pos++] % (unsigned)count);
        bool dup = false;
        for (int j = 0; j < i; j++) dup |= o[j] == v;
        if (!dup) {
          o[i] = v;
          break;
        }
      }
    }
    done = pos;
  }
out:
  if (fit) *fit = h;
  if (fit_draws) *fit_draws = (int)done;
  return h == want ? (int)done : -1;
}

}  // namespace ransac
}  // namespace rspl
