#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rspl {
namespace fm {

constexpr int kMaxIters = 1000;      // RANSACPointSetRegistrator's maxIters as findFundamentalMat sets it
constexpr int kDrawCap = 14336;      // raw RNG draws the gather kernel can index (its two 28 KB LDS tables)
constexpr int kRedrawSlack = 256;    // subsets failing checkSubset the draw table allows per frame, where it fits
constexpr int kMinSlack = 32;        // ... and the least a handle is created with
constexpr int kMaxAttempts = 10000;  // getSubset's attempt limit per iteration (host path)
constexpr int kMaxMatches = 65535;   // a reduced draw is kept in 16 bits

struct Desc {       // one frame of the batch
  int n;            // correspondences, at [f * K, f * K + n)
  int iters;        // subsets available, at [f * kMaxIters, ...): n < 7: 0; n == 7: 1 (the direct solve)
  float thr;        // (float)(threshold * threshold)
  int pad;
  double confidence;
};

struct Param {  // one frame of a device-resident batch, written by the host into host-mapped memory
  const double* feat0;     // [cap][259]
  const double* feat1;
  const int32_t* n0;
  const int32_t* n1;
  const int32_t* idx0;
  const int32_t* idx1;
  int32_t* idx0_out;
  int32_t* idx1_out;
  double threshold, confidence;
};

struct Out {  // per-frame result (host-mapped)
  double F[9];
  int n, n_inliers, hyps, pad;
};

struct Args {
  int K;                   // per-frame capacity (max_matches)
  int max_iters;           // the handle's RANSAC iteration limit (<= kMaxIters)
  Desc* frames;            // [B]
  double* p0;              // [B][K][2] float-rounded like cv::Point2f
  double* p1;
  int32_t* subsets;        // [B][kMaxIters][7]
  double* models;          // [B][kMaxIters][3][9]
  int32_t* nmodels;        // [B][kMaxIters]
  int32_t* counts;         // [B][kMaxIters][3]
  uint8_t* inl;            // [B][K] host-mapped
  Out* out;                // [B] host-mapped
  // device-resident path
  const Param* host_params;  // host-mapped, read once by the gather kernel
  Param* params;             // its device copy
  const uint32_t* draws;     // [n_draws] raw multiply-with-carry draws
  const int32_t* need;       // [K + 1] draws the gather kernel tabulates at each count (see fm.cpp)
  int n_draws;
  int32_t* match0;           // [B][K] compacted match -> keypoint of image 0 / image 1
  int32_t* match1;
};

hipError_t gather(const Args& a, int batch, hipStream_t s);                 // device-resident path only
hipError_t solve(const Args& a, int batch, bool write_back, hipStream_t s);  // hypotheses | counts | acceptance

}  // namespace fm
}  // namespace rspl
