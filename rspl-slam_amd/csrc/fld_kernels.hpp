#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fld_device.hpp"

namespace rspl {
namespace fld {

// The detector after Canny's classes as five stream-ordered launches, one workgroup per image (grid = batch):
//   hysteresis  cls -> edge bitmask (strong pixels through 8-connected candidates, then the corner zeroing)
//   labels      edge pixels listed in raster order, 8-connected components by union-find, each component's pixels
//               made contiguous (raster order kept) by a bitonic sort of (label, index) keys in LDS
//   walk        one lane per component: raster-order seeds, getPointChain steps, bits cleared by LDS atomics
//   fit         one lane per chain: extractSegments, filters, orientation -> (seed, k) keyed segment records
//   order       segments ranked by (seed, k): the sequential detector's order; count + first `capacity` out
// Image b's scratch is at b * (its per-image size); every cap ends in a Status bit of meta[b][kStatus].
struct Args {
  int hh, hw;             // half image
  const uint8_t* half;    // [B][hh * hw]
  const uint8_t* cls;     // [B][hh * hw] 2 strong, 0 candidate, 1 none
  uint32_t* ebits;        // [B][hh * words_per_row(hw)]
  int* pix;               // [B][kMaxEdge] pixel index of each edge pixel, raster order
  int* lab;               // [B][kMaxEdge] component label (its first pixel's list index)
  int* spix;              // [B][kMaxEdge] the pixels grouped by component, as packed points (pack_pt)
  int* cstart;            // [B][kMaxEdge + 1] first position of each component in spix
  uint32_t* pts;          // [B][kMaxEdge] chain points, component c's in [cstart[c], cstart[c + 1])
  int* chains;            // [B][kMaxEdge][3] seed pixel index, offset into pts, length
  unsigned long long* skey;  // [B][kMaxSeg] seed << 32 | k
  float* sseg;            // [B][kMaxSeg][4]
  int* meta;              // [B][kMetaInts]
  int len_thr;
  double dist_thr;
  float* out;             // [B][capacity][4]
  int capacity;
  int32_t* counts;        // [B]
};

bool mask_fits(int hh, int hw);  // both bitmasks within kMaskLdsBytes
hipError_t hysteresis(const Args& a, int B, hipStream_t s);
hipError_t labels(const Args& a, int B, hipStream_t s);
hipError_t walk(const Args& a, int B, hipStream_t s);
hipError_t fit(const Args& a, int B, hipStream_t s);
hipError_t order(const Args& a, int B, hipStream_t s);

}  // namespace fld
}  // namespace rspl
