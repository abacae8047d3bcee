// Stereo rectification on the device (rect_kernels.hip): cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on u8
// through a fixed-point table built once per camera (rect.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rspl {
namespace rect {

constexpr int kPixPerLane = 4;            // horizontally adjacent output pixels of one lane
constexpr int kTileW = 64 * kPixPerLane;  // a wave covers one 256-pixel row segment
constexpr int kTileH = 4;                 // rows (waves) per workgroup
constexpr int kMaxDim = 2044;             // ix + 2 and iy + 2 (-2 .. dim) in 11 bits each
constexpr int kMaxBatch = 1024;

// One table entry per output pixel: [0,11) ix + 2, [11,22) iy + 2, [22,27) fx, [27,32) fy.
inline uint32_t pack(int ix, int iy, int fx, int fy) {
  return (uint32_t)(ix + 2) | (uint32_t)(iy + 2) << 11 | (uint32_t)fx << 22 | (uint32_t)fy << 27;
}
// table row pitch in entries: rows start 16-byte aligned; the padding entries are 0 (outside)
inline size_t table_pitch(int W) { return ((size_t)W + kPixPerLane - 1) / kPixPerLane * kPixPerLane; }

struct Args {
  const uint32_t* table;  // [2][H][tpitch]
  size_t cam_pitch;       // entries per camera
  uint32_t tpitch;
  const uint8_t* src;
  uint32_t src_stride;  // H * src_stride < 2^31: offsets inside an image are 32-bit
  size_t src_pitch;
  uint8_t* dst;
  uint32_t dst_stride;  // H * dst_stride < 2^31 likewise
  size_t dst_pitch;
  int H, W, batch;
  int dst_aligned;                    // dst, dst_stride and dst_pitch are multiples of 4: rows take 4-byte stores
  uint32_t cam_bits[kMaxBatch / 32];  // bit b: the camera of image b
};

hipError_t remap(const Args& a, hipStream_t s);

}  // namespace rect
}  // namespace rspl
