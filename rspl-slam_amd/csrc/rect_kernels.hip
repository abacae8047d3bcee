// rect_kernel: the rectifying remap of a batch of u8 images, both cameras, in one launch.
// A lane owns four horizontally adjacent output pixels: one 16-byte load of their table entries (4 B per
// pixel, constant across frames, so cache resident), sixteen source bytes as plain global loads (no LDS) --
// neighbouring lanes read neighbouring source bytes, the maps being smooth -- integer arithmetic only, and
// one 4-byte store, so a wave writes 256 contiguous bytes.  The kernel is bound by its integer instructions,
// not by bytes, so a lane whose sixteen taps all lie inside the source takes a path
// without clamps and selects; the others clamp every address into the image before the load and apply the
// tap's validity afterwards.  Both decide on the coordinates they are about to use: no table content can
// make a load leave the source.  Row tails and unaligned outputs are written bytewise; nothing beyond `W` in
// a row is written.
#include "rect_kernels.hpp"

namespace rspl {
namespace rect {

namespace {

// cv::remap's bilinear table is 32 * (32 - fx or fx) * (32 - fy or fy), the four weights summing to 32768;
// the same integer, factored
__device__ inline uint32_t blend(int fx, int fy, int t00, int t01, int t10, int t11) {
  const int top = (32 - fx) * t00 + fx * t01, bot = (32 - fx) * t10 + fx * t11;
  const int s = (32 - fy) * top + fy * bot;
  return (uint32_t)((32 * s + 16384) >> 15);
}

__device__ inline int tap_x(uint32_t e) { return (int)(e & 2047u) - 2; }
__device__ inline int tap_y(uint32_t e) { return (int)((e >> 11) & 2047u) - 2; }
__device__ inline int frac_x(uint32_t e) { return (int)((e >> 22) & 31u); }
__device__ inline int frac_y(uint32_t e) { return (int)(e >> 27); }

// all four taps inside the source: the check is on the coordinates themselves, whatever the table holds
// (ints and '&': one mask for the lane's four pixels instead of a chain of branches)
__device__ inline int inside(uint32_t e, int H, int W) {
  return (int)((unsigned)tap_x(e) < (unsigned)(W - 1)) & (int)((unsigned)tap_y(e) < (unsigned)(H - 1));
}

// the plain path: the two taps of a row as one 2-byte load (global loads need no alignment) off a 32-bit
// offset (the host bounds H * stride), no clamps, no selects
__device__ inline uint32_t sample_inside(const uint8_t* __restrict__ src, uint32_t stride, uint32_t e) {
  const uint8_t* p = src + ((uint32_t)tap_y(e) * stride + (uint32_t)tap_x(e));
  uint16_t r0, r1;
  __builtin_memcpy(&r0, p, 2);
  __builtin_memcpy(&r1, p + stride, 2);
  return blend(frac_x(e), frac_y(e), r0 & 255, r0 >> 8, r1 & 255, r1 >> 8);
}

// the border path: every address clamped into the image, the tap's validity applied after the load
__device__ inline uint32_t sample_border(const uint8_t* __restrict__ src, uint32_t stride, int H, int W, uint32_t e) {
  const int ix = tap_x(e), iy = tap_y(e);
  const bool vx0 = (unsigned)ix < (unsigned)W, vx1 = (unsigned)(ix + 1) < (unsigned)W;
  const bool vy0 = (unsigned)iy < (unsigned)H, vy1 = (unsigned)(iy + 1) < (unsigned)H;
  const int x0 = min(max(ix, 0), W - 1), x1 = min(max(ix + 1, 0), W - 1);
  const uint8_t* r0 = src + (uint32_t)min(max(iy, 0), H - 1) * stride;
  const uint8_t* r1 = src + (uint32_t)min(max(iy + 1, 0), H - 1) * stride;
  int t00 = r0[x0], t01 = r0[x1], t10 = r1[x0], t11 = r1[x1];
  t00 = (vx0 && vy0) ? t00 : 0;
  t01 = (vx1 && vy0) ? t01 : 0;
  t10 = (vx0 && vy1) ? t10 : 0;
  t11 = (vx1 && vy1) ? t11 : 0;
  return blend(frac_x(e), frac_y(e), t00, t01, t10, t11);
}

__global__ __launch_bounds__(kTileH * 64) void rect_kernel(const Args a) {
  const int x = blockIdx.x * kTileW + (threadIdx.x & 63) * kPixPerLane;
  const int y = blockIdx.y * kTileH + (threadIdx.x >> 6);
  const int b = blockIdx.z;
  if (y >= a.H || x >= a.W) return;
  const size_t cam = (a.cam_bits[b >> 5] >> (b & 31)) & 1u;
  // (offsets inside a table, a source and an output image are 32-bit: the host bounds them)
  const uint4 e = *reinterpret_cast<const uint4*>(a.table + cam * a.cam_pitch + ((uint32_t)y * a.tpitch + (uint32_t)x));
  const uint8_t* src = a.src + (size_t)b * a.src_pitch;
  uint32_t p0, p1, p2, p3;
  if (inside(e.x, a.H, a.W) & inside(e.y, a.H, a.W) & inside(e.z, a.H, a.W) & inside(e.w, a.H, a.W)) {
    p0 = sample_inside(src, a.src_stride, e.x);
    p1 = sample_inside(src, a.src_stride, e.y);
    p2 = sample_inside(src, a.src_stride, e.z);
    p3 = sample_inside(src, a.src_stride, e.w);
  } else {
    p0 = sample_border(src, a.src_stride, a.H, a.W, e.x);
    p1 = sample_border(src, a.src_stride, a.H, a.W, e.y);
    p2 = sample_border(src, a.src_stride, a.H, a.W, e.z);
    p3 = sample_border(src, a.src_stride, a.H, a.W, e.w);
  }
  uint8_t* out = a.dst + (size_t)b * a.dst_pitch + ((uint32_t)y * a.dst_stride + (uint32_t)x);
  if (a.dst_aligned && x + kPixPerLane <= a.W) {
    *reinterpret_cast<uint32_t*>(out) = p0 | p1 << 8 | p2 << 16 | p3 << 24;
  } else {
    out[0] = (uint8_t)p0;
    if (x + 1 < a.W) out[1] = (uint8_t)p1;
    if (x + 2 < a.W) out[2] = (uint8_t)p2;
    if (x + 3 < a.W) out[3] = (uint8_t)p3;
  }
}

}  // namespace

hipError_t remap(const Args& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  const dim3 grid((a.W + kTileW - 1) / kTileW, (a.H + kTileH - 1) / kTileH, a.batch);
  hipLaunchKernelGGL(rect_kernel, grid, dim3(kTileH * 64), 0, s, a);
  return hipGetLastError();
}

}  // namespace rect
}  // namespace rspl
