// Device-side pieces shared by the SuperPoint units (sp_conv.hip, sp_heads.hip): MFMA operand types and wrappers,
// the conv tile constants, accumulator helpers for the heads, the bilinear tap geometry and the 65-way softmax.  Every helper keeps the floating-point operation order of the kernels it was lifted from.
//
// The conv kernels (sp_conv.hip) take only the types and tile constants from here.  Their tile addressing, pool
// pattern, LDS-staged epilogue and conv1a-on-MFMA operand build stay written out per kernel: a helper is inlined
// only after the compiler's first simplification round, and for those bodies that changed register allocation
// (VGPR counts moved by 1 to 28, SGPR counts by 1 or 2) or the instruction schedule although the arithmetic was
// the same.  A function is used in a kernel only if the kernel keeps its VGPR / AGPR / SGPR / LDS / occupancy row
// and its stage its time.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rspl {
namespace sp {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ floatx16 mfma32(float a, float b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ floatx16 mfma16(half8 a, half8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// split fp16 (RSPL_PREC_FP16X3): v = hi + lo, hi = (half)v, lo = (half)(v - hi)
struct Half2 {
  _Float16 hi, lo;
};
__device__ __forceinline__ Half2 split16(float v) {
  const _Float16 hi = (_Float16)v;
  return {hi, (_Float16)(v - (float)hi)};
}

// ---------------------------------------------------------------------------
// conv tiles: a 256-thread workgroup owns TH rows x TW cols of output pixels x 64 channels; wave wv owns rows
// wv * TH/4 .., as TH/8 M-tiles of 2 rows x 16 cols, times 2 N-tiles of 32 channels (lane (ml, kl): channel ml).
// ---------------------------------------------------------------------------
constexpr int TW = 16;
constexpr int CK = 16;        // fp32: input channels per stage
constexpr int CKP = CK + 1;   // fp32: LDS pixel stride (odd: conflict-free A reads)
constexpr int HCK = 32;       // fp16: input channels per stage
constexpr int HCS = HCK + 8;  // fp16: LDS row stride in halves (80 B: conflict-free ds_read_b128)
constexpr int C1S = 72;       // resident conv1: LDS row stride (halves) of the weight and halo rows, 64 channels + 8
constexpr int XCK = 16;       // split fp16: input channels per stage
constexpr int XCS = XCK + 8;  // split fp16: LDS row stride in halves (48-byte rows: conflict-free ds_read_b128)
constexpr int OS = 72;        // staged output tile: halves per pixel row in LDS (64 channels + pad)

__device__ __forceinline__ void zero(floatx16& d) {
#pragma unroll
  for (int r = 0; r < 16; r++) d[r] = 0.f;
}
template <int N>
__device__ __forceinline__ void zero(floatx16 (&acc)[N]) {
#pragma unroll
  for (int n = 0; n < N; n++) zero(acc[n]);
}

// accumulator register r of lane half kl -> row of the 32-row MFMA tile (a conv M-tile: pixel (row >> 4, row & 15))
__device__ __forceinline__ int acc_row(int r, int kl) { return (r & 3) + 8 * (r >> 2) + 4 * kl; }

// ---------------------------------------------------------------------------
// normalize_keypoints (src/super_point.cpp:276-287; s/2 is integer division) and grid_sample (:294-332,
// align_corners = True) of keypoint (x, y) on the h x w cell grid: cells and weights in nw, ne, sw, se order
// ---------------------------------------------------------------------------
struct BilinearTaps {
  int ix[4], iy[4];  // cell column and row
  double wt[4];
};
__device__ __forceinline__ BilinearTaps bilinear_taps(int x, int y, int h, int w) {
  const double gx = ((double)x - 8 / 2 + 0.5) / (w * 8 - 8 / 2 - 0.5) * 2 - 1;
  const double gy = ((double)y - 8 / 2 + 0.5) / (h * 8 - 8 / 2 - 0.5) * 2 - 1;
  const double ix = ((gx + 1) / 2) * (w - 1), iy = ((gy + 1) / 2) * (h - 1);
  auto clip = [](int v, int m) { return v < 0 ? 0 : (v < m - 1 ? v : m - 1); };
  const int ix_nw = clip((int)floor(ix), w), iy_nw = clip((int)floor(iy), h);
  const int ix_ne = clip(ix_nw + 1, w), iy_ne = clip(iy_nw, h);
  const int ix_sw = clip(ix_nw, w), iy_sw = clip(iy_nw + 1, h);
  const int ix_se = clip(ix_nw + 1, w), iy_se = clip(iy_nw + 1, h);
  BilinearTaps t;
  t.wt[0] = (ix_se - ix) * (iy_se - iy);
  t.wt[1] = (ix - ix_sw) * (iy_sw - iy);
  t.wt[2] = (ix_ne - ix) * (iy - iy_ne);
  t.wt[3] = (ix - ix_nw) * (iy - iy_nw);
  t.ix[0] = ix_nw; t.iy[0] = iy_nw;
  t.ix[1] = ix_ne; t.iy[1] = iy_ne;
  t.ix[2] = ix_sw; t.iy[2] = iy_sw;
  t.ix[3] = ix_se; t.iy[3] = iy_se;
  return t;
}

// softmax over the 65 real channels of accumulator row r (NT N-tiles of 32 columns, column n * 32 + ml; columns
// >= 65 are padding): e[n] = exp(acc - max), returns their sum over the row
template <int NT>
__device__ __forceinline__ float softmax65_row(const floatx16 (&acc)[NT], int r, int ml, float (&e)[NT]) {
  float m = -INFINITY;
#pragma unroll
  for (int n = 0; n < NT; n++)
    if (n * 32 + ml < 65) m = fmaxf(m, acc[n][r]);
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 32));
  float s = 0.f;
#pragma unroll
  for (int n = 0; n < NT; n++) {
    e[n] = (n * 32 + ml < 65) ? expf(acc[n][r] - m) : 0.f;
    s += e[n];
  }
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o, 32);
  return s;
}

}  // namespace sp
}  // namespace rspl
