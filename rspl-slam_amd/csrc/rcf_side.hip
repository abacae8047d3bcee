// RCF side branches and tail on gfx950 (the network behind RCF::infer, src/rcf.cpp:95-135).
//
// side_kernel: every 3x3 conv's ReLU output goes through its own 1x1 conv (C -> 21, bias) and the maps of a
// stage are summed; the stage's last call also applies score_dsn (21 -> 1).  The 1x1 conv is the transposed
// product D[channel][pixel] = W[channel][k] X[k][pixel] on MFMA with the 21 channels padded to the tile's 32
// rows: both operands are then contiguous runs of the NHWC activation and of the weight rows, loaded straight
// from global memory, and a lane ends up holding 16 channels of ONE pixel, so score_dsn is a sum inside the
// lane plus one exchange between the lane halves.  The stage's sum is built call after call on one stream in
// the order of the convs: no atomics, the same bits every run.
//
// tail_kernel: per output pixel the four bilinear transposed convs (at most 2 x 2 taps each) with their crops,
// score_fuse, the six logits, the sigmoid and process_output's u8 conversion (src/rcf.cpp:147-152).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rcf_kernels.hpp"

#pragma clang fp contract(off)

namespace rspl {
namespace rcf {

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// one wave per 32 pixels, 4 waves per workgroup.  Lane (ml, kl): A operand = weight row ml, B operand = pixel ml,
// both at k = 8 kl .. (fp16) or, for the fp32 steps j = 0..3 of a float4, at k = 4 kl + j: A and B agree on
// which k a lane half carries in which step, which is all the product needs.
template <bool HALF>
__global__ __launch_bounds__(256) void side_kernel(SideArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ml = lane & 31, kl = lane >> 5;
  const size_t p = ((size_t)blockIdx.x * 4 + wv) * 32 + ml;
  const bool valid = p < a.npix;
  const int C = a.C;
  floatx16 d;
#pragma unroll
  for (int r = 0; r < 16; r++) d[r] = 0.f;
  if constexpr (HALF) {
    const _Float16* w = (const _Float16*)a.w + (size_t)ml * C + 8 * kl;
    const _Float16* x = (const _Float16*)a.act + (valid ? p : 0) * C + 8 * kl;
    for (int k0 = 0; k0 < C; k0 += 16) {
      const half8 wa = *reinterpret_cast<const half8*>(w + k0);
      half8 xb = *reinterpret_cast<const half8*>(x + k0);
      if (!valid) xb = half8{};
      d = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa, xb, d, 0, 0, 0);
    }
  } else {
    const float* w = (const float*)a.w + (size_t)ml * C + 4 * kl;
    const float* x = (const float*)a.act + (valid ? p : 0) * C + 4 * kl;
    for (int k0 = 0; k0 < C; k0 += 8) {
      const float4 wa = *reinterpret_cast<const float4*>(w + k0);
      float4 xb = *reinterpret_cast<const float4*>(x + k0);
      if (!valid) xb = make_float4(0.f, 0.f, 0.f, 0.f);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.x, xb.x, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.y, xb.y, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.z, xb.z, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.w, xb.w, d, 0, 0, 0);
    }
  }
  // register 4 q + e of lane half kl: channel 8 q + 4 kl + e of pixel ml
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int cb = 8 * q + 4 * kl;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = d[4 * q + e] + a.bias[cb + e];
    if (cb < kSidePad && valid) {
      float4* dst = reinterpret_cast<float4*>(a.acc + p * kSidePad + cb);
      if (!a.first) {
        const float4 o = *dst;
        v[0] = o.x + v[0]; v[1] = o.y + v[1]; v[2] = o.z + v[2]; v[3] = o.w + v[3];
      }
      if (!a.last) *dst = make_float4(v[0], v[1], v[2], v[3]);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) s += a.dsn_w[cb + e] * v[e];  // rows 21.. carry zero weights
  }
  if (a.last) {
    const float other = __shfl_xor(s, 32);
    if (kl == 0 && valid) a.so[p] = (s + other) + a.dsn_b;
  }
}

// bilinear transposed conv of `so` (Hs x Ws), kernel 2 * st, stride st, at full-resolution pixel (y, x) after a crop
// at `off`: kernel weight (1 - |i - c| / st)(1 - |j - c| / st), c = st - 0.5.  Taps in row-major order of the source.
__device__ __forceinline__ float upsample(const float* so, int Hs, int Ws, int st, int off, int y, int x) {
  const int oy = y + off, ox = x + off;
  const int iy1 = oy / st, ix1 = ox / st;
  const float c = (float)st - 0.5f, f = (float)st;
  float s = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 0; dy++) {
    const int iy = iy1 + dy;
    if (iy < 0 || iy >= Hs) continue;
    const float wy = 1.f - fabsf((float)(oy - iy * st) - c) / f;
#pragma unroll
    for (int dx = -1; dx <= 0; dx++) {
      const int ix = ix1 + dx;
      if (ix < 0 || ix >= Ws) continue;
      const float wx = 1.f - fabsf((float)(ox - ix * st) - c) / f;
      s += (wy * wx) * so[(size_t)iy * Ws + ix];
    }
  }
  return s;
}

__global__ __launch_bounds__(256) void tail_kernel(TailArgs a) {
  const size_t hw = (size_t)a.H * a.W, n = hw * a.B;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t b = i / hw, pix = i % hw;
  const int y = (int)(pix / a.W), x = (int)(pix % a.W);
  constexpr int kStride[kStages] = {1, 2, 4, 8, 8}, kOff[kStages] = {0, 1, 2, 4, 0};
  float v[kStages + 1];
  v[0] = a.so[0][b * hw + pix];
#pragma unroll
  for (int s = 1; s < kStages; s++)
    v[s] = upsample(a.so[s] + b * a.Hs[s] * a.Ws[s], a.Hs[s], a.Ws[s], kStride[s], kOff[s], y, x);
  float fuse = a.fuse_b;
#pragma unroll
  for (int s = 0; s < kStages; s++) fuse += a.fuse_w[s] * v[s];
  v[kStages] = fuse;
  float* lg = a.logits + b * 6 * hw + pix;
  float sel = 0.f;
#pragma unroll
  for (int k = 0; k <= kStages; k++) {
    lg[k * hw] = v[k];
    if (k == a.output) sel = v[k];
  }
  const float p = 1.f / (1.f + expf(-sel));
  a.edges[b * a.out_pitch + (size_t)y * a.out_stride + x] = (uint8_t)(unsigned)(255.0f - p * 255.0f);
}

}  // namespace

hipError_t side(const SideArgs& a, bool half, hipStream_t s) {
  if (a.C % 16) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.npix + 127) / 128));
  if (half)
    hipLaunchKernelGGL(side_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(side_kernel<false>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t tail(const TailArgs& a, hipStream_t s) {
  const size_t n = (size_t)a.B * a.H * a.W;
  hipLaunchKernelGGL(tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace rcf
}  // namespace rspl
