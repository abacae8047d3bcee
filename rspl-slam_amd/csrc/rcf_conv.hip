// RCF backbone on gfx950 (CDNA4): the VGG16 3x3 convolutions, the one-channel first layer and the max-pools.
//
// Reference semantics: the network behind RCF::infer (src/rcf.cpp:95-135), yun-liu/RCF-PyTorch's VGG16-based
// RCF; the input is the gray image as raw floats 0..255 in three identical channels (src/rcf.cpp:161-192).
// Layout: activations NHWC, one batch of B images.  The 3x3 convolutions are implicit GEMMs (M = pixels,
// N = output channels, K = 9 * Cin): fp32 on v_mfma_f32_32x32x2_f32 (the reference's precision, kFP16 is
// commented out at src/rcf.cpp:51), fp16 on v_mfma_f32_32x32x16_f16 with fp32 accumulation and epilogue.
//
// The tile shape is the SuperPoint encoder's (sp_conv.hip): 4 waves, TH rows x 16 columns x 64 channels.
// These kernels are units of their own so that the SuperPoint kernels keep their instruction streams; what is
// new here is a run-time Cin up to 512 (the K loop walks it in LDS-staged chunks), a halo of `D` pixels for
// stage 5's dilation 2, and image sizes that are no multiple of the tile (every load and store is bounded).
// No workgroup waits for another one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "rcf_kernels.hpp"

namespace rspl {
namespace rcf {

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ floatx16 mfma32(float a, float b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ floatx16 mfma16(half8 a, half8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

constexpr int TW = 16;        // tile columns
constexpr int CK = 16;        // fp32: input channels per LDS stage
constexpr int CKP = CK + 1;   // fp32: LDS pixel stride (odd: conflict-free A reads)
constexpr int HCK = 32;       // fp16: input channels per LDS stage
constexpr int HCS = HCK + 8;  // fp16: LDS row stride in halves (80 B: conflict-free ds_read_b128)
constexpr int OS = 72;        // fp16: staged output tile, halves per pixel (64 channels + pad)

// ---------------------------------------------------------------------------
// conv1_1: 1 -> 64 channels.  K = 9 would fill 9 of an MFMA step's 16 lanes of K and the layer is 0.1 % of the
// network's multiplies, so it runs on the vector ALU: one thread per pixel and 8 channels, taps in row-major
// order, then the bias.
// ---------------------------------------------------------------------------
template <bool HALF>
__global__ __launch_bounds__(256) void first_kernel(FirstArgs a) {
  const size_t npix = (size_t)a.B * a.H * a.W;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t p = i >> 3;
  const int g = (int)(i & 7);
  if (p >= npix) return;
  const int x = (int)(p % a.W), y = (int)((p / a.W) % a.H);
  const size_t b = p / ((size_t)a.W * a.H);
  const uint8_t* img = a.img + b * a.pitch;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0.f;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
    const float v = (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) ? (float)img[(size_t)yy * a.stride + xx] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = fmaf(v, a.w[k * 64 + 8 * g + j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = fmaxf(acc[j] + a.bias[8 * g + j], 0.f);
  if constexpr (HALF) {
    half8 h;
#pragma unroll
    for (int j = 0; j < 8; j++) h[j] = (_Float16)acc[j];
    *reinterpret_cast<half8*>((_Float16*)a.out + p * 64 + 8 * g) = h;
  } else {
    float* o = (float*)a.out + p * 64 + 8 * g;
    *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(o + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
}

// ---------------------------------------------------------------------------
// fp32 3x3 conv, dilation D, pad D, bias + ReLU.
//   block  = 4 waves; tile = TH rows x 16 cols of output pixels x 64 channels
//   wave   = TH/4 rows (TH/8 M-tiles of 2 rows x 16 cols) x 2 N-tiles of 32 channels
//   K loop = Cin in chunks of CK = 16 through LDS: halo (TH + 2D) x (16 + 2D) pixels, weights [9][CK][64]
// ---------------------------------------------------------------------------
template <int TH, int D>
__global__ __launch_bounds__(256) void conv3x3_kernel(ConvArgs a) {
  constexpr int HX = TW + 2 * D, HY = TH + 2 * D;
  constexpr int MT = TH / 8;
  __shared__ float halo[HY * HX * CKP];
  __shared__ float wts[9 * CK * 64];

  const int H = a.H, W = a.W, CIN = a.cin, COUT = a.cout;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int per_img = tiles_x * tiles_y;
  const int bi = blockIdx.x / per_img;
  const int t = blockIdx.x % per_img;
  const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
  const int co0 = blockIdx.y * 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ml = lane & 31, kl = lane >> 5;
  const float* in = (const float*)a.in + (size_t)bi * H * W * CIN;
  const float* w = (const float*)a.w;

  floatx16 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

  for (int c0 = 0; c0 < CIN; c0 += CK) {
    __syncthreads();
    for (int i = tid; i < HY * HX * (CK / 4); i += 256) {
      const int q = i % (CK / 4), pix = i / (CK / 4);
      const int hy = pix / HX, hx = pix % HX;
      const int y = y0 - D + hy, x = x0 - D + hx;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (y >= 0 && y < H && x >= 0 && x < W)
        v = *reinterpret_cast<const float4*>(in + ((size_t)y * W + x) * CIN + c0 + 4 * q);
      float* d = &halo[pix * CKP + 4 * q];
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    for (int i = tid; i < 9 * CK * 16; i += 256) {
      const int n4 = i % 16, r = i / 16;  // r = kk * CK + ci
      const int kk = r / CK, ci = r % CK;
      const float4 v = *reinterpret_cast<const float4*>(w + ((size_t)(kk * CIN + c0 + ci)) * COUT + co0 + 4 * n4);
      *reinterpret_cast<float4*>(&wts[r * 64 + 4 * n4]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 9; kk++) {
      const int ky = kk / 3, kx = kk % 3;
#pragma unroll
      for (int kc = 0; kc < CK; kc += 2) {
        float av[MT], bv[2];
#pragma unroll
        for (int m = 0; m < MT; m++) {
          const int ly = wv * (TH / 4) + 2 * m + (ml >> 4);
          av[m] = halo[((ly + ky * D) * HX + (ml & 15) + kx * D) * CKP + kc + kl];
        }
#pragma unroll
        for (int n = 0; n < 2; n++) bv[n] = wts[(kk * CK + kc + kl) * 64 + n * 32 + ml];
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
          for (int n = 0; n < 2; n++) acc[m][n] = mfma32(av[m], bv[n], acc[m][n]);
      }
    }
  }

  // accumulator register r of lane half kl is row (r & 3) + 8 (r >> 2) + 4 kl of the M-tile: pixel (row >> 4, row & 15)
  float* out = (float*)a.out + (size_t)bi * H * W * COUT;
#pragma unroll
  for (int n = 0; n < 2; n++) {
    const int co = co0 + n * 32 + ml;
    const float bias = a.bias[co];
#pragma unroll
    for (int m = 0; m < MT; m++) {
      const int ly = wv * (TH / 4) + 2 * m;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int mm = (r & 3) + 8 * (r >> 2) + 4 * kl;
        const int y = y0 + ly + (mm >> 4), x = x0 + (mm & 15);
        const float v = acc[m][n][r] + bias;
        if (y < H && x < W) out[((size_t)y * W + x) * COUT + co] = v > 0.f ? v : 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// fp16 3x3 conv: the same tiling on v_mfma_f32_32x32x16_f16 (lane (r, h) holds A[r][8h..8h+7] and
// B[8h..8h+7][r]: one 16-byte LDS read each), 32 input channels per stage, LDS rows of 40 halves, the next
// stage's operands fetched into registers while the current stage's MFMAs run, fp32 bias + ReLU, the fp16
// output tile staged through LDS so the global stores are 16-byte rows of 8 channels.
// ---------------------------------------------------------------------------
template <int TH, int D>
__global__ __launch_bounds__(256) void conv3x3_h_kernel(ConvArgs a) {
  constexpr int HX = TW + 2 * D, HY = TH + 2 * D;
  constexpr int MT = TH / 8;
  __shared__ __attribute__((aligned(16))) _Float16 halo[HY * HX * HCS];
  __shared__ __attribute__((aligned(16))) _Float16 wts[9 * 64 * HCS];

  const int H = a.H, W = a.W, CIN = a.cin, COUT = a.cout;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int per_img = tiles_x * tiles_y;
  const int co0 = blockIdx.y * 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ml = lane & 31, kl = lane >> 5;
  const int bi = blockIdx.x / per_img;
  const int t = blockIdx.x % per_img;
  const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
  const _Float16* in = (const _Float16*)a.in + (size_t)bi * H * W * CIN;
  const _Float16* hw = (const _Float16*)a.w;

  constexpr int HALO8 = HY * HX * (HCK / 8), HPT = (HALO8 + 255) / 256;
  half8 pw[9], ph[HPT];
  floatx16 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

  auto fetch = [&](int c0) {
#pragma unroll
    for (int r = 0; r < 9; r++) {  // weights [9][64 co][32 ci]: 2304 half8, 9 per thread
      const int i = tid + 256 * r, q = i % (HCK / 8), rr = i / (HCK / 8);
      const int kk = rr / 64, co = rr % 64;
      pw[r] = *reinterpret_cast<const half8*>(hw + ((size_t)kk * COUT + co0 + co) * CIN + c0 + 8 * q);
    }
#pragma unroll
    for (int r = 0; r < HPT; r++) {
      const int i = tid + 256 * r, q = i % (HCK / 8), pix = i / (HCK / 8);
      const int hy = pix / HX, hx = pix % HX;
      const int y = y0 - D + hy, x = x0 - D + hx;
      half8 v = {};
      if (i < HALO8 && y >= 0 && y < H && x >= 0 && x < W)
        v = *reinterpret_cast<const half8*>(in + ((size_t)y * W + x) * CIN + c0 + 8 * q);
      ph[r] = v;
    }
  };
  fetch(0);
  for (int c0 = 0; c0 < CIN; c0 += HCK) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < HPT; r++) {
      const int i = tid + 256 * r;
      if (i < HALO8) *reinterpret_cast<half8*>(&halo[(i / (HCK / 8)) * HCS + 8 * (i % (HCK / 8))]) = ph[r];
    }
#pragma unroll
    for (int r = 0; r < 9; r++) {
      const int i = tid + 256 * r;
      *reinterpret_cast<half8*>(&wts[(i / (HCK / 8)) * HCS + 8 * (i % (HCK / 8))]) = pw[r];
    }
    __syncthreads();
    if (c0 + HCK < CIN) fetch(c0 + HCK);
#pragma unroll
    for (int kk = 0; kk < 9; kk++) {
      const int ky = kk / 3, kx = kk % 3;
#pragma unroll
      for (int ks = 0; ks < HCK; ks += 16) {
        half8 av[MT], bv[2];
#pragma unroll
        for (int m = 0; m < MT; m++) {
          const int ly = wv * (TH / 4) + 2 * m + (ml >> 4);
          av[m] = *reinterpret_cast<const half8*>(&halo[((ly + ky * D) * HX + (ml & 15) + kx * D) * HCS + ks + 8 * kl]);
        }
#pragma unroll
        for (int n = 0; n < 2; n++)
          bv[n] = *reinterpret_cast<const half8*>(&wts[(kk * 64 + n * 32 + ml) * HCS + ks + 8 * kl]);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
          for (int n = 0; n < 2; n++) acc[m][n] = mfma16(av[m], bv[n], acc[m][n]);
      }
    }
  }

  static_assert(TH * 16 * OS <= 9 * 64 * HCS, "output tile exceeds the weight buffer");
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 2; n++) {
    const float bias = a.bias[co0 + n * 32 + ml];
#pragma unroll
    for (int m = 0; m < MT; m++) {
      const int ly = wv * (TH / 4) + 2 * m;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int mm = (r & 3) + 8 * (r >> 2) + 4 * kl;
        const float v = acc[m][n][r] + bias;
        wts[((ly + (mm >> 4)) * 16 + (mm & 15)) * OS + n * 32 + ml] = (_Float16)(v > 0.f ? v : 0.f);
      }
    }
  }
  __syncthreads();
  _Float16* out = (_Float16*)a.out + (size_t)bi * H * W * COUT;
  for (int i = tid; i < TH * 16 * 8; i += 256) {
    const int px = i >> 3, q = i & 7;
    const int y = y0 + (px >> 4), x = x0 + (px & 15);
    if (y < H && x < W)
      *reinterpret_cast<half8*>(out + ((size_t)y * W + x) * COUT + co0 + 8 * q) =
          *reinterpret_cast<const half8*>(&wts[px * OS + 8 * q]);
  }
}

// ---------------------------------------------------------------------------
// 2x2 max-pool, stride 2 or 1, ceil_mode: taps past the last row / column are left out, so a last odd row or
// column pools alone.  One thread per output pixel and 16 bytes of channels.
// ---------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(256) void pool_kernel(PoolArgs a) {
  typedef T vec __attribute__((ext_vector_type(V)));
  const int CV = a.C / V;
  const size_t n = (size_t)a.B * a.Ho * a.Wo * CV;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % CV);
  const size_t p = i / CV;
  const int x = (int)(p % a.Wo), y = (int)((p / a.Wo) % a.Ho);
  const size_t b = p / ((size_t)a.Wo * a.Ho);
  const T* in = (const T*)a.in + b * a.H * a.W * a.C;
  const int iy = y * a.stride, ix = x * a.stride;
  vec m = *reinterpret_cast<const vec*>(in + ((size_t)iy * a.W + ix) * a.C + V * c);
#pragma unroll
  for (int k = 1; k < 4; k++) {
    const int yy = iy + (k >> 1), xx = ix + (k & 1);
    if (yy < a.H && xx < a.W) {
      const vec v = *reinterpret_cast<const vec*>(in + ((size_t)yy * a.W + xx) * a.C + V * c);
#pragma unroll
      for (int j = 0; j < V; j++) m[j] = v[j] > m[j] ? v[j] : m[j];
    }
  }
  *reinterpret_cast<vec*>((T*)a.out + p * a.C + V * c) = m;
}

template <int TH, int D>
hipError_t launch_conv(const ConvArgs& a, bool half, hipStream_t s) {
  const int tiles = ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
  const dim3 grid(a.B * tiles, a.cout / 64);
  if (half)
    hipLaunchKernelGGL((conv3x3_h_kernel<TH, D>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((conv3x3_kernel<TH, D>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t first_conv(const FirstArgs& a, bool half, hipStream_t s) {
  const size_t n = (size_t)a.B * a.H * a.W * 8;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (half)
    hipLaunchKernelGGL(first_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(first_kernel<false>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t conv3x3(const ConvArgs& a, bool half, hipStream_t s) {
  if (a.cout % 64 || a.cin % (half ? HCK : CK) || (a.dilation != 1 && a.dilation != 2) ||
      (a.tile_rows != 0 && a.tile_rows != 8 && a.tile_rows != 16))
    return hipErrorInvalidValue;
  // 8-row tiles where 16-row ones would leave most of the CUs without a workgroup
  // (the same sums in the same order either way: a pixel's K loop does not depend on the tile)
  const bool small = a.tile_rows ? a.tile_rows == 8 : (size_t)a.B * a.H * a.W * (a.cout / 64) <= (size_t)256 * 256 * 4;
  if (a.dilation == 1) return small ? launch_conv<8, 1>(a, half, s) : launch_conv<16, 1>(a, half, s);
  return small ? launch_conv<8, 2>(a, half, s) : launch_conv<16, 2>(a, half, s);
}

hipError_t pool(const PoolArgs& a, bool half, hipStream_t s) {
  const int V = half ? 8 : 4;
  if (a.C % V) return hipErrorInvalidValue;
  const size_t n = (size_t)a.B * a.Ho * a.Wo * (a.C / V);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (half)
    hipLaunchKernelGGL((pool_kernel<_Float16, 8>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((pool_kernel<float, 4>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace rcf
}  // namespace rspl
