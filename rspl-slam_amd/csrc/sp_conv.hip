// SuperPoint encoder on gfx950 (CDNA4): the 3x3 convolutions of the three precisions.
//
// Reference semantics:
//   network  convert2onnx/superpoint.py:114-161  (encoder, detector & descriptor heads)
//   host     src/super_point.cpp:137-152         (u8/255 input normalisation)
// Layout: activations NHWC (channels contiguous), one batch of B images.
// Convolutions are implicit GEMMs (M = pixels, N = output channels, K = 9*Cin): fp32 on
// v_mfma_f32_32x32x2_f32 (exact fp32: one rounding per product, like fmaf), fp16 and split fp16 on
// v_mfma_f32_32x32x16_f16.
//
// The four kernels share sp_device.hpp's types and tile constants and nothing else: each keeps its own tile
// addressing, accumulator-to-pixel map, pool pattern and staged epilogue.  Written as shared inline functions these
// gave the same arithmetic but other register counts or another instruction schedule, and stage times that left the
// parent's run-to-run spread; every kernel here compiles to the instruction stream it had before the units were
// split (profiles/sp_split_kernels.md).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdint>

#include "sp_device.hpp"
#include "sp_kernels.hpp"

namespace rspl {
namespace sp {

// ---------------------------------------------------------------------------
// 3x3 conv, pad 1, bias + ReLU (+ 2x2 max-pool) as an implicit GEMM.
//   block  = 4 waves; tile = TH rows x 16 cols of output pixels x 64 channels
//   wave   = TH/4 rows (TH/8 M-tiles of 2 rows x 16 cols) x 2 N-tiles of 32 ch
//   K loop = Cin in chunks of CK=16, staged in LDS with the 1-pixel halo;
//            weights staged as [9][CK][64].
// FUSE1A: the input tile is conv1a(relu) computed on the fly from the u8
// image (src/super_point.cpp:146-150 normalisation via LUT), so the 64-channel
// full-resolution conv1a map never touches HBM.
// ---------------------------------------------------------------------------
template <int CIN, int TH, bool POOL, bool FUSE1A>
__global__ __launch_bounds__(256) void conv3x3_kernel(ConvArgs a) {
  static_assert(CIN % CK == 0, "Cin must be a multiple of 16");
  constexpr int HX = TW + 2, HY = TH + 2;
  constexpr int MT = TH / 8;  // M-tiles per wave
  __shared__ float halo[HY * HX * CKP];
  __shared__ float wts[9 * CK * 64];
  __shared__ float patch[FUSE1A ? (TH + 4) * (TW + 4) : 1];
  __shared__ float w1a[FUSE1A ? 64 * 10 : 1];

  const int H = a.H, W = a.W, COUT = a.cout;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int per_img = tiles_x * tiles_y;
  const int bi = blockIdx.x / per_img;
  const int t = blockIdx.x % per_img;
  const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
  const int co0 = blockIdx.y * 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ml = lane & 31, kl = lane >> 5;

  if constexpr (FUSE1A) {
    // image patch (TH+4) x (TW+4), rows y0-2.., cols x0-2.., zero outside (conv1a padding)
    const uint8_t* img = a.img + (size_t)bi * a.img_pitch;
    for (int i = tid; i < (TH + 4) * (TW + 4); i += 256) {
      const int py = i / (TW + 4), px = i % (TW + 4);
      const int y = y0 - 2 + py, x = x0 - 2 + px;
      patch[i] = (y >= 0 && y < H && x >= 0 && x < W) ? a.lut[img[(size_t)y * a.img_stride + x]] : 0.f;
    }
    for (int i = tid; i < 64 * 10; i += 256) w1a[i] = (i % 10 < 9) ? a.w1a[(i / 10) * 9 + i % 10] : a.b1a[i / 10];
  }

  floatx16 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

  for (int c0 = 0; c0 < CIN; c0 += CK) {
    __syncthreads();
    // ---- stage input halo (chunk c0..c0+CK) ----
    if constexpr (FUSE1A) {
      for (int i = tid; i < HY * HX * CK; i += 256) {
        const int c = i % CK, pix = i / CK;
        const int hy = pix / HX, hx = pix % HX;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        float v = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
          const float* wc = &w1a[(c0 + c) * 10];
          float s = wc[9];
#pragma unroll
          for (int ky = 0; ky < 3; ky++)
#pragma unroll
            for (int kx = 0; kx < 3; kx++) s += wc[ky * 3 + kx] * patch[(hy + ky) * (TW + 4) + hx + kx];
          v = s > 0.f ? s : 0.f;
        }
        halo[pix * CKP + c] = v;
      }
    } else {
      const float* in = a.in + (size_t)bi * H * W * CIN;
      for (int i = tid; i < HY * HX * (CK / 4); i += 256) {
        const int q = i % (CK / 4), pix = i / (CK / 4);
        const int hy = pix / HX, hx = pix % HX;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y >= 0 && y < H && x >= 0 && x < W)
          v = *reinterpret_cast<const float4*>(in + ((size_t)y * W + x) * CIN + c0 + 4 * q);
        float* d = &halo[pix * CKP + 4 * q];
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
    }
    // ---- stage weights [9][CK][64] ----
    for (int i = tid; i < 9 * CK * 16; i += 256) {
      const int n4 = i % 16, r = i / 16;  // r = kk*CK + ci
      const int kk = r / CK, ci = r % CK;
      const float4 v = *reinterpret_cast<const float4*>(a.w + ((size_t)(kk * CIN + c0 + ci)) * COUT + co0 + 4 * n4);
      *reinterpret_cast<float4*>(&wts[r * 64 + 4 * n4]) = v;
    }
    __syncthreads();
    // ---- MFMA over this chunk ----
#pragma unroll
    for (int kk = 0; kk < 9; kk++) {
      const int ky = kk / 3, kx = kk % 3;
#pragma unroll
      for (int kc = 0; kc < CK; kc += 2) {
        float av[MT], bv[2];
#pragma unroll
        for (int m = 0; m < MT; m++) {
          const int ly = wv * (TH / 4) + 2 * m + (ml >> 4);
          av[m] = halo[((ly + ky) * HX + (ml & 15) + kx) * CKP + kc + kl];
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

  // ---- epilogue: bias + ReLU (+ pool), NHWC store ----
#pragma unroll
  for (int n = 0; n < 2; n++) {
    const int co = co0 + n * 32 + ml;
    const float bias = a.bias[co];
#pragma unroll
    for (int m = 0; m < MT; m++) {
      const int ly = wv * (TH / 4) + 2 * m;  // first of the M-tile's two rows
      if constexpr (POOL) {
        const int H2 = H / 2, W2 = W / 2;
        float* out = a.out + (size_t)bi * H2 * W2 * COUT;
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int r0 = (g & 1) * 2 + (g >> 1) * 4;
          const int pc = (r0 & 3) + 8 * ((r0 >> 2) & 1) + 4 * kl;
          float v = fmaxf(fmaxf(acc[m][n][r0], acc[m][n][r0 + 1]), fmaxf(acc[m][n][r0 + 8], acc[m][n][r0 + 9]));
          v += bias;
          v = v > 0.f ? v : 0.f;
          const int py = (y0 + ly) >> 1, px = (x0 + pc) >> 1;
          if (py < H2 && px < W2) out[((size_t)py * W2 + px) * COUT + co] = v;
        }
      } else {
        float* out = a.out + (size_t)bi * H * W * COUT;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int mm = (r & 3) + 8 * (r >> 2) + 4 * kl;
          const int y = y0 + ly + (mm >> 4), x = x0 + (mm & 15);
          float v = acc[m][n][r] + bias;
          v = v > 0.f ? v : 0.f;
          if (y < H && x < W) out[((size_t)y * W + x) * COUT + co] = v;
        }
      }
    }
  }
}

template <int CIN, int TH, bool POOL, bool FUSE1A>
static hipError_t launch_conv(const ConvArgs& a, int B, hipStream_t s, hipEvent_t t0 = nullptr,
                              hipEvent_t t1 = nullptr) {
  const int tiles = ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
  dim3 grid(B * tiles, a.cout / 64);
  hipExtLaunchKernelGGL((conv3x3_kernel<CIN, TH, POOL, FUSE1A>), grid, dim3(256), 0, s, t0, t1, 0, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// fp16 variant of the 3x3 conv (RSPL_PREC_FP16 = the reference's TensorRT kFP16
// engines): same tiling, v_mfma_f32_32x32x16_f16 (lane (r, h) holds A[r][8h..8h+7] and
// B[8h..8h+7][r]: one 16-byte LDS read each), 32 input channels per stage, LDS rows of
// 40 halves (80 B: conflict-free ds_read_b128), fp32 accumulation, bias/ReLU/pool epilogue.
// ---------------------------------------------------------------------------
template <int CIN, int TH, bool POOL>
__global__ __launch_bounds__(256) void conv3x3_h_kernel(ConvArgs a) {
  static_assert(CIN % HCK == 0, "Cin must be a multiple of 32");
  constexpr int HX = TW + 2, HY = TH + 2;
  constexpr int MT = TH / 8;
  __shared__ __attribute__((aligned(16))) _Float16 halo[HY * HX * HCS];
  __shared__ __attribute__((aligned(16))) _Float16 wts[9 * 64 * HCS];

  const int H = a.H, W = a.W, COUT = a.cout;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int per_img = tiles_x * tiles_y;
  const int co0 = blockIdx.y * 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ml = lane & 31, kl = lane >> 5;

  constexpr int HALO8 = HY * HX * (HCK / 8), HPT = (HALO8 + 255) / 256;
  half8 pw[9], ph[HPT];  // the next stage's weights / halo in flight
  const int tile = blockIdx.x;  // one tile per workgroup (grid = tiles)
  const int bi = tile / per_img;
  const int t = tile % per_img;
  const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
  floatx16 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

  // software pipeline over the input-channel stages: the next stage's weights and halo are fetched into
  // registers while the current stage's MFMAs run, and written to LDS after the next barrier
  auto fetch = [&](int c0) {
#pragma unroll
    for (int r = 0; r < 9; r++) {  // weights [9][64 co][32 ci]: 2304 half8, 9 per thread
      const int i = tid + 256 * r, q = i % (HCK / 8), rr = i / (HCK / 8);
      const int kk = rr / 64, co = rr % 64;
      pw[r] = *reinterpret_cast<const half8*>(a.hw + ((size_t)kk * COUT + co0 + co) * CIN + c0 + 8 * q);
    }
    {
      const _Float16* in = a.hin + (size_t)bi * H * W * CIN;
#pragma unroll
      for (int r = 0; r < HPT; r++) {
        const int i = tid + 256 * r, q = i % (HCK / 8), pix = i / (HCK / 8);
        const int hy = pix / HX, hx = pix % HX;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        half8 v = {};
        if (i < HALO8 && y >= 0 && y < H && x >= 0 && x < W)
          v = *reinterpret_cast<const half8*>(in + ((size_t)y * W + x) * CIN + c0 + 8 * q);
        ph[r] = v;
      }
    }
  };
  fetch(0);
  for (int c0 = 0; c0 < CIN; c0 += HCK) {
    __syncthreads();
    {
#pragma unroll
      for (int r = 0; r < HPT; r++) {
        const int i = tid + 256 * r;
        if (i < HALO8) *reinterpret_cast<half8*>(&halo[(i / (HCK / 8)) * HCS + 8 * (i % (HCK / 8))]) = ph[r];
      }
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
          av[m] = *reinterpret_cast<const half8*>(&halo[((ly + ky) * HX + (ml & 15) + kx) * HCS + ks + 8 * kl]);
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

  if constexpr (!POOL) {
    // full-resolution fp16 output staged through LDS (the weight buffer, free after the last
    // stage) so the global stores are 16-byte rows of 8 channels instead of 2-byte scatters
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
    for (int i = tid; i < TH * 16 * 8; i += 256) {
      const int px = i >> 3, q = i & 7;
      const int y = y0 + (px >> 4), x = x0 + (px & 15);
      if (y < H && x < W)
        *reinterpret_cast<half8*>(a.hout + (size_t)bi * H * W * COUT + ((size_t)y * W + x) * COUT + co0 + 8 * q) =
            *reinterpret_cast<const half8*>(&wts[px * OS + 8 * q]);
    }
  } else {
    // 2x2-pooled output tile (TH/2 x 8 pixels x 64 channels) staged through LDS the same way
    static_assert((TH / 2) * 8 * OS <= 9 * 64 * HCS, "pooled tile exceeds the weight buffer");
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 2; n++) {
      const float bias = a.bias[co0 + n * 32 + ml];
#pragma unroll
      for (int m = 0; m < MT; m++) {
        const int pyl = wv * (TH / 8) + m;  // (wv * TH/4 + 2m) / 2
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int r0 = (g & 1) * 2 + (g >> 1) * 4;
          const int pc = (r0 & 3) + 8 * ((r0 >> 2) & 1) + 4 * kl;
          float v = fmaxf(fmaxf(acc[m][n][r0], acc[m][n][r0 + 1]), fmaxf(acc[m][n][r0 + 8], acc[m][n][r0 + 9]));
          v += bias;
          wts[(pyl * 8 + (pc >> 1)) * OS + n * 32 + ml] = (_Float16)(v > 0.f ? v : 0.f);
        }
      }
    }
    __syncthreads();
    const int H2 = H / 2, W2 = W / 2;
    for (int i = tid; i < (TH / 2) * 8 * 8; i += 256) {
      const int px = i >> 3, q = i & 7;
      const int py = (y0 >> 1) + (px >> 3), pxx = (x0 >> 1) + (px & 7);
      if (py < H2 && pxx < W2)
        *reinterpret_cast<half8*>(a.hout + (size_t)bi * H2 * W2 * COUT + ((size_t)py * W2 + pxx) * COUT + co0 + 8 * q) =
            *reinterpret_cast<const half8*>(&wts[px * OS + 8 * q]);
    }
  }
}

template <int CIN, int TH, bool POOL>
static hipError_t launch_conv_h(const ConvArgs& a, int B, hipStream_t s) {
  const int tiles = ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
  dim3 grid(B * tiles, a.cout / 64);
  hipLaunchKernelGGL((conv3x3_h_kernel<CIN, TH, POOL>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// conv1 (conv1a 1->64 + ReLU + conv1b 64->64 + ReLU + 2x2 max-pool, superpoint.py:120-124) with the
// whole conv1b weight tensor RESIDENT in LDS: one persistent 256-thread workgroup per CU walks 16x16-pixel
// output tiles.  The round-4 per-stage kernel (removed in round 6) restaged each 32-channel half of the weights
// per tile and per stage (two workgroups per CU, 76 KB each, phases separated by barriers: 29 % MFMA-busy SIMD
// time, profiles/r05_experiments.md).  Here per tile: the image patch (prefetched during the previous tile's
// MFMAs) -> LDS; conv1a of all 64 channels on MFMA (transposed product: 8-byte LDS stores) into the halo;
// 144 v_mfma_f32_32x32x16_f16 per wave from LDS; bias + ReLU + pool through LDS to 16-byte stores.
// LDS: weights 9 x 64 x 72 halves (82.9 KB) + halo 18 x 18 x 72 halves (46.7 KB) + patch + conv1a weights.
// The same fp16 roundings of the same fp32 accumulations as that kernel (bitwise equal in round 5's A/B):
// conv1a one MFMA over the 9 taps + bias, conv1b the MFMA k-steps in the same channel order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv1_res_kernel(ConvArgs a) {
  constexpr int TH = 16, HX = TW + 2, HY = TH + 2, MT = TH / 8, CIN = 64;
  extern __shared__ __attribute__((aligned(16))) _Float16 c1lds[];
  _Float16* wts = c1lds;                              // [9][64 co][C1S]
  _Float16* halo = wts + 9 * 64 * C1S;                // [HY][HX][C1S]; the pooled output staging afterwards
  float* patch = reinterpret_cast<float*>(halo + HY * HX * C1S);  // [TH + 4][TW + 4]
  float* w1a = patch + (TH + 4) * (TW + 4);           // [64][10] taps + bias

  const int H = a.H, W = a.W;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int per_img = tiles_x * tiles_y, ntiles = a.B * per_img;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ml = lane & 31, kl = lane >> 5;

  constexpr int PP = ((TH + 4) * (TW + 4) + 255) / 256;
  int pv[PP];
  auto load_patch = [&](int tile_) {
    const int bi_ = tile_ / per_img, t_ = tile_ % per_img;
    const int y0_ = (t_ / tiles_x) * TH, x0_ = (t_ % tiles_x) * TW;
    const uint8_t* img = a.img + (size_t)bi_ * a.img_pitch;
#pragma unroll
    for (int r = 0; r < PP; r++) {
      const int i = tid + 256 * r, py = i / (TW + 4), px = i % (TW + 4);
      const int y = y0_ - 2 + py, x = x0_ - 2 + px;
      pv[r] = (i < (TH + 4) * (TW + 4) && tile_ < ntiles && y >= 0 && y < H && x >= 0 && x < W)
                  ? (int)img[(size_t)y * a.img_stride + x]
                  : -1;
    }
  };
  load_patch(blockIdx.x);
  // the workgroup's resident weights: conv1b [9][64 co][64 ci] (16-byte pieces) and conv1a
  for (int i = tid; i < 9 * 64 * 8; i += 256) {
    const int q = i & 7, row = i >> 3;
    *reinterpret_cast<half8*>(&wts[row * C1S + 8 * q]) = *reinterpret_cast<const half8*>(a.hw + (size_t)row * CIN + 8 * q);
  }
  for (int i = tid; i < 64 * 10; i += 256) w1a[i] = (i % 10 < 9) ? a.w1a[(i / 10) * 9 + i % 10] : a.b1a[i / 10];
  __syncthreads();
  // conv1a B operands of the two 32-channel halves (A[c][k]: lane (c, kl) holds k = 8 kl .. 8 kl + 7)
  half8 bw[2];
#pragma unroll
  for (int hf = 0; hf < 2; hf++)
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int k = 8 * kl + j;
      bw[hf][j] = (_Float16)(k <= 9 ? w1a[(32 * hf + ml) * 10 + k] : 0.f);
    }
  float bias[2];
#pragma unroll
  for (int n = 0; n < 2; n++) bias[n] = a.bias[n * 32 + ml];

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int bi = tile / per_img, t = tile % per_img;
    const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
#pragma unroll
    for (int r = 0; r < PP; r++) {  // (every reader of the previous tile's patch and staging has passed a barrier)
      const int i = tid + 256 * r;
      // src/super_point.cpp:146-150 normalisation, (float)(u / 255.0) in double (= the host LUT)
      if (i < (TH + 4) * (TW + 4)) patch[i] = pv[r] >= 0 ? (float)((double)pv[r] / 255.0) : 0.f;
    }
    __syncthreads();
    // conv1a -> ReLU -> fp16 halo, all 64 channels: D[c][px] = W1a[c][k] P[k][px] per halo row and channel half
    {
      const int hx = ml, x = x0 - 1 + hx;
      for (int hy = wv; hy < HY; hy += 4) {
        const int y = y0 - 1 + hy;
        half8 av;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int k = 8 * kl + j;
          float v = 0.f;
          if (hx < HX) v = k < 9 ? patch[(hy + k / 3) * (TW + 4) + hx + k % 3] : (k == 9 ? 1.f : 0.f);
          av[j] = (_Float16)v;
        }
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
          floatx16 d;
#pragma unroll
          for (int r = 0; r < 16; r++) d[r] = 0.f;
          d = mfma16(bw[hf], av, d);
          if (hx < HX) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
              half4 h4;
#pragma unroll
              for (int e = 0; e < 4; e++) h4[e] = (_Float16)(in ? fmaxf(d[4 * q + e], 0.f) : 0.f);
              *reinterpret_cast<half4*>(&halo[(hy * HX + hx) * C1S + 32 * hf + 8 * q + 4 * kl]) = h4;
            }
          }
        }
      }
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) load_patch(tile + gridDim.x);  // in flight during the MFMAs
    floatx16 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int n = 0; n < 2; n++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;
    // the two 32-channel stages of conv3x3_h_kernel in the same order: stage, tap, k-step
#pragma unroll
    for (int c0 = 0; c0 < CIN; c0 += 32)
#pragma unroll
      for (int kk = 0; kk < 9; kk++) {
        const int ky = kk / 3, kx = kk % 3;
#pragma unroll
        for (int ks = 0; ks < 32; ks += 16) {
          half8 av[MT], bv[2];
#pragma unroll
          for (int m = 0; m < MT; m++) {
            const int ly = wv * (TH / 4) + 2 * m + (ml >> 4);
            av[m] = *reinterpret_cast<const half8*>(&halo[((ly + ky) * HX + (ml & 15) + kx) * C1S + c0 + ks + 8 * kl]);
          }
#pragma unroll
          for (int n = 0; n < 2; n++)
            bv[n] = *reinterpret_cast<const half8*>(&wts[(kk * 64 + n * 32 + ml) * C1S + c0 + ks + 8 * kl]);
#pragma unroll
          for (int m = 0; m < MT; m++)
#pragma unroll
            for (int n = 0; n < 2; n++) acc[m][n] = mfma16(av[m], bv[n], acc[m][n]);
        }
      }
    // bias + ReLU + 2x2 max-pool, the pooled (TH / 2) x 8 x 64 tile staged in LDS (the halo, now free)
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 2; n++) {
#pragma unroll
      for (int m = 0; m < MT; m++) {
        const int pyl = wv * (TH / 8) + m;
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int r0 = (g & 1) * 2 + (g >> 1) * 4;
          const int pc = (r0 & 3) + 8 * ((r0 >> 2) & 1) + 4 * kl;
          float v = fmaxf(fmaxf(acc[m][n][r0], acc[m][n][r0 + 1]), fmaxf(acc[m][n][r0 + 8], acc[m][n][r0 + 9]));
          v += bias[n];
          halo[(pyl * 8 + (pc >> 1)) * OS + n * 32 + ml] = (_Float16)(v > 0.f ? v : 0.f);
        }
      }
    }
    __syncthreads();
    const int H2 = H / 2, W2 = W / 2;
    for (int i = tid; i < (TH / 2) * 8 * 8; i += 256) {
      const int px = i >> 3, q = i & 7;
      const int py = (y0 >> 1) + (px >> 3), pxx = (x0 >> 1) + (px & 7);
      if (py < H2 && pxx < W2)
        *reinterpret_cast<half8*>(a.hout + (size_t)bi * H2 * W2 * 64 + ((size_t)py * W2 + pxx) * 64 + 8 * q) =
            *reinterpret_cast<const half8*>(&halo[px * OS + 8 * q]);
    }
  }
}

// the device's CU count (the persistent conv1's grid)
static int device_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || cus <= 0)
      cus = 256;
    n = cus;
  }
  return n;
}

static hipError_t launch_conv1_res(const ConvArgs& a, int B, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {
  constexpr size_t lds = sizeof(_Float16) * (9 * 64 * C1S + 18 * 18 * C1S) + sizeof(float) * (20 * 20 + 64 * 10);
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute((const void*)conv1_res_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    attr = true;
  }
  ConvArgs b = a;
  b.B = B;
  const int tiles = B * ((a.W + TW - 1) / TW) * ((a.H + 15) / 16);
  // one persistent workgroup on every other CU: each holds 131 KB of a CU's LDS for the whole conv1, so on a
  // CU it occupies no local-BA Schur chunk wave (35 KB) fits -- with a workgroup on every CU the BA chain
  // stalled for the length of conv1 every step.  Measured in the C3 pipeline (r05 experiments): 256 workgroups
  // 936 frames/s, 192 951-967, 128 976-977 (conv1 0.15 -> 0.19 ms, off the critical path).
  const int wgs = std::max(1, device_cus() / 2);
  hipExtLaunchKernelGGL(conv1_res_kernel, dim3(std::min(tiles, wgs)), dim3(256), lds, s, t0, t1, 0, b);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Split-fp16 3x3 conv (RSPL_PREC_FP16X3): fp32-grade accuracy at the fp16 MFMA rate.  Every operand is
// carried as a pair of fp16 planes, v = hi + lo (hi = (half)v, lo = (half)(v - hi): 22 significant bits,
// lo unscaled -- below |v| ~ 0.125 it is subnormal, its absolute error then under 3e-8), and each k-step
// accumulates the three products hi*hi + lo*hi + hi*lo on v_mfma_f32_32x32x16_f16 into ONE fp32
// accumulator (the dropped lo*lo term is 2^-22 relative).  Against the fp32 oracle this keeps SuperPoint's
// keypoint sets identical where the fp16 path loses 1-5 of 400 keypoints per image near the top-k cut
// (tools/sp_fp16_split.py: a CPU emulation of both paths over the C1 images).  Same tiling as
// conv3x3_h_kernel with 16 input channels per stage (LDS: hi + lo halo and weights, 86 KB at TH = 16, so a
// local-BA Schur chunk wave (35 KB) still fits beside a workgroup); conv1a (FUSE1A) runs split on MFMA
// too, from the image in fp32 (u8 / 255 as src/super_point.cpp:146-150) split into hi + lo.
// Output planes: hout (hi) and hout_lo (lo), the same NHWC layout.
// ---------------------------------------------------------------------------
template <int CIN, int TH, bool POOL, bool FUSE1A>
__global__ __launch_bounds__(256) void conv3x3_x3_kernel(ConvArgs a) {
  static_assert(CIN % 32 == 0, "Cin must be a multiple of 32");
  constexpr int HX = TW + 2, HY = TH + 2, MT = TH / 8;
  constexpr int HALO = HY * HX * XCS, WTS = 9 * 64 * XCS;
  __shared__ __attribute__((aligned(16))) _Float16 halo[2 * HALO];  // [hi | lo]
  __shared__ __attribute__((aligned(16))) _Float16 wts[2 * WTS];    // [hi | lo]: [9][64 co][XCS]
  __shared__ float patch[FUSE1A ? (TH + 4) * (TW + 4) : 1];

  const int H = a.H, W = a.W, COUT = a.cout;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int per_img = tiles_x * tiles_y;
  const int bi = blockIdx.x / per_img, t = blockIdx.x % per_img;
  const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
  const int co0 = blockIdx.y * 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ml = lane & 31, kl = lane >> 5;

  if constexpr (FUSE1A) {
    const uint8_t* img = a.img + (size_t)bi * a.img_pitch;
    for (int i = tid; i < (TH + 4) * (TW + 4); i += 256) {
      const int py = i / (TW + 4), px = i % (TW + 4);
      const int y = y0 - 2 + py, x = x0 - 2 + px;
      // src/super_point.cpp:146-150 normalisation, (float)(u / 255.0) in double (= the host LUT)
      patch[i] = (y >= 0 && y < H && x >= 0 && x < W) ? (float)((double)img[(size_t)y * a.img_stride + x] / 255.0)
                                                      : 0.f;
    }
  }
  floatx16 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

  // next stage's weights / halo (hi and lo) in registers while the current stage runs on MFMA
  constexpr int W8 = 9 * 64 * (XCK / 8);               // half8 per weight plane per stage
  constexpr int WPT = 2 * W8 / 256;                    // 9
  static_assert(2 * W8 % 256 == 0, "weight staging");
  constexpr int HALO8 = HY * HX * (XCK / 8), HPT = (2 * HALO8 + 255) / 256;
  half8 pw[WPT], ph[FUSE1A ? 1 : HPT];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int r = 0; r < WPT; r++) {
      const int i = tid + 256 * r, pl = i / W8, j = i % W8, q = j % (XCK / 8), rr = j / (XCK / 8);
      const int kk = rr / 64, co = rr % 64;
      pw[r] = *reinterpret_cast<const half8*>((pl ? a.hw_lo : a.hw) + ((size_t)kk * COUT + co0 + co) * CIN + c0 + 8 * q);
    }
    if constexpr (!FUSE1A) {
#pragma unroll
      for (int r = 0; r < HPT; r++) {
        const int i = tid + 256 * r, pl = i / HALO8, j = i % HALO8, q = j % (XCK / 8), pix = j / (XCK / 8);
        const int hy = pix / HX, hx = pix % HX;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        half8 v = {};
        if (i < 2 * HALO8 && y >= 0 && y < H && x >= 0 && x < W)
          v = *reinterpret_cast<const half8*>((pl ? a.hin_lo : a.hin) + (size_t)bi * H * W * CIN +
                                              ((size_t)y * W + x) * CIN + c0 + 8 * q);
        ph[r] = v;
      }
    }
  };
  // conv1a operands (FUSE1A): B[k][c] = W1a[c][k] (k < 9), the bias at k = 9, split hi / lo
  half8 bwh[FUSE1A ? 2 : 1], bwl[FUSE1A ? 2 : 1];
  if constexpr (FUSE1A) {
#pragma unroll
    for (int hf = 0; hf < 2; hf++)
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int k = 8 * kl + j, c = 32 * hf + ml;
        const Half2 w = split16(k < 9 ? a.w1a[c * 9 + k] : (k == 9 ? a.b1a[c] : 0.f));
        bwh[hf][j] = w.hi;
        bwl[hf][j] = w.lo;
      }
  }
  fetch(0);
  for (int c0 = 0; c0 < CIN; c0 += XCK) {
    __syncthreads();
    if constexpr (FUSE1A) {
      // conv1a -> ReLU for channels c0 .. c0 + 15 of the halo: the transposed product D[c][px] =
      // W1a[c][k] P[k][px] of the 32-channel half holding them (lane (px, kl) gets channels 8 q + 4 kl + e;
      // this stage keeps q = 2 (c0 % 32 / 16), + 1), three products per MFMA step
      const int hf = (c0 % 64) / 32, q0 = 2 * ((c0 % 32) / 16);
      const int hx = ml, x = x0 - 1 + hx;
      for (int hy = wv; hy < HY; hy += 4) {
        const int y = y0 - 1 + hy;
        half8 ah, al;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int k = 8 * kl + j;
          float v = 0.f;
          if (hx < HX) v = k < 9 ? patch[(hy + k / 3) * (TW + 4) + hx + k % 3] : (k == 9 ? 1.f : 0.f);
          const Half2 p = split16(v);
          ah[j] = p.hi;
          al[j] = p.lo;
        }
        floatx16 d;
#pragma unroll
        for (int r = 0; r < 16; r++) d[r] = 0.f;
        d = mfma16(bwh[hf], ah, d);
        d = mfma16(bwh[hf], al, d);
        d = mfma16(bwl[hf], ah, d);
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        if (hx < HX) {
#pragma unroll
          for (int qq = 0; qq < 2; qq++) {
            half4 h4, l4;
#pragma unroll
            for (int e = 0; e < 4; e++) {
              const Half2 p = split16(in ? fmaxf(d[4 * (q0 + qq) + e], 0.f) : 0.f);
              h4[e] = p.hi;
              l4[e] = p.lo;
            }
            const int o = (hy * HX + hx) * XCS + 8 * qq + 4 * kl;
            *reinterpret_cast<half4*>(&halo[o]) = h4;
            *reinterpret_cast<half4*>(&halo[HALO + o]) = l4;
          }
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < HPT; r++) {
        const int i = tid + 256 * r, pl = i / HALO8, j = i % HALO8;
        if (i < 2 * HALO8) *reinterpret_cast<half8*>(&halo[pl * HALO + (j / (XCK / 8)) * XCS + 8 * (j % (XCK / 8))]) = ph[r];
      }
    }
#pragma unroll
    for (int r = 0; r < WPT; r++) {
      const int i = tid + 256 * r, pl = i / W8, j = i % W8;
      *reinterpret_cast<half8*>(&wts[pl * WTS + (j / (XCK / 8)) * XCS + 8 * (j % (XCK / 8))]) = pw[r];
    }
    __syncthreads();
    if (c0 + XCK < CIN) fetch(c0 + XCK);
#pragma unroll
    for (int kk = 0; kk < 9; kk++) {
      const int ky = kk / 3, kx = kk % 3;
      half8 ah[MT], al[MT], bh[2], bl[2];
#pragma unroll
      for (int m = 0; m < MT; m++) {
        const int ly = wv * (TH / 4) + 2 * m + (ml >> 4);
        const int o = ((ly + ky) * HX + (ml & 15) + kx) * XCS + 8 * kl;
        ah[m] = *reinterpret_cast<const half8*>(&halo[o]);
        al[m] = *reinterpret_cast<const half8*>(&halo[HALO + o]);
      }
#pragma unroll
      for (int n = 0; n < 2; n++) {
        const int o = (kk * 64 + n * 32 + ml) * XCS + 8 * kl;
        bh[n] = *reinterpret_cast<const half8*>(&wts[o]);
        bl[n] = *reinterpret_cast<const half8*>(&wts[WTS + o]);
      }
      // the three products in three sweeps over the (m, n) accumulators: consecutive MFMAs independent
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < 2; n++) acc[m][n] = mfma16(al[m], bh[n], acc[m][n]);
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < 2; n++) acc[m][n] = mfma16(ah[m], bl[n], acc[m][n]);
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < 2; n++) acc[m][n] = mfma16(ah[m], bh[n], acc[m][n]);
    }
  }

  // epilogue: bias + ReLU (+ 2x2 max-pool), split into hi / lo, staged through LDS (the weight buffer) so
  // the global stores are 16-byte rows of 8 channels
  constexpr int OPIX = POOL ? (TH / 2) * 8 : TH * 16;
  static_assert((POOL ? 2 : 1) * OPIX * OS <= 2 * WTS, "output tile exceeds the weight buffer");
  float bias[2];
#pragma unroll
  for (int n = 0; n < 2; n++) bias[n] = a.bias[co0 + n * 32 + ml];
  const int Ho = POOL ? H / 2 : H, Wo = POOL ? W / 2 : W;
  // POOL: both planes staged at once; otherwise hi, then lo (each fills most of the buffer)
#pragma unroll
  for (int pass = 0; pass < (POOL ? 1 : 2); pass++) {
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int m = 0; m < MT; m++) {
        if constexpr (POOL) {
          const int pyl = wv * (TH / 8) + m;
#pragma unroll
          for (int g = 0; g < 4; g++) {
            const int r0 = (g & 1) * 2 + (g >> 1) * 4;
            const int pc = (r0 & 3) + 8 * ((r0 >> 2) & 1) + 4 * kl;
            float v = fmaxf(fmaxf(acc[m][n][r0], acc[m][n][r0 + 1]), fmaxf(acc[m][n][r0 + 8], acc[m][n][r0 + 9]));
            v += bias[n];
            const Half2 p = split16(v > 0.f ? v : 0.f);
            const int o = (pyl * 8 + (pc >> 1)) * OS + n * 32 + ml;
            wts[o] = p.hi;
            wts[OPIX * OS + o] = p.lo;
          }
        } else {
          const int ly = wv * (TH / 4) + 2 * m;
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int mm = (r & 3) + 8 * (r >> 2) + 4 * kl;
            const float v = acc[m][n][r] + bias[n];
            const Half2 p = split16(v > 0.f ? v : 0.f);
            wts[((ly + (mm >> 4)) * 16 + (mm & 15)) * OS + n * 32 + ml] = pass ? p.lo : p.hi;
          }
        }
      }
    __syncthreads();
#pragma unroll
    for (int pl = 0; pl < (POOL ? 2 : 1); pl++) {
      _Float16* out = (POOL ? (pl ? a.hout_lo : a.hout) : (pass ? a.hout_lo : a.hout)) + (size_t)bi * Ho * Wo * COUT;
      for (int i = tid; i < OPIX * 8; i += 256) {
        const int px = i >> 3, q = i & 7;
        const int y = POOL ? (y0 >> 1) + (px >> 3) : y0 + (px >> 4);
        const int x = POOL ? (x0 >> 1) + (px & 7) : x0 + (px & 15);
        if (y < Ho && x < Wo)
          *reinterpret_cast<half8*>(out + ((size_t)y * Wo + x) * COUT + co0 + 8 * q) =
              *reinterpret_cast<const half8*>(&wts[pl * OPIX * OS + px * OS + 8 * q]);
      }
    }
  }
}

template <int CIN, int TH, bool POOL, bool FUSE1A>
static hipError_t launch_conv_x3(const ConvArgs& a, int B, hipStream_t s, hipEvent_t t0 = nullptr,
                                 hipEvent_t t1 = nullptr) {
  const int tiles = ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
  dim3 grid(B * tiles, a.cout / 64);
  hipExtLaunchKernelGGL((conv3x3_x3_kernel<CIN, TH, POOL, FUSE1A>), grid, dim3(256), 0, s, t0, t1, 0, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// host entry points: (cin, pool, level size) -> the <CIN, TH, POOL> instance, for every precision
// ---------------------------------------------------------------------------
template <int CIN_, int TH_, bool POOL_>
struct ConvShape {
  static constexpr int CIN = CIN_, TH = TH_;
  static constexpr bool POOL = POOL_;
};

// launch(ConvShape<..>{}) starts the caller's kernel of that shape
template <typename Launch>
static hipError_t dispatch_conv(const ConvArgs& a, int cin, bool pool, Launch&& launch) {
  const bool small = (a.H * a.W) <= 128 * 192;  // more, smaller tiles for the low-res layers
  if (cin == 64 && pool) return launch(ConvShape<64, 16, true>{});
  if (cin == 64 && !pool) return small ? launch(ConvShape<64, 8, false>{}) : launch(ConvShape<64, 16, false>{});
  if (cin == 128 && pool) return launch(ConvShape<128, 16, true>{});
  if (cin == 128 && !pool) return small ? launch(ConvShape<128, 8, false>{}) : launch(ConvShape<128, 16, false>{});
  return hipErrorInvalidValue;
}

hipError_t conv3x3(const ConvArgs& a, int cin, bool pool, bool fuse1a, int B, hipStream_t s, hipEvent_t t0,
                   hipEvent_t t1) {
  if (fuse1a) return launch_conv<64, 16, true, true>(a, B, s, t0, t1);
  return dispatch_conv(a, cin, pool, [&](auto sh) {
    return launch_conv<decltype(sh)::CIN, decltype(sh)::TH, decltype(sh)::POOL, false>(a, B, s);
  });
}

hipError_t conv3x3_h(const ConvArgs& a, int cin, bool pool, bool fuse1a, int B, hipStream_t s, hipEvent_t t0,
                     hipEvent_t t1) {
  if (fuse1a) return launch_conv1_res(a, B, s, t0, t1);
  return dispatch_conv(a, cin, pool, [&](auto sh) {
    return launch_conv_h<decltype(sh)::CIN, decltype(sh)::TH, decltype(sh)::POOL>(a, B, s);
  });
}

hipError_t conv3x3_x3(const ConvArgs& a, int cin, bool pool, bool fuse1a, int B, hipStream_t s, hipEvent_t t0,
                      hipEvent_t t1) {
  if (fuse1a) return launch_conv_x3<64, 16, true, true>(a, B, s, t0, t1);
  return dispatch_conv(a, cin, pool, [&](auto sh) {
    return launch_conv_x3<decltype(sh)::CIN, decltype(sh)::TH, decltype(sh)::POOL, false>(a, B, s);
  });
}

}  // namespace sp
}  // namespace rspl
