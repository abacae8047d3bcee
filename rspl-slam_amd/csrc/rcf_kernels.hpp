// RCF edge network on gfx950: host-facing interface of rcf_conv.hip (3x3 convolutions, the one-channel first
// layer, max-pool) and rcf_side.hip (1x1 side branches, upsampling + fuse + edge image).
// Network: the VGG16-based RCF (yun-liu/RCF-PyTorch) behind RCF::infer (src/rcf.cpp:95-135).
// Layout: activations NHWC, fp32 (RSPL_PREC_FP32) or fp16 (RSPL_PREC_FP16); side maps and logits fp32.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rspl {
namespace rcf {

constexpr int kSide = 21;     // channels of a side branch (convS_K_down)
constexpr int kSideRows = 32; // its weight rows: the MFMA tile's 32, rows 21.. zero
constexpr int kSidePad = 24;  // floats per pixel of a stage's summed side map
constexpr int kStages = 5;

// conv1_1: u8 image (raw 0..255, three identical channels folded into the weights) -> 64 channels, ReLU
struct FirstArgs {
  const uint8_t* img;
  size_t stride, pitch;
  const float* w;     // [9][64] (fp16 path: the fp16-rounded weights, held as floats)
  const float* bias;  // [64]
  void* out;          // NHWC [B][H][W][64], float or _Float16
  int H, W, B;
};

// 3x3 conv, pad = dilation, bias + ReLU, as an implicit GEMM (M = pixels, N = cout, K = 9 * cin)
struct ConvArgs {
  const void* in;     // NHWC [B][H][W][cin]
  const void* w;      // fp32: [9][cin][cout] floats; fp16: [9][cout][cin] halves
  const float* bias;  // [cout]
  void* out;          // NHWC [B][H][W][cout]
  int H, W, B;
  int cin, cout;      // fp32: cin % 16 == 0; fp16: cin % 32 == 0; cout % 64 == 0
  int dilation;       // 1 or 2
  int tile_rows;      // 8 or 16 rows per workgroup tile; 0: chosen from the launch's size
};

// 2x2 max-pool, stride 2 or 1, ceil_mode: a last odd row / column pools alone
struct PoolArgs {
  const void* in;  // NHWC [B][H][W][C]
  void* out;       // NHWC [B][Ho][Wo][C]
  int H, W, Ho, Wo, B, C, stride;
};

// side branch of one conv: acc (+)= act x down^T + bias (1x1, C -> 21); on a stage's last conv also
// so = score_dsn(acc) (1x1, 21 -> 1)
struct SideArgs {
  const void* act;    // NHWC [npix][C]
  const void* w;      // [32][C], float or _Float16, rows 21.. zero
  const float* bias;  // [32], 21.. zero
  float* acc;         // [npix][kSidePad]
  const float* dsn_w; // [32], 21.. zero
  float dsn_b;
  float* so;          // [npix]
  size_t npix;
  int C;
  int first, last;    // first conv of the stage: acc is written, not added to
};

// one thread per output pixel: the four bilinear transposed convs with their crops, score_fuse, the
// six logits, the sigmoid of map `output` and the u8 edge value
struct TailArgs {
  const float* so[kStages];  // [B][Hs][Ws]
  int Hs[kStages], Ws[kStages];
  float fuse_w[kStages], fuse_b;
  float* logits;   // [B][6][H][W]
  uint8_t* edges;
  size_t out_stride, out_pitch;
  int H, W, B, output;
};

hipError_t first_conv(const FirstArgs& a, bool half, hipStream_t s);
hipError_t conv3x3(const ConvArgs& a, bool half, hipStream_t s);
hipError_t pool(const PoolArgs& a, bool half, hipStream_t s);
hipError_t side(const SideArgs& a, bool half, hipStream_t s);
hipError_t tail(const TailArgs& a, hipStream_t s);

}  // namespace rcf
}  // namespace rspl
