// SuperPoint heads and descriptor sampling on gfx950 (CDNA4): the 1x1 detector / descriptor heads of the three
// precisions and the bilinear descriptor samplers that pack the 259-double feature records.
//
// Reference semantics:
//   network  convert2onnx/superpoint.py:130-135, 159-161  (detector & descriptor heads)
//   host     src/super_point.cpp:206-319                  (bilinear sampling in double, packing)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sp_device.hpp"
#include "sp_kernels.hpp"

namespace rspl {
namespace sp {

// ---------------------------------------------------------------------------
// 1x1 heads on the H/8 x W/8 cell grid.  in = [P][512] (convPa | convDa, ReLU'd).
//   MODE 0: convPb 256->65, softmax over 65, drop dustbin, depth-to-space ->
//           scores [H][W]  (superpoint.py:131-135)
//   MODE 1: convDb 256->256, per-cell L2 normalise -> desc [P][256]
//           (superpoint.py:160-161)
// One wave owns 32 cells; block = 4 waves = 128 cells.  K = 256 staged in LDS
// in chunks of 32.  Weights pre-transposed to [256][NPAD] (NPAD = 96 / 256).
// ---------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void head_kernel(HeadArgs a) {
  constexpr int NT = MODE == 0 ? 3 : 8;  // N-tiles of 32
  constexpr int NP = NT * 32;
  constexpr int KC = 32;
  __shared__ float As[KC][128 + 1];
  __shared__ float Bs[KC][NP];
  const int P = a.P;  // cells per image
  const int cell0 = blockIdx.x * 128;  // flattened over batch
  const int total = a.B * P;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ml = lane & 31, kl = lane >> 5;
  const int in_off = MODE == 0 ? 0 : 256;

  floatx16 acc[NT];
  zero(acc);

  for (int k0 = 0; k0 < 256; k0 += KC) {
    __syncthreads();
    for (int i = tid; i < 128 * (KC / 4); i += 256) {
      const int q = i % (KC / 4), c = i / (KC / 4);
      const int cell = cell0 + c;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cell < total) v = *reinterpret_cast<const float4*>(a.in + (size_t)cell * 512 + in_off + k0 + 4 * q);
      As[4 * q + 0][c] = v.x; As[4 * q + 1][c] = v.y; As[4 * q + 2][c] = v.z; As[4 * q + 3][c] = v.w;
    }
    for (int i = tid; i < KC * (NP / 4); i += 256) {
      const int q = i % (NP / 4), k = i / (NP / 4);
      *reinterpret_cast<float4*>(&Bs[k][4 * q]) = *reinterpret_cast<const float4*>(a.w + (size_t)(k0 + k) * NP + 4 * q);
    }
    __syncthreads();
#pragma unroll 4
    for (int kc = 0; kc < KC; kc += 2) {
      const float av = As[kc + kl][wv * 32 + ml];
#pragma unroll
      for (int n = 0; n < NT; n++) acc[n] = mfma32(av, Bs[kc + kl][n * 32 + ml], acc[n]);
    }
  }

  // epilogue: rows (cells) on registers, channels on lanes (col = ml within N-tile)
#pragma unroll
  for (int n = 0; n < NT; n++) {
    const float b = a.bias[n * 32 + ml];
#pragma unroll
    for (int r = 0; r < 16; r++) acc[n][r] += b;
  }
  if constexpr (MODE == 0) {
    // channels >= 65 are padding: exclude from the softmax
#pragma unroll
    for (int r = 0; r < 16; r++) {
      // (not softmax65_row() / acc_row(): with them this kernel is rescheduled and its stage ran 0.2 % slower than
      // the parent's slowest run)
      float m = -INFINITY;
#pragma unroll
      for (int n = 0; n < NT; n++) {
        const int c = n * 32 + ml;
        if (c < 65) m = fmaxf(m, acc[n][r]);
      }
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 32));
      float e[NT];
      float s = 0.f;
#pragma unroll
      for (int n = 0; n < NT; n++) {
        const int c = n * 32 + ml;
        e[n] = (c < 65) ? expf(acc[n][r] - m) : 0.f;
        s += e[n];
      }
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o, 32);
      const int cell = cell0 + wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
      if (cell < total) {
        const int bi = cell / P, p = cell % P;
        const int cy = p / a.W8, cx = p % a.W8;
        float* sc = a.scores + (size_t)bi * P * 64;
        const int Wf = a.W8 * 8;
#pragma unroll
        for (int n = 0; n < 2; n++) {  // channels 0..63 live in N-tiles 0,1
          const int c = n * 32 + ml;
          sc[(size_t)(cy * 8 + (c >> 3)) * Wf + cx * 8 + (c & 7)] = e[n] / s;
        }
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      float s = 0.f;
#pragma unroll
      for (int n = 0; n < NT; n++) s += acc[n][r] * acc[n][r];
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o, 32);
      float nrm = sqrtf(s);
      nrm = nrm < 1e-12f ? 1e-12f : nrm;
      const int cell = cell0 + wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
      if (cell < total) {
#pragma unroll
        for (int n = 0; n < NT; n++) a.desc[(size_t)cell * 256 + n * 32 + ml] = acc[n][r] / nrm;
      }
    }
  }
}

hipError_t heads(const HeadArgs& a, int mode, hipStream_t s) {
  const int blocks = (a.B * a.P + 127) / 128;
  if (mode == 0)
    hipLaunchKernelGGL(head_kernel<0>, dim3(blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(head_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// RSPL_PREC_FP16 heads.  The fp16 convPa | convDa map ([P][512] halves) is read straight into
// v_mfma_f32_32x32x16_f16 A operands (lane (r, h): cell r, channels 16t + 8h .. +7); the 1x1
// weights come from L2 in B-fragment order, so neither head stages anything through LDS.
//   det_head_h:    convPb 256->65, softmax over 65, dustbin dropped, depth-to-space
//                  (superpoint.py:131-135); one wave per 32 cells.
//   sample_taps_h: convDb 256->256 + per-cell L2 normalise (superpoint.py:160-161) evaluated
//                  only at the 4 bilinear taps of each selected keypoint (the dense map is never
//                  formed: the 1x1 conv and the per-cell normalise are pointwise, so this is the
//                  same function), then the double-precision bilinear sample and renormalise of
//                  src/super_point.cpp:206-319.  A workgroup takes 8 keypoints = 32 tap rows
//                  (one M-tile); wave w owns output channels 64w .. 64w+63.
// ---------------------------------------------------------------------------
// X3 (RSPL_PREC_FP16X3): cells and weights as hi + lo fp16 planes, three products per MFMA step (the split
// arithmetic of conv3x3_x3_kernel)
template <bool X3>
__global__ __launch_bounds__(256) void det_head_h_kernel(HeadHArgs a) {
  constexpr int NT = 3;  // 96 columns, 65 real
  const int total = a.B * a.P;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ml = lane & 31, kl = lane >> 5;
  const int base = (blockIdx.x * 4 + wv) * 32;
  if (base >= total) return;  // per wave: no barriers below
  const size_t ro = (size_t)min(base + ml, total - 1) * 512 + 8 * kl;
  half8 av[16], al[X3 ? 16 : 1];
#pragma unroll
  for (int t = 0; t < 16; t++) av[t] = *reinterpret_cast<const half8*>(a.cells + ro + 16 * t);
  if constexpr (X3)
#pragma unroll
    for (int t = 0; t < 16; t++) al[t] = *reinterpret_cast<const half8*>(a.cells_lo + ro + 16 * t);
  floatx16 acc[NT];
  zero(acc);
  const half8* wf = reinterpret_cast<const half8*>(a.wPb) + lane;
  const half8* wfl = reinterpret_cast<const half8*>(a.wPb_lo) + lane;
#pragma unroll
  for (int t = 0; t < 16; t++) {
    half8 bv[NT], bl[X3 ? NT : 1];
#pragma unroll
    for (int n = 0; n < NT; n++) bv[n] = wf[(n * 16 + t) * 64];
    if constexpr (X3)
#pragma unroll
      for (int n = 0; n < NT; n++) bl[n] = wfl[(n * 16 + t) * 64];
    if constexpr (X3) {
#pragma unroll
      for (int n = 0; n < NT; n++) acc[n] = mfma16(al[t], bv[n], acc[n]);
#pragma unroll
      for (int n = 0; n < NT; n++) acc[n] = mfma16(av[t], bl[n], acc[n]);
    }
#pragma unroll
    for (int n = 0; n < NT; n++) acc[n] = mfma16(av[t], bv[n], acc[n]);
  }
#pragma unroll
  for (int n = 0; n < NT; n++) {
    const float b = a.bPb[n * 32 + ml];
#pragma unroll
    for (int r = 0; r < 16; r++) acc[n][r] += b;
  }
  const int Wf = a.W8 * 8;
  // the wave's 32 cells x 64 scores go through LDS, then out as rows of the full-resolution map
  // (lanes = consecutive cells of one pixel row: 32-byte pieces side by side) instead of 4-byte
  // scatters into 8 rows per cell
  __shared__ __attribute__((aligned(16))) float stage[4][32][65];
  float(*sg)[65] = stage[wv];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    float e[NT];
    const float sum = softmax65_row(acc, r, ml, e);
    const int cl = acc_row(r, kl);
#pragma unroll
    for (int n = 0; n < 2; n++) sg[cl][n * 32 + ml] = e[n] / sum;  // channels 0..63 (dustbin dropped)
  }
  __builtin_amdgcn_wave_barrier();  // LDS in program order within the wave
  for (int i = lane; i < 32 * 8 * 2; i += 64) {  // (pixel row pr, cell j, half h): 4 floats each
    const int pr = i >> 6, j = (i >> 1) & 31, hh = i & 1;
    const int cell = base + j;
    if (cell >= total) continue;
    const int bi = cell / a.P, p = cell % a.P;
    const int cy = p / a.W8, cx = p % a.W8;
    const float* src = &sg[j][pr * 8 + 4 * hh];
    *reinterpret_cast<float4*>(a.scores + (size_t)bi * a.P * 64 + (size_t)(cy * 8 + pr) * Wf + cx * 8 + 4 * hh) =
        make_float4(src[0], src[1], src[2], src[3]);
  }
}

hipError_t det_head_h(const HeadHArgs& a, bool x3, hipStream_t s) {
  const int blocks = (a.B * a.P + 127) / 128;
  if (x3) hipLaunchKernelGGL(det_head_h_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(det_head_h_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

template <bool X3>
__global__ __launch_bounds__(256) void sample_taps_h_kernel(TapArgs a) {
  __shared__ int tcell[32];      // tap row 4 kp + q: cell of tap q (nw, ne, sw, se) of keypoint kp
  __shared__ double twt[32];     // its bilinear weight
  __shared__ float part[4][32];  // per-wave partial sums of squares per tap row
  __shared__ double part2[4][8]; // per-wave partial sums of squares per keypoint
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ml = lane & 31, kl = lane >> 5;
  const int bpi = (a.per_image + 7) / 8;
  const int bi = blockIdx.x / bpi, i0 = (blockIdx.x % bpi) * 8;
  if (bi >= a.B) return;
  const int n = a.sel_count[bi];
  if (tid == 0 && i0 == 0) a.counts[bi] = n;
  if (i0 >= n) return;  // uniform over the workgroup
  const int H = a.H, W = a.W, h = H / 8, w = W / 8, P = h * w;
  if (tid < 8) {
    const int i = i0 + tid;
    BilinearTaps t = {};
    if (i < n) {
      const unsigned flat = a.sel[(size_t)bi * a.sel_stride + i];
      const int y = flat / W, x = flat % W;
      t = bilinear_taps(x, y, h, w);
      double* f = a.features + ((size_t)bi * a.feat_cap + i) * 259;
      f[0] = (double)a.nms[(size_t)bi * H * W + flat];
      f[1] = (double)x;
      f[2] = (double)y;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      tcell[4 * tid + q] = t.iy[q] * w + t.ix[q];
      twt[4 * tid + q] = t.wt[q];
    }
  }
  __syncthreads();
  const size_t ro = ((size_t)bi * P + tcell[ml]) * 512 + 256 + 8 * kl;
  half8 av[16], al[X3 ? 16 : 1];
#pragma unroll
  for (int t = 0; t < 16; t++) av[t] = *reinterpret_cast<const half8*>(a.cells + ro + 16 * t);
  if constexpr (X3)
#pragma unroll
    for (int t = 0; t < 16; t++) al[t] = *reinterpret_cast<const half8*>(a.cells_lo + ro + 16 * t);
  floatx16 acc[2];
  zero(acc);
  const half8* wf = reinterpret_cast<const half8*>(a.wDb) + lane;
  const half8* wfl = reinterpret_cast<const half8*>(a.wDb_lo) + lane;
#pragma unroll
  for (int t = 0; t < 16; t++) {
    const half8 b0 = wf[((2 * wv) * 16 + t) * 64], b1 = wf[((2 * wv + 1) * 16 + t) * 64];
    if constexpr (X3) {
      const half8 l0 = wfl[((2 * wv) * 16 + t) * 64], l1 = wfl[((2 * wv + 1) * 16 + t) * 64];
      acc[0] = mfma16(al[t], b0, acc[0]);
      acc[1] = mfma16(al[t], b1, acc[1]);
      acc[0] = mfma16(av[t], l0, acc[0]);
      acc[1] = mfma16(av[t], l1, acc[1]);
    }
    acc[0] = mfma16(av[t], b0, acc[0]);
    acc[1] = mfma16(av[t], b1, acc[1]);
  }
  // bias; per tap row (register r, lane half kl: row (r & 3) + 8 (r >> 2) + 4 kl) the sum of
  // squares over this wave's 64 channels, then over the 4 waves in a fixed order
  const float bias0 = a.bDb[64 * wv + ml], bias1 = a.bDb[64 * wv + 32 + ml];
  float ss[16];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    acc[0][r] += bias0;
    acc[1][r] += bias1;
    ss[r] = acc[0][r] * acc[0][r] + acc[1][r] * acc[1][r];
  }
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1)
#pragma unroll
    for (int r = 0; r < 16; r++) ss[r] += __shfl_xor(ss[r], o, 32);
  if (ml == 0)
#pragma unroll
    for (int r = 0; r < 16; r++) part[wv][acc_row(r, kl)] = ss[r];
  __syncthreads();
  // keypoint kp = 2 q + kl holds its taps in registers 4q .. 4q+3 (nw, ne, sw, se)
  double v[4][2], s2[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int kp = 2 * q + kl;
    double vv0 = 0, vv1 = 0;
#pragma unroll
    for (int tp = 0; tp < 4; tp++) {
      const int rw = 4 * kp + tp;
      float nrm = sqrtf(((part[0][rw] + part[1][rw]) + part[2][rw]) + part[3][rw]);
      nrm = nrm < 1e-12f ? 1e-12f : nrm;
      const double wt = twt[rw];
      vv0 += (double)(acc[0][4 * q + tp] / nrm) * wt;
      vv1 += (double)(acc[1][4 * q + tp] / nrm) * wt;
    }
    v[q][0] = vv0;
    v[q][1] = vv1;
    s2[q] = vv0 * vv0 + vv1 * vv1;
  }
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1)
#pragma unroll
    for (int q = 0; q < 4; q++) s2[q] += __shfl_xor(s2[q], o, 32);
  if (ml == 0)
#pragma unroll
    for (int q = 0; q < 4; q++) part2[wv][2 * q + kl] = s2[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int kp = 2 * q + kl, i = i0 + kp;
    if (i >= n) continue;
    const double inv = 1.0 / sqrt(((part2[0][kp] + part2[1][kp]) + part2[2][kp]) + part2[3][kp]);
    double* f = a.features + ((size_t)bi * a.feat_cap + i) * 259 + 3 + 64 * wv + ml;
    f[0] = inv * v[q][0];
    f[32] = inv * v[q][1];
  }
}

hipError_t sample_taps_h(const TapArgs& a, bool x3, hipStream_t s) {
  const int blocks = a.B * ((a.per_image + 7) / 8);
  if (x3) hipLaunchKernelGGL(sample_taps_h_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(sample_taps_h_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Descriptor sampling + packing (src/super_point.cpp:206-319), fp64.
// One wave per keypoint, 4 channels per lane.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_kernel(SampleArgs a) {
  const int wv = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int bi = wv / a.per_image, i = wv % a.per_image;
  if (bi >= a.B) return;
  const int n = a.sel_count[bi];
  if (lane == 0 && i == 0) a.counts[bi] = n;
  if (i >= n) return;
  const int H = a.H, W = a.W, h = H / 8, w = W / 8;
  const unsigned flat = a.sel[(size_t)bi * a.sel_stride + i];
  const int y = flat / W, x = flat % W;
  const float score = a.nms[(size_t)bi * H * W + flat];
  const BilinearTaps t = bilinear_taps(x, y, h, w);
  const double nw = t.wt[0], ne = t.wt[1], sw = t.wt[2], se = t.wt[3];
  const float* d = a.desc + (size_t)bi * h * w * 256;
  const float4 vnw = *reinterpret_cast<const float4*>(d + ((size_t)t.iy[0] * w + t.ix[0]) * 256 + 4 * lane);
  const float4 vne = *reinterpret_cast<const float4*>(d + ((size_t)t.iy[1] * w + t.ix[1]) * 256 + 4 * lane);
  const float4 vsw = *reinterpret_cast<const float4*>(d + ((size_t)t.iy[2] * w + t.ix[2]) * 256 + 4 * lane);
  const float4 vse = *reinterpret_cast<const float4*>(d + ((size_t)t.iy[3] * w + t.ix[3]) * 256 + 4 * lane);
  double v[4];
  v[0] = (double)vnw.x * nw + (double)vne.x * ne + (double)vsw.x * sw + (double)vse.x * se;
  v[1] = (double)vnw.y * nw + (double)vne.y * ne + (double)vsw.y * sw + (double)vse.y * se;
  v[2] = (double)vnw.z * nw + (double)vne.z * ne + (double)vsw.z * sw + (double)vse.z * se;
  v[3] = (double)vnw.w * nw + (double)vne.w * ne + (double)vsw.w * sw + (double)vse.w * se;
  double ss = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const double inv = 1.0 / sqrt(ss);
  double* f = a.features + ((size_t)bi * a.feat_cap + i) * 259;
  if (lane == 0) {
    f[0] = (double)score;
    f[1] = (double)x;
    f[2] = (double)y;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) f[3 + 4 * lane + j] = inv * v[j];
}

hipError_t sample(const SampleArgs& a, hipStream_t s) {
  const int waves = a.B * a.per_image;
  hipLaunchKernelGGL(sample_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sp
}  // namespace rspl
