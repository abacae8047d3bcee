// SuperGlue GEMMs on gfx950 (CDNA4): the fp32 MFMA GEMMs, their fp16 counterparts (RSPL_PREC_FP16) and the
// one-time weight re-layouts.  Each kernel is followed by its host launcher.
// Layout: token-major.  Token t = (pair*2 + image)*nmax + i; descriptors X[t][256].
#include <hip/hip_runtime.h>

#include "sg_device.hpp"
#include "sg_kernels.hpp"

namespace rspl {
namespace sg {

// ---------------------------------------------------------------------------
// Generic fp32 MFMA GEMM: 64x64 tile, BK = 32, 4 waves (2x2) of 32x32 each.
// Double-buffered LDS with a register prefetch of the next K tile issued before
// the 16 MFMAs of the current one: one barrier per K step, load latency hidden.
// ---------------------------------------------------------------------------
template <int EPI, bool BNT>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs a) {
  __shared__ float As[2][32][64 + 4];
  __shared__ float Bs[2][32][64 + 4];
  const int z = blockIdx.z;
  int M = a.M, N = a.N;
  if (a.mcount) M = a.mcount[(size_t)z * a.count_stride];
  if (a.ncount) N = a.ncount[(size_t)z * a.count_stride];
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  if (m0 >= M || n0 >= N) return;
  const float* A = a.A + z * a.sA;
  const float* A2 = a.A2 ? a.A2 + z * a.sA : nullptr;
  const float* B = a.B + z * a.sB;
  float* C = a.C + z * a.sC;
  const int K = a.K;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ml = lane & 31, kl = lane >> 5;
  const int wm = wv >> 1, wn = wv & 1;
  // loader coordinates: A / B^T tiles 64 x 32 (row = tid>>3 (+32), k4 = (tid&7)*4),
  // B tile 32 x 64 (k = tid>>4 (+16), n4 = (tid&15)*4)
  const int lr = tid >> 3, lk4 = (tid & 7) * 4;
  const int bk = tid >> 4, bn4 = (tid & 15) * 4;
  float4 ra[2], rb[2];
  auto load = [&](int k0) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int m = m0 + lr + 32 * h, k = k0 + lk4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < M && k < K) {
        const float* src = (A2 && k >= a.ksplit) ? A2 + (size_t)m * a.lda + (k - a.ksplit) : A + (size_t)m * a.lda + k;
        v = *reinterpret_cast<const float4*>(src);
      }
      ra[h] = v;
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (!BNT) {
        const int k = k0 + bk + 16 * h;
        if (k < K && n0 + bn4 < N) v = *reinterpret_cast<const float4*>(B + (size_t)k * a.ldb + n0 + bn4);
      } else {
        const int n = n0 + lr + 32 * h, k = k0 + lk4;
        if (n < N && k < K) v = *reinterpret_cast<const float4*>(B + (size_t)n * a.ldb + k);
      }
      rb[h] = v;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int r = lr + 32 * h;
      As[buf][lk4 + 0][r] = ra[h].x; As[buf][lk4 + 1][r] = ra[h].y;
      As[buf][lk4 + 2][r] = ra[h].z; As[buf][lk4 + 3][r] = ra[h].w;
      if constexpr (!BNT) {
        *reinterpret_cast<float4*>(&Bs[buf][bk + 16 * h][bn4]) = rb[h];
      } else {
        Bs[buf][lk4 + 0][r] = rb[h].x; Bs[buf][lk4 + 1][r] = rb[h].y;
        Bs[buf][lk4 + 2][r] = rb[h].z; Bs[buf][lk4 + 3][r] = rb[h].w;
      }
    }
  };
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  const int nk = (K + 31) / 32;
  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt++) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load((kt + 1) * 32);
#pragma unroll
    for (int kk = 0; kk < 32; kk += 2)
      acc = mfma32(As[buf][kk + kl][wm * 32 + ml], Bs[buf][kk + kl][wn * 32 + ml], acc);
    if (kt + 1 < nk) store(buf ^ 1);
    __syncthreads();
  }
  const int n = n0 + wn * 32 + ml;
  if (n >= N) return;
  const float b = a.bias ? a.bias[n] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
    if (m < M) {
      float v = acc[r] * a.alpha + b;
      float* dst = C + (size_t)m * a.ldc + n;
      if constexpr (EPI == 1) v = v > 0.f ? v : 0.f;
      if constexpr (EPI == 2) v = *dst + v;
      *dst = v;
    }
  }
}

// ---------------------------------------------------------------------------
// Split-K fp32 MFMA GEMM for the token-parallel layers (M = tokens ~ 1600 is too
// short for 64x64 tiles to fill 256 CUs): one 32x32 output tile per workgroup, the
// 4 waves take interleaved quarters of K (32-wide steps), each with a register
// prefetch into a wave-private LDS slot (no block barriers in the K loop).  The 4
// partial tiles are summed in a fixed order (w0+w1+w2+w3): deterministic.
// ---------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256) void gemm_sk_kernel(GemmArgs a) {
  __shared__ float As[4][32][33];  // [wave][k][m]
  __shared__ float Bs[4][32][33];  // [wave][k][n]
  const int z = blockIdx.z;
  int M = a.M, N = a.N;
  if (a.mcount) M = a.mcount[(size_t)z * a.count_stride];
  if (a.ncount) N = a.ncount[(size_t)z * a.count_stride];
  const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  if (m0 >= M || n0 >= N) return;
  const float* A = a.A + z * a.sA;
  const float* A2 = a.A2 ? a.A2 + z * a.sA : nullptr;
  const float* B = a.B + z * a.sB;
  float* C = a.C + z * a.sC;
  const int K = a.K, nsteps = (K + 31) / 32;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ml = lane & 31, kl = lane >> 5;
  float4 ra[4], rb[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = lane + 64 * u, r = i >> 3, c4 = (i & 7) * 4;
      const int m = m0 + r, ka = k0 + c4, kb = k0 + r, n = n0 + c4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f), w = v;
      if (m < M && ka < K) {
        const float* src = (A2 && ka >= a.ksplit) ? A2 + (size_t)m * a.lda + (ka - a.ksplit) : A + (size_t)m * a.lda + ka;
        v = *reinterpret_cast<const float4*>(src);
      }
      if (kb < K && n < N) w = *reinterpret_cast<const float4*>(B + (size_t)kb * a.ldb + n);
      ra[u] = v;
      rb[u] = w;
    }
  };
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  int step = wv;
  if (step < nsteps) load(step * 32);
  for (; step < nsteps; step += 4) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = lane + 64 * u, r = i >> 3, c4 = (i & 7) * 4;
      As[wv][c4 + 0][r] = ra[u].x; As[wv][c4 + 1][r] = ra[u].y;
      As[wv][c4 + 2][r] = ra[u].z; As[wv][c4 + 3][r] = ra[u].w;
      Bs[wv][r][c4 + 0] = rb[u].x; Bs[wv][r][c4 + 1] = rb[u].y;
      Bs[wv][r][c4 + 2] = rb[u].z; Bs[wv][r][c4 + 3] = rb[u].w;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    if (step + 4 < nsteps) load((step + 4) * 32);
#pragma unroll
    for (int kk = 0; kk < 32; kk += 2) acc = mfma32(As[wv][kk + kl][ml], Bs[wv][kk + kl][ml], acc);
  }
  // fixed-order reduction of the 4 K-partials through LDS (reuses As/Bs: 4 x 1056 >= 3 x 16 x 64)
  __syncthreads();
  float* red = &As[0][0][0];
  if (wv > 0) {
#pragma unroll
    for (int r = 0; r < 16; r++) red[((wv - 1) * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wv != 0) return;
  const int n = n0 + ml;
  if (n >= N) return;
  const float b = a.bias ? a.bias[n] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const float s = ((acc[r] + red[(0 * 16 + r) * 64 + lane]) + red[(1 * 16 + r) * 64 + lane]) +
                    red[(2 * 16 + r) * 64 + lane];
    const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kl;
    if (m < M) {
      float v = s * a.alpha + b;
      float* dst = C + (size_t)m * a.ldc + n;
      if constexpr (EPI == 1) v = v > 0.f ? v : 0.f;
      if constexpr (EPI == 2) v = *dst + v;
      *dst = v;
    }
  }
}

// ---------------------------------------------------------------------------
// RSPL_PREC_FP16 GEMM (the reference's TensorRT kFP16 SuperGlue engine,
// super_glue.cpp:132): v_mfma_f32_32x32x16_f16, fp32 accumulation and epilogue.
// Lane (r, h) operand fragments come straight from global memory: A = 8 consecutive
// fp32 activations of row m0+r converted to fp16, B = 8 consecutive fp16 weights of
// row n0+r of the transposed weight.  Same 32x32 tile / 4-way K split / fixed-order
// LDS reduction as gemm_sk_kernel; four 16-wide K steps in flight per wave.
// ---------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256) void gemm_h_kernel(GemmArgs a) {
  __shared__ float red[3 * 16 * 64];
  const int z = blockIdx.z;
  int M = a.M, N = a.N;
  if (a.mcount) M = a.mcount[(size_t)z * a.count_stride];
  if (a.ncount) N = a.ncount[(size_t)z * a.count_stride];
  const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  if (m0 >= M || n0 >= N) return;
  const float* A = a.A + z * a.sA;
  const float* A2 = a.A2 ? a.A2 + z * a.sA : nullptr;
  float* C = a.C + z * a.sC;
  const int K = a.K, nsteps = K / 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ml = lane & 31, kl = lane >> 5;
  const int m = m0 + ml, n = n0 + ml;
  const bool mok = m < M, nok = n < N;
  const _Float16* Brow = a.hB + (size_t)(nok ? n : 0) * a.ldbh + 8 * kl;
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  auto afrag = [&](int k0) {
    const int k = k0 + 8 * kl;
    half8 h = {};
    if (mok) {
      const float* src = (A2 && k >= a.ksplit) ? A2 + (size_t)m * a.lda + (k - a.ksplit) : A + (size_t)m * a.lda + k;
      const float4 u = *reinterpret_cast<const float4*>(src), v = *reinterpret_cast<const float4*>(src + 4);
      h[0] = (_Float16)u.x; h[1] = (_Float16)u.y; h[2] = (_Float16)u.z; h[3] = (_Float16)u.w;
      h[4] = (_Float16)v.x; h[5] = (_Float16)v.y; h[6] = (_Float16)v.z; h[7] = (_Float16)v.w;
    }
    return h;
  };
  auto bfrag = [&](int k0) {
    half8 h = {};
    if (nok) h = *reinterpret_cast<const half8*>(Brow + k0);
    return h;
  };
  int step = wv;
  for (; step + 12 < nsteps; step += 16) {  // 4 steps per wave in flight
    half8 av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      av[u] = afrag((step + 4 * u) * 16);
      bv[u] = bfrag((step + 4 * u) * 16);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) acc = mfma16(av[u], bv[u], acc);
  }
  for (; step < nsteps; step += 4) acc = mfma16(afrag(step * 16), bfrag(step * 16), acc);
  if (wv > 0) {
#pragma unroll
    for (int r = 0; r < 16; r++) red[((wv - 1) * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wv != 0 || !nok) return;
  const float b = a.bias ? a.bias[n] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const float s = ((acc[r] + red[(0 * 16 + r) * 64 + lane]) + red[(1 * 16 + r) * 64 + lane]) +
                    red[(2 * 16 + r) * 64 + lane];
    const int mm = m0 + (r & 3) + 8 * (r >> 2) + 4 * kl;
    if (mm < M) {
      float v = s * a.alpha + b;
      float* dst = C + (size_t)mm * a.ldc + n;
      if constexpr (EPI == 1) v = v > 0.f ? v : 0.f;
      if constexpr (EPI == 2) v = *dst + v;
      *dst = v;
    }
  }
}

hipError_t gemm(const GemmArgs& a, int batch, hipStream_t s) {
  if (a.hB && !a.b_nt) {  // fp16 weights: the keypoint encoder's ReLU / residual layers only
    dim3 grid((a.N + 31) / 32, (a.M + 31) / 32, batch);
    if (a.epi == 1) hipLaunchKernelGGL(gemm_h_kernel<1>, grid, dim3(256), 0, s, a);
    else if (a.epi == 2) hipLaunchKernelGGL(gemm_h_kernel<2>, grid, dim3(256), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
  }
  if (a.b_nt) {
    dim3 grid((a.N + 63) / 64, (a.M + 63) / 64, batch);
    hipLaunchKernelGGL((gemm_kernel<0, true>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
  }
  dim3 grid((a.N + 31) / 32, (a.M + 31) / 32, batch);
  if (a.epi == 1) {
    hipLaunchKernelGGL(gemm_sk_kernel<1>, grid, dim3(256), 0, s, a);
  } else if (a.epi == 2) {
    hipLaunchKernelGGL(gemm_sk_kernel<2>, grid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(gemm_sk_kernel<0>, grid, dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

__global__ void to_half_t_kernel(const float* W, int K, int N, _Float16* Wt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K * N) return;
  const int n = i / K, k = i - n * K;
  Wt[i] = (_Float16)W[(size_t)k * N + n];
}

hipError_t to_half_t(const float* W, int K, int N, _Float16* Wt, hipStream_t s) {
  hipLaunchKernelGGL(to_half_t_kernel, dim3((K * N + 255) / 256), dim3(256), 0, s, W, K, N, Wt);
  return hipGetLastError();
}

// fp16 GEMM epilogue of one output element (MODE 0: C32 = v, the only mode left)
template <int MODE>
__device__ __forceinline__ void gemm_h_store(const GemmHArgs& a, int m, int n, float v) {
  static_assert(MODE == 0, "gemm_h stores fp32 only");
  a.C32[(size_t)m * a.ldc32 + n] = v;
}

// ---------------------------------------------------------------------------
// fp16 GEMM for final_proj (gemm_h; M = 2B x nmax tokens, K = 256; MODE 0, TN 1 is the one instantiation): one
// workgroup per 32 x (32 TN) output tile, K split four ways (wave w takes the w-th quarter,
// K / 64 <= 8 MFMA steps with every load in flight at once: a single memory round trip).
// Lane (r, h) loads its fragments straight from global memory (16 bytes of row r at
// k = 16 s + 8 h, the 32x32x16 operand layout); the four partial tiles are summed in wave
// order through LDS (16 KB) and stored coalesced.  Small LDS / VGPR footprint, so the BA's
// latency-bound kernels still find room on the CUs while the GNN runs.
// ---------------------------------------------------------------------------
constexpr int kRdU = 8;  // max K steps (16 each) per wave: K <= 512
template <int MODE, int TN>
__global__ __launch_bounds__(256) void gemm_rk_kernel(GemmHArgs a, int ntn) {
  __shared__ float red[4][TN * 16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tm = blockIdx.x / ntn, tn = blockIdx.x - tm * ntn;
  const int m0 = 32 * tm, n0 = 32 * TN * tn;
  const int r = lane & 31, h = lane >> 5;
  const int m = m0 + r;
  const bool mok = m < a.M;
  const int nsw = a.K / 64, k0 = wv * nsw * 16;
  const _Float16* Ap = a.A + (size_t)(mok ? m : 0) * a.lda + 8 * h;
  const _Float16* A2p = a.A2 ? a.A2 + (size_t)(mok ? m : 0) * a.lda2 + 8 * h - a.ksplit : nullptr;
  const _Float16* Bp[TN];
  bool nok[TN];
#pragma unroll
  for (int t = 0; t < TN; t++) {
    const int n = n0 + 32 * t + r;
    nok[t] = n < a.N;
    Bp[t] = a.B + (size_t)(nok[t] ? n : 0) * a.ldb + 8 * h;
  }
  half8 av[kRdU], bv[kRdU][TN];
  const half8 z = {};
#pragma unroll
  for (int u = 0; u < kRdU; u++) {
    const int k = k0 + 16 * u;
    const bool in = u < nsw;
    const _Float16* src = (A2p && k >= a.ksplit) ? A2p + k : Ap + k;
    av[u] = (in && mok) ? *reinterpret_cast<const half8*>(src) : z;
#pragma unroll
    for (int t = 0; t < TN; t++) bv[u][t] = (in && nok[t]) ? *reinterpret_cast<const half8*>(Bp[t] + k) : z;
  }
  floatx16 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[t][i] = 0.f;
#pragma unroll
  for (int u = 0; u < kRdU; u++)
    if (u < nsw)
#pragma unroll
      for (int t = 0; t < TN; t++) acc[t] = mfma16(av[u], bv[u][t], acc[t]);
#pragma unroll
  for (int t = 0; t < TN; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) red[wv][16 * t + i][lane] = acc[t][i];
  __syncthreads();
#pragma unroll
  for (int e = threadIdx.x; e < TN * 16 * 64; e += 256) {
    const int i16 = e >> 6, ln = e & 63;
    const float v = (red[0][i16][ln] + red[1][i16][ln]) + (red[2][i16][ln] + red[3][i16][ln]);
    const int t = i16 >> 4, i = i16 & 15;
    const int n = n0 + 32 * t + (ln & 31);
    const int mm = m0 + (i & 3) + 8 * (i >> 2) + 4 * (ln >> 5);
    if (n < a.N && mm < a.M) gemm_h_store<MODE>(a, mm, n, v + (a.bias ? a.bias[n] : 0.f));
  }
}

hipError_t gemm_h(const GemmHArgs& a, hipStream_t s) {
  if (a.K % 64 != 0 || a.K > 64 * kRdU || (a.A2 && a.ksplit % 16 != 0)) return hipErrorInvalidValue;
  const int ntn = (a.N + 31) / 32, tiles = (a.M + 31) / 32 * ntn;
  hipLaunchKernelGGL((gemm_rk_kernel<0, 1>), dim3(tiles), dim3(256), 0, s, a, ntn);
  return hipGetLastError();
}

__global__ void to_half_kernel(const float* x, _Float16* y, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (_Float16)x[i];
}

hipError_t to_half(const float* x, _Float16* y, size_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n);
  return hipGetLastError();
}

// n-major fp16 weights Wt [N][K] -> 32x32x16 MFMA B-fragment order: block (nt, ks) = the 64 lanes'
// 16-byte operands of n-tile nt, k-step ks, lane L = r + 32 h holding Wt[32 nt + r][16 ks + 8 h ..];
// a wave's operand load is then one contiguous 1 KB read
__global__ void frag_kernel(const _Float16* Wt, int N, int K, _Float16* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // one 8-half operand
  const int KS = K / 16;
  if (i >= (N / 32) * KS * 64) return;
  const int L = i & 63, blk = i >> 6, nt = blk / KS, ks = blk - nt * KS, r = L & 31, h = L >> 5;
  *reinterpret_cast<uint4*>(out + (size_t)i * 8) =
      *reinterpret_cast<const uint4*>(Wt + (size_t)(32 * nt + r) * K + 16 * ks + 8 * h);
}

hipError_t to_frag(const _Float16* Wt, int N, int K, _Float16* out, hipStream_t s) {
  if (N % 32 || K % 16) return hipErrorInvalidValue;
  const int n = (N / 32) * (K / 16) * 64;
  hipLaunchKernelGGL(frag_kernel, dim3((n + 255) / 256), dim3(256), 0, s, Wt, N, K, out);
  return hipGetLastError();
}

}  // namespace sg
}  // namespace rspl
