// SuperGlue input packing and AttentionalGNN on gfx950 (CDNA4): prep, the fp32 attention kernel and the fused
// fp16 layer.  Each kernel is followed by its host launcher.
//
// Reference semantics (convert2onnx/superglue.py; src/super_glue.cpp):
//   attention/MHA :88-142 (channel c = d*4 + h), GNN :145-173,
//   process_input (double -> float packing) super_glue.cpp:199-246,
//   PointMatching::NormalizeKeypoints point_matching.cc:50-62.
// Layout: token-major.  Token t = (pair*2 + image)*nmax + i; descriptors X[t][256].
// Q/K/V channels are stored head-contiguous (h*64 + d); the weight rows are
// permuted once on the host so this equals the reference's d*4 + h interleave.
#include <hip/hip_runtime.h>

#include "sg_device.hpp"
#include "sg_kernels.hpp"

namespace rspl {
namespace sg {

// ---------------------------------------------------------------------------
// process_input + NormalizeKeypoints: one wave per token.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_kernel(PrepArgs a) {
  const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  const int total = a.B * 2 * a.nmax;
  if (w >= total) return;
  const int i = w % a.nmax, pi = w / a.nmax, p = pi >> 1, img = pi & 1;
  const int n = img ? a.n1[p] : a.n0[p];
  float* X = a.X + (size_t)w * 256;
  float* kin = a.kin + (size_t)w * 16;
  if (i >= n) {  // padding tokens: zeros (finite everywhere downstream)
    *reinterpret_cast<float4*>(X + 4 * lane) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < 16) kin[lane] = 0.f;
    return;
  }
  const double* f = (img ? a.f1 : a.f0) + ((size_t)p * a.stride + i) * 259;
  if (lane < 16) {
    float v = 0.f;
    if (lane == 0 || lane == 1) {
      double c = f[1 + lane];
      if (a.normalize) {
        const int half = (lane == 0 ? a.width : a.height) / 2;  // integer division (point_matching.cc:56-59)
        c = (c - half) / ((a.width > a.height ? a.width : a.height) * 0.7);
      }
      v = (float)c;
    } else if (lane == 2) {
      v = (float)f[0];
    }
    kin[lane] = v;
  }
  float4 d;
  d.x = (float)f[3 + 4 * lane + 0];
  d.y = (float)f[3 + 4 * lane + 1];
  d.z = (float)f[3 + 4 * lane + 2];
  d.w = (float)f[3 + 4 * lane + 3];
  *reinterpret_cast<float4*>(X + 4 * lane) = d;
}

hipError_t prep(const PrepArgs& a, hipStream_t s) {
  const int waves = a.B * 2 * a.nmax;
  hipLaunchKernelGGL(prep_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Multi-head attention, one head and 32 queries per block; the 4 waves split
// the keys (flash split-K) and merge through LDS.  "Swapped" product
// S^T = K Q^T puts keys on registers and queries on lanes, so the softmax
// reductions are in-lane (+ one xor-32 swap) and S^T feeds O^T = V^T P^T as
// the MFMA B operand with no data movement (keys taken in register order).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_kernel(AttnArgs a) {
  __shared__ float Ks[4][32][65];
  __shared__ float Vs[4][32][64];
  __shared__ float Ml[4][32], Ll[4][32];
  const int pz = blockIdx.z, p = pz >> 1, img = pz & 1;
  const int simg = a.cross ? 1 - img : img;
  const int nq = img ? a.n1[p] : a.n0[p];
  const int nk = simg ? a.n1[p] : a.n0[p];
  const int q0 = blockIdx.x * 32;
  if (q0 >= nq || nk <= 0) return;
  const int h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ml = lane & 31, kl = lane >> 5;
  const float* Qb = a.qkv + (size_t)(p * 2 + img) * a.nmax * 768 + h * 64;
  const float* Kb = a.qkv + (size_t)(p * 2 + simg) * a.nmax * 768 + 256 + h * 64;
  const float* Vb = a.qkv + (size_t)(p * 2 + simg) * a.nmax * 768 + 512 + h * 64;
  float qf[32];
  {
    const int q = min(q0 + ml, nq - 1);
    const float* qr = Qb + (size_t)q * 768;
#pragma unroll
    for (int s = 0; s < 32; s++) qf[s] = qr[2 * s + kl];
  }
  floatx16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; r++) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -INFINITY, l_run = 0.f;
  const int ntiles = (nk + 31) / 32;
  // each wave owns key tiles wv, wv+4, ... and a private LDS slot: the next tile is
  // prefetched into registers while the current one is multiplied (no block barriers)
  float4 pk[8], pv[8];
  auto fetch = [&](int t) {
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = lane + 64 * u, row = i >> 4, c4 = (i & 15) * 4, key = t * 32 + row;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (key < nk) {
        kv = *reinterpret_cast<const float4*>(Kb + (size_t)key * 768 + c4);
        vv = *reinterpret_cast<const float4*>(Vb + (size_t)key * 768 + c4);
      }
      pk[u] = kv;
      pv[u] = vv;
    }
  };
  if (wv < ntiles) fetch(wv);
  for (int t = wv; t < ntiles; t += 4) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = lane + 64 * u, row = i >> 4, c4 = (i & 15) * 4;
      Ks[wv][row][c4 + 0] = pk[u].x; Ks[wv][row][c4 + 1] = pk[u].y;
      Ks[wv][row][c4 + 2] = pk[u].z; Ks[wv][row][c4 + 3] = pk[u].w;
      *reinterpret_cast<float4*>(&Vs[wv][row][c4]) = pv[u];
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes landed
    __builtin_amdgcn_wave_barrier();
    if (t + 4 < ntiles) fetch(t + 4);
    floatx16 st;
#pragma unroll
    for (int r = 0; r < 16; r++) st[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 32; s++) st = mfma32(Ks[wv][ml][2 * s + kl], qf[s], st);
    float x[16];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int key = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
      x[r] = key < nk ? st[r] * 0.125f : -INFINITY;  // scores / dim**.5 (superglue.py:90)
      mx = fmaxf(mx, x[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - m_new);
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      x[r] = expf(x[r] - m_new);
      sum += x[r];
    }
    sum += __shfl_xor(sum, 32);
    l_run = l_run * alpha + sum;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; r++) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int key = (s & 3) + 8 * (s >> 2) + 4 * kl;
      o0 = mfma32(Vs[wv][key][ml], x[s], o0);
      o1 = mfma32(Vs[wv][key][32 + ml], x[s], o1);
    }
  }
  __syncthreads();
  float* Om = &Ks[0][0][0];  // reuse: [4][64][32]
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int d = (r & 3) + 8 * (r >> 2) + 4 * kl;
    Om[(wv * 64 + d) * 32 + ml] = o0[r];
    Om[(wv * 64 + 32 + d) * 32 + ml] = o1[r];
  }
  if (kl == 0) {
    Ml[wv][ml] = m_run;
    Ll[wv][ml] = l_run;
  }
  __syncthreads();
  float* O = a.O + (size_t)(p * 2 + img) * a.nmax * 256 + h * 64;
  for (int idx = tid; idx < 32 * 64; idx += 256) {
    const int q = idx >> 6, d = idx & 63;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; w++) M = fmaxf(M, Ml[w][q]);
    float L = 0.f, acc = 0.f;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const float e = (Ml[w][q] == -INFINITY) ? 0.f : __expf(Ml[w][q] - M);
      L += e * Ll[w][q];
      acc += e * Om[(w * 64 + d) * 32 + q];
    }
    if (q0 + q < nq) O[(size_t)(q0 + q) * 256 + d] = acc / L;
  }
}

hipError_t attention(const AttnArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(attn_kernel, dim3((a.nmax + 31) / 32, 4, B * 2), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// One AttentionalGNN layer, fused (fp16 engine; superglue.py:88-173): a 512-thread workgroup
// owns 32 tokens of one image and runs, without leaving the CU,
//   (1) multi-head attention of its 32 queries against all keys / values of the source image
//       (self or cross), flash-style (online softmax; swapped product S^T = K Q^T, keys on registers,
//       queries on lanes): wave w takes head w & 3 and every other 32-key tile; the two partial
//       softmax states per head merge through LDS;
//   (2) mlp.0 on [x | message] (merge folded into W1, BN folded) + ReLU -> HID in LDS;
//   (3) mlp.3 + the residual: x += delta (fp32 stream, fp16 shadow, and the new fp16 x in LDS);
//   (4) the NEXT layer's q / k / v projections of the same 32 tokens (v stored transposed).
// The only cross-token dependency of a layer -- attention reads every token's k / v of the
// layer -- is the kernel boundary: Q/K/V ping-pong between two buffer sets.  All operands of the
// 32x32x16 f16 MFMAs: activations from LDS (rows padded to 1040 B), weights straight from
// global (L2-resident: 1.15 MB per layer, read once per workgroup), fp32 accumulation.
// One launch per layer instead of four (QKV GEMM, attention, mlp.0, mlp.3).
// ---------------------------------------------------------------------------
constexpr int kLdA = 520;  // halves per LDS activation row (512 + 8: 16-byte aligned, bank spread)

// acc[t] += A[32 x K] (LDS rows) * W[n0 + 32 t + r][k]^T, t < NT; W in B-fragment order
// (to_frag): the operand of (n-tile, k-step) is one contiguous 1 KB read per wave
// one output tile per wave: odd k-steps go to a second accumulator set (two independent MFMA
// dependency chains per tile instead of one), summed at the end
template <int NT, bool SPLIT = (NT < 2)>
__device__ __forceinline__ void wave_mm(const _Float16* Al, const _Float16* Wf, int n0, int K, floatx16 (&acc)[NT],
                                        int lda = kLdA) {
  floatx16 acc2[NT];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc2[t][i] = 0.f;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, KS = K / 16;
  const _Float16* ap = Al + r * lda + 8 * h;
  const _Float16* bp[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) bp[t] = Wf + ((size_t)(n0 / 32 + t) * KS * 64 + lane) * 8;
  constexpr int U = 8;  // k-steps per chunk (16 each): the next chunk's weights load during this one
  half8 bcur[U][NT], bnxt[U][NT];
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int t = 0; t < NT; t++) bcur[u][t] = *reinterpret_cast<const half8*>(bp[t] + 512 * u);
  for (int k0 = 0; k0 < K; k0 += 16 * U) {
    const bool more = k0 + 16 * U < K;
    const int ks0 = k0 / 16;
    if (more) {
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int t = 0; t < NT; t++) bnxt[u][t] = *reinterpret_cast<const half8*>(bp[t] + 512 * (ks0 + U + u));
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const half8 a = *reinterpret_cast<const half8*>(ap + k0 + 16 * u);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        if (SPLIT && (u & 1)) acc2[t] = mfma16(a, bcur[u][t], acc2[t]);
        else acc[t] = mfma16(a, bcur[u][t], acc[t]);
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int t = 0; t < NT; t++) bcur[u][t] = bnxt[u][t];
    }
  }
  if (SPLIT)
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] += acc2[t];
}

__global__ __launch_bounds__(512) void layer_kernel(LayerArgs a) {
  extern __shared__ _Float16 lds_l[];
  _Float16* Ab = lds_l;               // [32][kLdA]: x (0..255) | message (256..511)
  _Float16* Hb = lds_l + 32 * kLdA;   // [32][kLdA]: HID; before that the attention merge buffer
  float* Om = reinterpret_cast<float*>(Hb);  // [4 heads][64 d][32 q]
  __shared__ float Ml[4][32], Ll[4][32];
  // XCD-aware placement: the tiles of one token set go to the same XCD(s) (block b runs on XCD
  // b % 8), so each XCD's L2 holds the k / v of one set instead of all of them
  int bx, set;
  if (a.xps > 0) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    set = xcd / a.xps;
    bx = (xcd % a.xps) * a.tpx + slot;
    if (set >= a.nsets || slot >= a.tpx || bx >= (a.nmax + 31) / 32) return;  // whole workgroup
  } else {
    bx = blockIdx.x;
    set = blockIdx.y;
  }
  const int p = set >> 1, img = set & 1;
  const int simg = a.cross ? 1 - img : img;
  const int nk = simg ? a.n1[p] : a.n0[p];
  const int q0 = bx * 32;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 31, kh = lane >> 5;
  const size_t tok0 = (size_t)set * a.nmax + q0;   // first token of the tile
  const int kset = p * 2 + simg;
  // x tile -> LDS (rows past the set clamp to its last token; never stored back)
  for (int e = tid; e < 32 * 32; e += 512) {
    const int row = e >> 5, ch = e & 31;
    const int q = min(q0 + row, a.nmax - 1);
    *reinterpret_cast<uint4*>(Ab + row * kLdA + 8 * ch) =
        *reinterpret_cast<const uint4*>(a.Xh + ((size_t)set * a.nmax + q) * 256 + 8 * ch);
  }
  // the fp32 residual values this lane updates in (3), fetched now so the load latency hides
  // behind attention and mlp.0: X[token row(i)][32 wv + r]
  float xres[16];
  if (!a.qkv_only) {
    const int r_ = lane & 31, h_ = lane >> 5;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * h_;
      const int q = min(q0 + row, a.nmax - 1);
      xres[i] = a.X[((size_t)set * a.nmax + q) * 256 + 32 * wv + r_];
    }
  }
  if (a.qkv_only) __syncthreads();  // prologue: layer 0's q / k / v from the current x
  // ---- (1) attention: head h = wv & 3, key tiles part, part + 2, ... (part = wv >> 2) ----
  if (!a.qkv_only) {
    const int h = wv & 3, part = wv >> 2;
    const _Float16* Qb = a.Qc + (size_t)set * a.nmax * 256 + h * 64;
    // fragment-ordered k / v of (source set, head): 32-key tile t, k-step / (d-half, key-half) blocks
    // of 64 lanes x 16 B, every operand load one contiguous 1 KB read
    const _Float16* Kb = a.Kc + ((size_t)(kset * 4 + h) * a.nt) * 4 * 512 + 8 * lane;
    const _Float16* Vb = a.Vc + ((size_t)(kset * 4 + h) * a.nt) * 4 * 512 + 8 * lane;
    half8 qf[4];
    {
      const _Float16* qr = Qb + (size_t)min(q0 + c, a.nmax - 1) * 256 + 8 * kh;
#pragma unroll
      for (int s4 = 0; s4 < 4; s4++) qf[s4] = *reinterpret_cast<const half8*>(qr + 16 * s4);
    }
    floatx16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      o0[r] = 0.f;
      o1[r] = 0.f;
    }
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles = (nk + 31) / 32;
    // operands two tiles ahead: this wave's tiles are t, t + 2, t + 4, ...; A and B alternate as the
    // operand sets (the loop body is written for a pair of tiles: static register names, no indexing)
    half8 kA[4], vA[2][2], kB[4], vB[2][2];
    auto fetch = [&](int t, half8 (&kf)[4], half8 (&vf)[2][2]) {
#pragma unroll
      for (int s4 = 0; s4 < 4; s4++) kf[s4] = *reinterpret_cast<const half8*>(Kb + ((size_t)t * 4 + s4) * 512);
#pragma unroll
      for (int dt = 0; dt < 2; dt++)
#pragma unroll
        for (int j = 0; j < 2; j++)
          vf[dt][j] = *reinterpret_cast<const half8*>(Vb + ((size_t)t * 4 + 2 * dt + j) * 512);
    };
    auto tile = [&](int t, const half8 (&kc_)[4], const half8 (&vc)[2][2]) {
      floatx16 st;
#pragma unroll
      for (int r = 0; r < 16; r++) st[r] = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < 4; s4++) st = mfma16(kc_[s4], qf[s4], st);
      float x[16];
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int key = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        x[r] = key < nk ? st[r] * 0.125f : -INFINITY;  // scores / dim**.5 (superglue.py:90)
        mx = fmaxf(mx, x[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __expf(m_run - m_new);
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        x[r] = __expf(x[r] - m_new);
        sum += x[r];
      }
      sum += __shfl_xor(sum, 32);
      l_run = l_run * alpha + sum;
      m_run = m_new;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        o0[r] *= alpha;
        o1[r] *= alpha;
      }
#pragma unroll
      for (int j = 0; j < 2; j++) {
        half8 pf;
#pragma unroll
        for (int u = 0; u < 8; u++) pf[u] = (_Float16)x[8 * j + u];
        o0 = mfma16(vc[0][j], pf, o0);
        o1 = mfma16(vc[1][j], pf, o1);
      }
    };
    if (part < ntiles) fetch(part, kA, vA);
    if (part + 2 < ntiles) fetch(part + 2, kB, vB);
    for (int t = part; t < ntiles; t += 4) {
      tile(t, kA, vA);
      if (t + 4 < ntiles) fetch(t + 4, kA, vA);
      if (t + 2 >= ntiles) break;
      tile(t + 2, kB, vB);
      if (t + 6 < ntiles) fetch(t + 6, kB, vB);
    }
    // merge the two partial states of each head (part 1 -> LDS -> part 0), message -> Ab
    if (part == 1) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int d = (r & 3) + 8 * (r >> 2) + 4 * kh;
        Om[(h * 64 + d) * 32 + c] = o0[r];
        Om[(h * 64 + 32 + d) * 32 + c] = o1[r];
      }
      if (kh == 0) {
        Ml[h][c] = m_run;
        Ll[h][c] = l_run;
      }
    }
    __syncthreads();
    if (part == 0) {
      const float m1 = Ml[h][c], l1 = Ll[h][c];
      const float M = fmaxf(m_run, m1);
      const float e0 = m_run == -INFINITY ? 0.f : __expf(m_run - M);
      const float e1 = m1 == -INFINITY ? 0.f : __expf(m1 - M);
      const float L = e0 * l_run + e1 * l1;
      const float inv = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int d = (r & 3) + 8 * (r >> 2) + 4 * kh;
        const float v0 = (e0 * o0[r] + e1 * Om[(h * 64 + d) * 32 + c]) * inv;
        const float v1 = (e0 * o1[r] + e1 * Om[(h * 64 + 32 + d) * 32 + c]) * inv;
        Ab[c * kLdA + 256 + h * 64 + d] = (_Float16)v0;
        Ab[c * kLdA + 256 + h * 64 + 32 + d] = (_Float16)v1;
      }
    }
    __syncthreads();
  }
  const int r = lane & 31, hh = lane >> 5;
  if (!a.qkv_only) {
  // ---- (2) HID = ReLU([x | message] W1^T + b1): wave wv -> columns 64 wv .. 64 wv + 63 ----
  {
    floatx16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[t][i] = 0.f;
    wave_mm<2>(Ab, a.W1, 64 * wv, 512, acc);
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const int n = 64 * wv + 32 * t + r;
      const float b = a.b1[n];
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
        const float v = acc[t][i] + b;
        Hb[row * kLdA + n] = (_Float16)(v > 0.f ? v : 0.f);
      }
    }
  }
  __syncthreads();
  // ---- (3) x += HID W2^T + b2 (fp32 stream, fp16 shadow, new x into Ab): columns 32 wv .. +31 ----
  {
    floatx16 acc[1];
#pragma unroll
    for (int i = 0; i < 16; i++) acc[0][i] = 0.f;
    wave_mm<1>(Hb, a.W2, 32 * wv, 512, acc);
    const int n = 32 * wv + r;
    const float b = a.b2[n];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
      if (q0 + row >= a.nmax) continue;
      const float x = xres[i] + (acc[0][i] + b);
      a.X[(tok0 + row) * 256 + n] = x;
      const _Float16 xh = (_Float16)x;
      a.Xh[(tok0 + row) * 256 + n] = xh;
      Ab[row * kLdA + n] = xh;
    }
  }
  if (a.last) return;
  __syncthreads();
  }
  // ---- (4) next layer's q | k | v of these tokens: columns 96 wv .. 96 wv + 95 ----
  {
    floatx16 acc[3];
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[t][i] = 0.f;
    wave_mm<3>(Ab, a.Wq, 96 * wv, 256, acc);
    __syncthreads();  // every wave is done with Ab: the q | k | v tile is staged over Ab + Hb
    _Float16* Tq = lds_l;  // [32 tokens][776]
#pragma unroll
    for (int t = 0; t < 3; t++) {
      const int n = 96 * wv + 32 * t + r;
      const float b = a.bq[n];
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
        Tq[row * 776 + n] = (_Float16)(acc[t][i] + b);
      }
    }
    __syncthreads();
    // q rows out (valid tokens), 16-byte stores
    for (int e = tid; e < 32 * 32; e += 512) {
      const int row = e >> 5, ch = e & 31;
      if (q0 + row < a.nmax)
        *reinterpret_cast<uint4*>(a.Qn + (tok0 + row) * 256 + 8 * ch) = *reinterpret_cast<const uint4*>(Tq + row * 776 + 8 * ch);
    }
    // k / v in fragment order: this tile is key tile q0 / 32 of the set; 16 + 16 blocks of 1 KB
    const int kt = q0 >> 5;
    for (int e = tid; e < 2 * 16 * 64; e += 512) {
      const int isv = e >> 10, blk = (e >> 6) & 15, L = e & 63, cl = L & 31, kl = L >> 5, hd = blk >> 2, q4 = blk & 3;
      _Float16* dst = (isv ? a.Vn : a.Kn) + (((size_t)(set * 4 + hd) * a.nt + kt) * 4 + q4) * 512 + 8 * L;
      if (!isv) {  // k: key cl, dims 16 q4 + 8 kl .. +7 of head hd
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(Tq + cl * 776 + 256 + 64 * hd + 16 * q4 + 8 * kl);
      } else {  // v: dim 32 dt + cl, keys 16 j + 4 kl + {0..3, 8..11} (q4 = 2 dt + j)
        const int dt = q4 >> 1, j = q4 & 1, d = 512 + 64 * hd + 32 * dt + cl, k0 = 16 * j + 4 * kl;
        half8 v;
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = Tq[(k0 + (u < 4 ? u : u + 4)) * 776 + d];
        *reinterpret_cast<half8*>(dst) = v;
      }
    }
  }
}

hipError_t gnn_layer(const LayerArgs& a, int B, hipStream_t s) {
  constexpr size_t lds = sizeof(_Float16) * 2 * 32 * kLdA;  // x | message, HID (>= the 32 x 776 q|k|v stage)
  static_assert(2 * kLdA >= 776, "q | k | v staging tile exceeds the LDS carve");
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute((const void*)layer_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds);
    if (e != hipSuccess) return e;
    attr = true;
  }
  LayerArgs la = a;
  const int sets = B * 2, tiles = (a.nmax + 31) / 32;
  la.nsets = sets;
  la.xps = sets <= 8 ? 8 / sets : 0;                                // XCDs per token set
  la.tpx = la.xps ? (tiles + la.xps - 1) / la.xps : 0;            // tiles per XCD
  if (la.xps)
    hipLaunchKernelGGL(layer_kernel, dim3(8 * la.tpx), dim3(512), lds, s, la);
  else
    hipLaunchKernelGGL(layer_kernel, dim3(tiles, sets), dim3(512), lds, s, la);
  return hipGetLastError();
}

}  // namespace sg
}  // namespace rspl
