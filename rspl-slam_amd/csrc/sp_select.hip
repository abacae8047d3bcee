// SuperPoint post-processing on gfx950 (CDNA4): simple_nms with candidate extraction, and top-k selection.
//
// Reference semantics:
//   NMS      convert2onnx/superpoint.py:16-33    (simple_nms, radius 4)
//   host     src/super_point.cpp:154-204         (threshold, borders, top-k)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sp_kernels.hpp"

namespace rspl {
namespace sp {

// ---------------------------------------------------------------------------
// Fused simple_nms (5 x 9x9 max-pools) + threshold / border candidate extraction.  Scores are
// softmax outputs (>= 0) and every window contains its centre, so zero padding outside the image
// equals MaxPool2d's -inf padding here.  Tile 64 x 32 outputs with the 20-pixel halo the five
// dependent pools need (104 x 72 in LDS).  Each 1-D pass gives a thread 8 consecutive outputs
// from 16 register-held inputs (van Herk / Gil-Werman with block 8: suffix maxima of the first 8,
// prefix maxima of the second, out[i] = max(suffix[i], prefix[i]) = the 9-window [i, i+8]): 2 LDS
// reads per output instead of 9.  Passes run over the whole region; values near its border are
// garbage that never reaches the output tile (each pool shrinks the valid region by 4, five pools =
// the 20-pixel halo).
// LDS: 10 bytes per region pixel (74.9 KB: two workgroups per CU, every tile of a C3 step in one
// dispatch round) -- scores S and the row-pass scratch T in fp32, max_mask K and supp_mask M in
// bytes; the two mask pools run on bytes (T reused as u8), supp_scores = M ? 0 : S is formed on the
// fly by the score pools.  XCD-aware placement: tile order is row-major per image and the tiles are
// dealt to the 8 XCDs in contiguous bands (blockIdx % 8 = XCD), so the halo rows a tile shares with
// its vertical neighbours are fetched once into that XCD's L2, not once per XCD.
// ---------------------------------------------------------------------------
constexpr int NTX = 64, NTY = 32, NH = 20, RX = NTX + 2 * NH, RY = NTY + 2 * NH;  // 104 x 72
static_assert(RX % 8 == 0 && (RX - 8) % 8 == 0 && (RY - 8) % 8 == 0, "8-output chunks tile the passes");

// 9-window max of 16 register values: out[i] = max(v[i .. i+8]), i < 8
template <typename V>
__device__ __forceinline__ void window9(const V (&v)[16], V (&o)[8]) {
  V suf[8], pre[8];
  suf[7] = v[7];
#pragma unroll
  for (int i = 6; i >= 0; i--) suf[i] = v[i] > suf[i + 1] ? v[i] : suf[i + 1];
  pre[0] = v[8];
#pragma unroll
  for (int i = 1; i < 8; i++) pre[i] = v[8 + i] > pre[i - 1] ? v[8 + i] : pre[i - 1];
#pragma unroll
  for (int i = 0; i < 8; i++) o[i] = suf[i] > pre[i] ? suf[i] : pre[i];
}
__device__ __forceinline__ void window9f(const float (&v)[16], float (&o)[8]) {
  float suf[8], pre[8];
  suf[7] = v[7];
#pragma unroll
  for (int i = 6; i >= 0; i--) suf[i] = fmaxf(v[i], suf[i + 1]);
  pre[0] = v[8];
#pragma unroll
  for (int i = 1; i < 8; i++) pre[i] = fmaxf(pre[i - 1], v[8 + i]);
#pragma unroll
  for (int i = 0; i < 8; i++) o[i] = fmaxf(suf[i], pre[i]);
}
// dst[y][x] = max_{|k|<=4} src'[y][x+k] for every row, x in [4, RX-4), src' = M ? 0 : S when SUPP
template <bool SUPP>
__device__ __forceinline__ void rowpass9(const float* S, const unsigned char* M, float* dst) {
  constexpr int CPR = (RX - 8) / 8;
  for (int c = threadIdx.x; c < CPR * RY; c += blockDim.x) {
    const int y = c / CPR, x0 = 4 + 8 * (c % CPR), b = y * RX + x0 - 4;
    const float4* p = reinterpret_cast<const float4*>(S + b);
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float4 t = p[q];
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
    if (SUPP) {
      const uint2* mp = reinterpret_cast<const uint2*>(M + b);
      const uint2 m0 = mp[0], m1 = mp[1];
      const unsigned mw[4] = {m0.x, m0.y, m1.x, m1.y};
#pragma unroll
      for (int k = 0; k < 16; k++) v[k] = ((mw[k >> 2] >> (8 * (k & 3))) & 0xff) ? 0.f : v[k];
    }
    float o[8];
    window9f(v, o);
    float4* d = reinterpret_cast<float4*>(dst + y * RX + x0);
    d[0] = make_float4(o[0], o[1], o[2], o[3]);
    d[1] = make_float4(o[4], o[5], o[6], o[7]);
  }
}
// the byte (mask) row pass: dst[y][x] = max_{|k|<=4} src[y][x+k]
__device__ __forceinline__ void rowpass9_u8(const unsigned char* src, unsigned char* dst) {
  constexpr int CPR = (RX - 8) / 8;
  for (int c = threadIdx.x; c < CPR * RY; c += blockDim.x) {
    const int y = c / CPR, x0 = 4 + 8 * (c % CPR), b = y * RX + x0 - 4;
    const uint2* mp = reinterpret_cast<const uint2*>(src + b);
    const uint2 m0 = mp[0], m1 = mp[1];
    const unsigned mw[4] = {m0.x, m0.y, m1.x, m1.y};
    unsigned v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = (mw[k >> 2] >> (8 * (k & 3))) & 0xff;
    unsigned o[8];
    window9(v, o);
    uint2 w;
    w.x = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    w.y = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
    *reinterpret_cast<uint2*>(dst + y * RX + x0) = w;
  }
}
// dst[y][x] = max_{|k|<=4} src[y+k][x] for every column, y in [4, RY-4); F(o, x, y0) consumes the
// 8 outputs of column x from row y0
template <typename V, typename F>
__device__ __forceinline__ void colpass9(const V* src, F&& out) {
  constexpr int CPC = (RY - 8) / 8;
  for (int c = threadIdx.x; c < CPC * RX; c += blockDim.x) {
    const int x = c % RX, y0 = 4 + 8 * (c / RX);
    V v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = src[(y0 - 4 + k) * RX + x];
    V o[8];
    window9(v, o);
    out(o, x, y0);
  }
}

__global__ __launch_bounds__(1024) void nms_kernel(NmsArgs a) {
  __shared__ __attribute__((aligned(16))) float S[RY * RX];  // scores (0 outside the image)
  __shared__ __attribute__((aligned(16))) float T[RY * RX];  // row-pass result (fp32, or bytes)
  __shared__ __attribute__((aligned(16))) unsigned char K[RY * RX];  // max_mask
  __shared__ __attribute__((aligned(16))) unsigned char M[RY * RX];  // supp_mask
  unsigned char* T8 = reinterpret_cast<unsigned char*>(T);
  const int H = a.H, W = a.W;
  const int tiles_x = (W + NTX - 1) / NTX, tiles_y = (H + NTY - 1) / NTY;
  const int per = tiles_x * tiles_y, total = a.B * per, band = (total + 7) / 8;
  const int lt = ((int)blockIdx.x & 7) * band + ((int)blockIdx.x >> 3);  // XCD band placement
  if (lt >= total) return;
  const int bi = lt / per, t = lt % per;
  const int y0 = (t / tiles_x) * NTY - NH, x0 = (t % tiles_x) * NTX - NH;
  const float* sc = a.scores + (size_t)bi * H * W;
  for (int i = threadIdx.x; i < RY * RX; i += blockDim.x) {
    const int ly = i / RX, lx = i - ly * RX;
    const int y = y0 + ly, x = x0 + lx;
    S[i] = (y >= 0 && y < H && x >= 0 && x < W) ? sc[(size_t)y * W + x] : 0.f;
  }
  __syncthreads();
  // max_mask = scores == max_pool(scores)
  rowpass9<false>(S, M, T);
  __syncthreads();
  colpass9(T, [&](const float (&o)[8], int x, int y) {
#pragma unroll
    for (int k = 0; k < 8; k++) K[(y + k) * RX + x] = S[(y + k) * RX + x] == o[k];
  });
  __syncthreads();
  for (int it = 0; it < 2; it++) {
    // supp_mask = max_pool(max_mask) > 0 (byte pools)
    rowpass9_u8(K, T8);
    __syncthreads();
    colpass9(T8, [&](const unsigned char (&o)[8], int x, int y) {
#pragma unroll
      for (int k = 0; k < 8; k++) M[(y + k) * RX + x] = o[k] > 0;
    });
    __syncthreads();
    // supp_scores = where(supp_mask, 0, scores); new_max_mask = supp_scores == max_pool(supp_scores);
    // max_mask |= new_max_mask & ~supp_mask
    rowpass9<true>(S, M, T);
    __syncthreads();
    colpass9(T, [&](const float (&o)[8], int x, int y) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = (y + k) * RX + x;
        const bool m = M[i] != 0;
        const float f = m ? 0.f : S[i];
        K[i] = K[i] | ((f == o[k]) && !m);
      }
    });
    __syncthreads();
  }
  // output region [NH, NH+NTY) x [NH, NH+NTX): NMS'd map (debug entry points only) + candidates.
  // The workgroup reserves its candidates' slots with ONE atomic (wave ballots + a scan of the
  // wave counts): a per-candidate atomic on the image's counter serialises thousands of
  // candidates at one L2 address.  Slot order is free: top-k orders by (score, flat index).
  static_assert(NTX * NTY == 2 * 1024, "two outputs per thread");
  __shared__ int wcount[16], wbase[16], blk_base;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long key[2];
  bool take[2];
  int mine = 0;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int i = threadIdx.x + q * 1024;
    const int ly = NH + i / NTX, lx = NH + i % NTX;
    const int y = y0 + ly, x = x0 + lx;
    take[q] = false;
    key[q] = 0;
    if (y < H && x < W) {
      const float v = K[ly * RX + lx] ? S[ly * RX + lx] : 0.f;
      if (a.nms_out) a.nms_out[(size_t)bi * H * W + (size_t)y * W + x] = v;
      // find_high_score_index: float score > double threshold (src/super_point.cpp:158);
      // remove_borders: border <= y < H-border, border <= x < W-border (:244-245)
      take[q] = (double)v > a.threshold && y >= a.border && y < H - a.border && x >= a.border && x < W - a.border;
      key[q] = ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(v)) << 32) | (unsigned)(y * W + x);
    }
    mine += take[q];
  }
  // exclusive prefix of `mine` within the wave (lane order), then over the waves
  int pre = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(pre, o);
    if (lane >= o) pre += t;
  }
  if (lane == 63) wcount[wv] = pre;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int w = 0; w < 16; w++) {
      wbase[w] = run;
      run += wcount[w];
    }
    blk_base = run ? atomicAdd(&a.cand_count[bi], run) : 0;
  }
  __syncthreads();
  int slot = blk_base + wbase[wv] + pre - mine;
#pragma unroll
  for (int q = 0; q < 2; q++)
    if (take[q]) {
      if (slot < a.cand_cap) a.cand[(size_t)bi * a.cand_cap + slot] = key[q];
      slot++;
    }
}

hipError_t nms(const NmsArgs& a, int B, hipStream_t s) {
  const int tiles = ((a.W + NTX - 1) / NTX) * ((a.H + NTY - 1) / NTY);
  NmsArgs b = a;
  b.B = B;
  hipLaunchKernelGGL(nms_kernel, dim3(8 * ((B * tiles + 7) / 8)), dim3(1024), 0, s, b);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Top-k selection: one workgroup per image, bitonic sort in LDS.
// Key = (~score_bits << 32) | flat_index: ascending key order = score desc,
// then flat index asc (documented tie-break for the reference's non-stable
// std::sort, src/super_point.cpp:185-190).  If n <= k the reference does not
// sort: keypoints stay in row-major scan order (flat index asc).
// ---------------------------------------------------------------------------
// Keys are (~score bits) << 32 | flat index: ascending key = descending score, ties by flat
// index.  Up to lds_cap candidates are sorted whole in LDS (bitonic).  With more (large images)
// and k > 0, an MSB-first 8-bit radix select over the 64-bit keys (LDS histograms) finds the
// exact k-th key first; the k keys at or below it are compacted into LDS and sorted there.
__global__ __launch_bounds__(1024) void topk_kernel(TopkArgs a) {
  extern __shared__ unsigned long long keys[];
  __shared__ unsigned hist[256];
  __shared__ unsigned long long sel_prefix, sel_mask;
  __shared__ unsigned sel_want, sel_n;
  const int bi = blockIdx.x;
  int n = a.cand_count[bi];
  if (n > a.cand_cap) n = a.cand_cap;
  const bool sorted_by_score = (a.k != -1 && a.k < n);
  const unsigned long long* src = a.cand + (size_t)bi * a.cand_cap;
  // k = 0 keeps nothing (the reference's k < n sort-and-resize, src/super_point.cpp:192-204): no select, keys[]
  // untouched.  Keep-all beyond the LDS sort also yields 0, reported by the host.
  if (a.k == 0 || (n > a.lds_cap && !sorted_by_score)) {
    if (threadIdx.x == 0) a.sel_count[bi] = 0;
    return;
  }
  // k well below the candidate count (or beyond the LDS sort): select the k-th key first, then
  // sort only the k selected keys (the same k keys in the same order as sorting all of them)
  if (sorted_by_score && (n > a.lds_cap || n > 2 * a.k)) {
    if (threadIdx.x == 0) {
      sel_prefix = 0;
      sel_mask = 0;
      sel_want = (unsigned)a.k;
      sel_n = 0;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
      for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
      __syncthreads();
      const unsigned long long pre = sel_prefix, msk = sel_mask;
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned long long key = src[i];
        if ((key & msk) == pre) atomicAdd(&hist[(key >> shift) & 255], 1u);
      }
      __syncthreads();
      if (threadIdx.x < 64) {  // the first bin whose cumulative count reaches sel_want: wave scan
        const int l = threadIdx.x;
        unsigned h[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          h[j] = hist[4 * l + j];
          sum += h[j];
        }
        unsigned incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned y = __shfl_up(incl, o);
          if (l >= o) incl += y;
        }
        const unsigned want = sel_want, excl = incl - sum;
        const bool mine = excl < want && want <= incl;
        const unsigned long long any = __ballot(mine);
        if (mine || (any == 0 && l == 63)) {  // (a bin is always found: the total reaches want)
          unsigned below = excl, d = 4 * l, j = 0;
          while (j < 3 && below + h[j] < want) below += h[j++];
          d += j;
          sel_want = want - below;
          sel_prefix |= (unsigned long long)d << shift;
          sel_mask |= 0xFFull << shift;
        }
      }
      __syncthreads();
    }
    const unsigned long long kth = sel_prefix;  // keys are unique: exactly k keys are <= kth
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const unsigned long long key = src[i];
      if (key <= kth) keys[atomicAdd(&sel_n, 1u)] = key;
    }
    __syncthreads();
    n = a.k;
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      unsigned long long key = src[i];
      if (!sorted_by_score) key &= 0xFFFFFFFFull;  // flat index only
      keys[i] = key;
    }
  }
  int L = 1;
  while (L < n) L <<= 1;
  for (int i = n + threadIdx.x; i < L; i += blockDim.x) keys[i] = ~0ull;
  __syncthreads();
  for (int size = 2; size <= L; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < L / 2; i += blockDim.x) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const unsigned long long x = keys[lo], y = keys[hi];
        if ((x > y) == up) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  const int kout = sorted_by_score ? a.k : n;
  for (int i = threadIdx.x; i < kout; i += blockDim.x) a.sel[(size_t)bi * a.sel_cap + i] = (unsigned)(keys[i] & 0xFFFFFFFFull);
  if (threadIdx.x == 0) a.sel_count[bi] = kout;
}

hipError_t topk(const TopkArgs& a, int B, hipStream_t s) {
  int L = 1;
  while (L < a.lds_cap) L <<= 1;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)(L * sizeof(unsigned long long)));
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL(topk_kernel, dim3(B), dim3(1024), L * sizeof(unsigned long long), s, a);
  return hipGetLastError();
}

}  // namespace sp
}  // namespace rspl
