// The line detector after Canny's classes on the device (FastLineDetector restated, oracle/fld_ref.py): see
// fld_kernels.hpp for the five stages.  Chains interact only through the pixels they consume and never leave
// their 8-connected component, so walking each component on its own with its seeds in raster order and sorting
// the segments by (seed raster index, index within the chain) gives the sequential detector's output exactly.
// Every loop is bounded by a pixel count and every cap ends in a status bit, never in a hang or a stray write.
#include "fld_kernels.hpp"

#pragma clang fp contract(off)

namespace rspl {
namespace fld {

namespace {

constexpr int kT = 1024;

__device__ __forceinline__ void flag(int* meta, int bit) { atomicOr(meta + kStatus, bit); }

// inclusive scan of one int per thread over the 1024-thread block; sc is [1024] in LDS
__device__ int block_scan(int v, int* sc) {
  const int tid = threadIdx.x;
  sc[tid] = v;
  __syncthreads();
  for (int o = 1; o < kT; o <<= 1) {
    const int t = tid >= o ? sc[tid - o] : 0;
    __syncthreads();
    sc[tid] += t;
    __syncthreads();
  }
  return sc[tid];
}

__host__ __device__ inline int sort_cap(int hp) {  // keys the bitonic sort may have to hold (a power of two)
  int p = 2;
  while (p < hp && p < kMaxEdge) p <<= 1;
  return p;
}
__host__ __device__ inline int labels_main_words(int hh, int hw) {
  const int m = 2 * hh * words_per_row(hw), p = sort_cap(hh * hw);
  return m > p ? m : p;
}

// ---------------------------------------------------------------------------------------------------------
// 1. hysteresis.  E (edges) and C (candidates) as bitmasks in LDS; E |= dilate8(E) & C until a block-wide
// reduction reports no change.  A word is updated in place by its one owner thread while neighbours may read
// it: the update is monotone (bits are only ever set), so a stale read only delays a bit to the next pass and
// the fixed point -- reached when a whole pass changes nothing -- is the same.  Each word also saturates
// along its own row within the pass.  Passes <= pixels.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void hysteresis_kernel(Args a) {
  extern __shared__ uint32_t lds[];
  const int b = blockIdx.x, tid = threadIdx.x, hh = a.hh, hw = a.hw, wpr = words_per_row(hw), nw = hh * wpr;
  const size_t hp = (size_t)hh * hw;
  volatile uint32_t* E = lds;
  uint32_t* Cn = lds + nw;
  const uint8_t* cls = a.cls + b * hp;
  int* meta = a.meta + b * kMetaInts;
  for (int wi = tid; wi < nw; wi += kT) {
    const int r = wi / wpr, c0 = (wi - r * wpr) * 32;
    uint32_t e = 0, c = 0;
    const int nb = min(32, hw - c0);
    for (int k = 0; k < nb; k++) {
      const uint8_t v = cls[(size_t)r * hw + c0 + k];
      e |= (uint32_t)(v == 2) << k;
      c |= (uint32_t)(v == 0) << k;
    }
    E[wi] = e;
    Cn[wi] = c;
  }
  __syncthreads();
  const long long bound = (long long)hp + 1;
  long long passes = 0;
  for (;;) {
    int changed = 0;
    for (int wi = tid; wi < nw; wi += kT) {
      const uint32_t cur = E[wi], cand = Cn[wi] & ~cur;
      if (!cand) continue;
      const int r = wi / wpr, wc = wi - r * wpr;
      uint32_t d = 0;
      for (int dr = -1; dr <= 1; dr++) {
        const int rr = r + dr;
        if (rr < 0 || rr >= hh) continue;
        const int base = rr * wpr + wc;
        const uint32_t v = E[base], l = wc > 0 ? E[base - 1] : 0u, rt = wc + 1 < wpr ? E[base + 1] : 0u;
        d |= v | (v << 1) | (l >> 31) | (v >> 1) | (rt << 31);
      }
      uint32_t n = cur | (d & cand);
      for (int k = 0; k < 32; k++) {  // along the word's own row
        const uint32_t g = ((n << 1) | (n >> 1)) & cand & ~n;
        if (!g) break;
        n |= g;
      }
      if (n != cur) {
        E[wi] = n;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
    if (++passes > bound) {
      if (tid == 0) flag(meta, kStLogic);
      break;
    }
  }
  // the corner zeroing of OpenCV's lineDetection (top-left 6 x 6, bottom-right 5 x 5)
  if (tid < 6 && tid < hh) {
    for (int c = 0; c < min(6, hw); c++) atomicAnd((uint32_t*)lds + tid * wpr, ~(1u << c));
  } else if (tid >= 32 && tid < 37) {
    const int r = hh - 5 + (tid - 32);
    if (r >= 0)
      for (int c = max(hw - 5, 0); c < hw; c++) atomicAnd((uint32_t*)lds + r * wpr + (c >> 5), ~(1u << (c & 31)));
  }
  __syncthreads();
  uint32_t* out = a.ebits + (size_t)b * nw;
  for (int wi = tid; wi < nw; wi += kT) out[wi] = E[wi];
  if (tid == 0) meta[kPasses] = (int)passes;
}

// ---------------------------------------------------------------------------------------------------------
// 2. compaction, labels, component order
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int uf_load(int* lab, int i) {
  return __hip_atomic_load(lab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ int uf_find(int* lab, int a, int N, int& bad) {  // labels only ever point to a smaller index
  for (int it = 0; it <= N; it++) {
    const int p = uf_load(lab, a);
    if (p == a) return a;
    a = p;
  }
  bad = 1;
  return a;
}
__device__ void uf_union(int* lab, int a, int b, int N, int& bad) {  // the larger root hooks under the smaller
  for (int it = 0; it <= N && !bad; it++) {
    a = uf_find(lab, a, N, bad);
    b = uf_find(lab, b, N, bad);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(lab + a, b);
    if (old == a) return;
    a = old;  // another lane hooked a first: go on from where it points
  }
  bad = 1;
}

__global__ __launch_bounds__(kT) void labels_kernel(Args a) {
  extern __shared__ uint32_t lds[];
  const int b = blockIdx.x, tid = threadIdx.x, hh = a.hh, hw = a.hw, wpr = words_per_row(hw), nw = hh * wpr;
  uint32_t* E = lds;
  int* pre = (int*)lds + nw;  // edge pixels before each word
  uint32_t* keys = lds;       // reuses E / pre once the labels are final
  int* sc = (int*)lds + labels_main_words(hh, hw);
  int* misc = sc + kT;
  int* meta = a.meta + b * kMetaInts;
  int* pix = a.pix + (size_t)b * kMaxEdge;
  int* lab = a.lab + (size_t)b * kMaxEdge;
  int* spix = a.spix + (size_t)b * kMaxEdge;
  int* cstart = a.cstart + (size_t)b * (kMaxEdge + 1);
  const uint32_t* in = a.ebits + (size_t)b * nw;
  for (int wi = tid; wi < nw; wi += kT) E[wi] = in[wi];
  if (tid == 0) misc[0] = 0;
  __syncthreads();
  // raster-order list: popcount prefix sums over the words, a contiguous run of words per thread
  const int per = (nw + kT - 1) / kT, w0 = min(tid * per, nw), w1 = min(w0 + per, nw);
  int cnt = 0;
  for (int wi = w0; wi < w1; wi++) cnt += __popc(E[wi]);
  int run = block_scan(cnt, sc) - cnt;
  int N = sc[kT - 1];
  if (N > kMaxEdge) {  // block-uniform
    if (tid == 0) {
      flag(meta, kStEdgePixels);
      meta[kNEdge] = 0;
      meta[kNComp] = 0;
      cstart[0] = 0;
    }
    return;
  }
  for (int wi = w0; wi < w1; wi++) {
    pre[wi] = run;
    const int r = wi / wpr, c0 = (wi - r * wpr) * 32;
    for (uint32_t m = E[wi]; m; m &= m - 1) {
      pix[run] = r * hw + c0 + (__ffs(m) - 1);
      lab[run] = run;
      run++;
    }
  }
  __syncthreads();
  // 8-connected components: union with the four neighbours that precede a pixel in raster order
  int bad = 0;
  for (int i = tid; i < N; i += kT) {
    const int p = pix[i], r = p / hw, c = p - r * hw;
    for (int k = 0; k < 4; k++) {
      const int rr = k == 0 ? r : r - 1, cc = k == 0 ? c - 1 : c + k - 2;
      if (rr < 0 || cc < 0 || cc >= hw) continue;
      const int wi = rr * wpr + (cc >> 5);
      const uint32_t m = E[wi], bit = 1u << (cc & 31);
      if (!(m & bit)) continue;
      uf_union(lab, i, pre[wi] + __popc(m & (bit - 1)), N, bad);
    }
  }
  __syncthreads();
  for (int i = tid; i < N; i += kT) lab[i] = uf_find(lab, i, N, bad);
  if (bad) flag(meta, kStLogic);
  __syncthreads();
  // (label, index) keys: each component contiguous, its pixels still in raster order
  int P = 2;
  while (P < N) P <<= 1;
  for (int k = tid; k < P; k += kT) keys[k] = k < N ? ((uint32_t)lab[k] << 15) | (uint32_t)k : 0xffffffffu;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += kT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint32_t x = keys[i], y = keys[l];
        if ((x > y) == ((i & k) == 0)) {
          keys[i] = y;
          keys[l] = x;
        }
      }
      __syncthreads();
    }
  // component starts: a prefix sum over the positions where the label changes
  const int per2 = (N + kT - 1) / kT, k0 = min(tid * per2, N), k1 = min(k0 + per2, N);
  int heads = 0;
  for (int k = k0; k < k1; k++) heads += k == 0 || (keys[k] >> 15) != (keys[k - 1] >> 15);
  int cid = block_scan(heads, sc) - heads;
  const int ncomp = sc[kT - 1];
  for (int k = k0; k < k1; k++) {
    const int p = pix[keys[k] & 0x7fffu], r = p / hw;
    spix[k] = (int)pack_pt(p - r * hw, r);
    if (k == 0 || (keys[k] >> 15) != (keys[k - 1] >> 15)) cstart[cid++] = k;
  }
  if (tid == 0) cstart[ncomp] = N;
  __syncthreads();
  int big = 0;
  for (int c = tid; c < ncomp; c += kT) big = max(big, cstart[c + 1] - cstart[c]);
  if (big) atomicMax(misc, big);
  __syncthreads();
  if (tid == 0) {
    meta[kNEdge] = N;
    meta[kNComp] = ncomp;
    meta[kMaxComp] = misc[0];
  }
}

// LDS words the walk has left for the component-ordered pixel list beside its bitmask, counters and choice table
// (160 KiB per workgroup)
__host__ __device__ inline int walk_list_words(int hh, int hw) {
  int s = 40960 - 64 - (hh * words_per_row(hw) + 2 + 9 * 64);
  s = s < hh * hw ? s : hh * hw;
  s = s < kMaxEdge ? s : kMaxEdge;
  return s > 0 ? s : 0;
}

// ---------------------------------------------------------------------------------------------------------
// 3. walk: one wave, one lane per component (a lane that finishes takes the next one).  A lane either seeks
// its component's next pixel that is still set or takes one getPointChain step.  A component's chains consume
// disjoint pixels of it, so their points go to the component's own range of the point buffer.  What the loop
// costs is the latency of what it waits for, so the bitmask, the choice table and -- when it fits, as it does
// below about 24 k edge pixels at 960 x 540 -- the pixel list are in LDS, and global memory is only stored to.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void walk_kernel(Args a) {
  extern __shared__ uint32_t lds[];
  const int b = blockIdx.x, tid = threadIdx.x, hh = a.hh, hw = a.hw, wpr = words_per_row(hw), nw = hh * wpr;
  uint32_t* E = lds;
  int* ctr = (int*)lds + nw;  // [0] next component, [1] chains
  // getPointChain's choice for every neighbour mask: [0][mask] at step 0, [direction + 4][mask] (direction -3 .. 4)
  // at later steps; 0 = none, else neighbour index + 1.  Filled by chain_pick itself, the host's function.
  uint8_t* pick = (uint8_t*)(ctr + 2);
  for (int t = tid; t < 9 * 256; t += 64)
    pick[t] = (uint8_t)(chain_pick((unsigned)t & 255u, (t >> 8) - 4, t >> 8) + 1);
  int* meta = a.meta + b * kMetaInts;
  const int* spix = a.spix + (size_t)b * kMaxEdge;
  const int N = meta[kNEdge], ncomp = meta[kNComp];
  // (two explicit paths, not one pointer to either memory: a read through a generic pointer would wait for the
  // point stores before it as well)
  const int* list = (const int*)(pick + 9 * 256);
  const bool in_lds = N <= walk_list_words(hh, hw);
  if (in_lds)
    for (int i = tid; i < N; i += 64) ((int*)lds)[(list - (const int*)lds) + i] = spix[i];
  const int* cstart = a.cstart + (size_t)b * (kMaxEdge + 1);
  uint32_t* pts = a.pts + (size_t)b * kMaxEdge;
  int* chains = a.chains + (size_t)b * kMaxEdge * 3;
  const uint32_t* in = a.ebits + (size_t)b * nw;
  for (int wi = tid; wi < nw; wi += 64) E[wi] = in[wi];
  if (tid < 2) ctr[tid] = 0;
  __syncthreads();
  // Plain reads indexed off the LDS array itself: through a volatile pointer, or one held in a struct, they become
  // generic-address loads, which wait for the point stores before them.  A lane only ever tests pixels of its own
  // component, whose bits no other lane clears, and its own atomic clears order its later reads.
  auto edge = [&](int px, int py) { return (lds[py * wpr + (px >> 5)] >> (px & 31)) & 1u; };
  auto clear = [&](int x, int y) { atomicAnd(E + y * wpr + (x >> 5), ~(1u << (x & 31))); };
  enum { GRAB, SEEK, STEP };
  int mode = GRAB, k = 0, end = 0, wpos = 0, x = 0, y = 0, dir = 0, step = 0, seed = 0, off = 0;
  const int bound = 5 * N + 8;  // one lane's seeks, steps and chain ends (<= N each) and its component grabs and ends
  int it = 0;
  for (; it < bound; it++) {
    if (mode == GRAB) {
      const int c = atomicAdd(ctr, 1);
      if (c >= ncomp) break;
      k = wpos = cstart[c];
      end = cstart[c + 1];
      if (k < 0 || end > N || k > end) {
        flag(meta, kStLogic);
        break;
      }
      mode = SEEK;
    } else if (mode == SEEK) {
      if (k >= end) {
        mode = GRAB;
        continue;
      }
      // most of a component's pixels are consumed by earlier chains: four list entries per look, loaded together
      const int nq = min(4, end - k);
      int q[4];
      if (in_lds) {
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = list[k + min(j, nq - 1)];
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = spix[k + min(j, nq - 1)];
      }
      int p = -1, used = nq;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int tx = pt_x((uint32_t)q[j]), ty = pt_y((uint32_t)q[j]);
        if (p >= 0 || j >= nq || tx >= hw || ty >= hh) continue;
        if (edge(tx, ty)) {
          p = ty * hw + tx;
          x = tx;
          y = ty;
          used = j + 1;
        }
      }
      k += used;
      if (p < 0) continue;
      if (wpos >= end) {
        flag(meta, kStLogic);
        break;
      }
      clear(x, y);
      seed = p;
      off = wpos;
      pts[wpos++] = pack_pt(x, y);
      dir = 0;
      step = 0;
      mode = STEP;
    } else if (const int i = pick[((step ? dir + 4 : 0) << 8) | neighbour_mask(edge, hh, hw, x, y)]) {
      x += nb_dc(i - 1);
      y += nb_dr(i - 1);
      dir = nb_dir(i - 1);
      if (wpos >= end) {
        flag(meta, kStLogic);
        break;
      }
      clear(x, y);
      pts[wpos++] = pack_pt(x, y);
      step++;
    } else {
      const int ci = atomicAdd(ctr + 1, 1);
      if (ci >= kMaxEdge) {
        flag(meta, kStLogic);
        break;
      }
      chains[3 * ci] = seed;
      chains[3 * ci + 1] = off;
      chains[3 * ci + 2] = wpos - off;
      mode = SEEK;
    }
  }
  if (it >= bound) flag(meta, kStLogic);
  atomicMax(meta + kWalkIters, it);
  __syncthreads();
  if (tid == 0) meta[kNChain] = min(ctr[1], kMaxEdge);
}

// ---------------------------------------------------------------------------------------------------------
// 4. fit: one lane per chain of at least len_thr + 1 points
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fit_kernel(Args a) {
  const int b = blockIdx.y, hh = a.hh, hw = a.hw;
  int* meta = a.meta + b * kMetaInts;
  const int nch = meta[kNChain];
  const int ci = blockIdx.x * 256 + threadIdx.x;
  if (ci >= nch) return;
  const int* ch = a.chains + ((size_t)b * kMaxEdge + ci) * 3;
  const int seed = ch[0], off = ch[1], len = ch[2];
  if (len < a.len_thr + 1) return;
  if (off < 0 || len > kMaxEdge - off) {
    flag(meta, kStLogic);
    return;
  }
  const uint8_t* half = a.half + (size_t)b * hh * hw;
  unsigned long long* skey = a.skey + (size_t)b * kMaxSeg;
  float* sseg = a.sseg + (size_t)b * kMaxSeg * 4;
  const int lt = a.len_thr;
  extract_segments(a.pts + (size_t)b * kMaxEdge + off, len, lt, a.dist_thr,
                   [&](int k, double x1, double y1, double x2, double y2) {
                     float o[4];
                     if (!finish_segment(half, hh, hw, lt, x1, y1, x2, y2, o)) return;
                     const int si = atomicAdd(meta + kNSeg, 1);
                     if (si >= kMaxSeg) {
                       flag(meta, kStLogic);
                       return;
                     }
                     skey[si] = ((unsigned long long)(uint32_t)seed << 32) | (uint32_t)k;
                     for (int q = 0; q < 4; q++) sseg[4 * si + q] = o[q];
                   });
}

// ---------------------------------------------------------------------------------------------------------
// 5. order: a segment's place is the number of segments with a smaller (seed, k) key (the keys are distinct)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void order_kernel(Args a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int* meta = a.meta + b * kMetaInts;
  const int n = min(meta[kNSeg], kMaxSeg);
  const unsigned long long* skey = a.skey + (size_t)b * kMaxSeg;
  const float* sseg = a.sseg + (size_t)b * kMaxSeg * 4;
  float* out = a.out + (size_t)b * a.capacity * 4;
  for (int s = tid; s < n; s += kT) {
    const unsigned long long key = skey[s];
    int rank = 0;
    for (int t = 0; t < n; t++) rank += skey[t] < key;
    if (rank < a.capacity)
      for (int q = 0; q < 4; q++) out[4 * (size_t)rank + q] = sseg[4 * s + q];
  }
  if (tid == 0) {
    a.counts[b] = n;
    if (n > a.capacity) flag(meta, kStSegments);
  }
}

template <class K>
hipError_t big_lds(K kernel, size_t bytes) {
  if (bytes <= 65536) return hipSuccess;
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

bool mask_fits(int hh, int hw) { return (long long)hh * words_per_row(hw) * 8 <= kMaskLdsBytes; }

hipError_t hysteresis(const Args& a, int B, hipStream_t s) {
  const size_t lds = (size_t)a.hh * words_per_row(a.hw) * 8;
  if (hipError_t e = big_lds(hysteresis_kernel, lds)) return e;
  hipLaunchKernelGGL(hysteresis_kernel, dim3(B), dim3(kT), lds, s, a);
  return hipGetLastError();
}

hipError_t labels(const Args& a, int B, hipStream_t s) {
  const size_t lds = ((size_t)labels_main_words(a.hh, a.hw) + kT + 4) * 4;
  if (hipError_t e = big_lds(labels_kernel, lds)) return e;
  hipLaunchKernelGGL(labels_kernel, dim3(B), dim3(kT), lds, s, a);
  return hipGetLastError();
}

hipError_t walk(const Args& a, int B, hipStream_t s) {
  const size_t lds = ((size_t)a.hh * words_per_row(a.hw) + 2 + walk_list_words(a.hh, a.hw)) * 4 + 9 * 256;
  if (hipError_t e = big_lds(walk_kernel, lds)) return e;
  hipLaunchKernelGGL(walk_kernel, dim3(B), dim3(64), lds, s, a);
  return hipGetLastError();
}

hipError_t fit(const Args& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(fit_kernel, dim3(kMaxEdge / 256, B), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t order(const Args& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(order_kernel, dim3(B), dim3(kT), 0, s, a);
  return hipGetLastError();
}

}  // namespace fld
}  // namespace rspl
