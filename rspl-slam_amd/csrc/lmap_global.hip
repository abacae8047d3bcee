// Global descriptor search of the local table on fp64 MFMA (relocalisation).
//   lmap_gpack_kernel    the frame's descriptors (rows 3..258 of the records, 8-byte aligned at a 2072-byte stride)
//                        into a dense 16-byte-aligned [Kpad][256] array, zero rows past n1; the clamped count
//   lmap_gsearch_kernel  one workgroup per (query tile of 64 keypoints, chunk of bank rows, frame): 64 bank rows at
//                        a time (through local_row) against the tile, both staged through LDS in slabs of 64
//                        descriptor entries with 16-byte global loads one slab ahead in registers; wave w owns
//                        keypoints 16w..16w+15 against all 64 bank rows: four 16x16 fp64 accumulator tiles of
//                        v_mfma_f64_16x16x4_f64.  The epilogue reads the accumulators in place: per keypoint
//                        (best, second, arg) accumulates in-lane over the chunk and crosses the 16 lanes of a row
//                        once at the end; per bank row (min, arg) goes in-lane over the 4 registers, across the four
//                        16-lane groups, then across the waves through LDS.  Padding rows and columns are masked by
//                        index, never through their values.
//   lmap_gfold_kernel    the partials folded: a wave per keypoint over its chunks, a thread per local point over its
//                        query tiles (kbest goes to host-mapped memory from here, coalesced)
//   lmap_gmerge_kernel   one block per frame: the pass and mutual tests, the matches
//                        compacted in keypoint order (a contiguous quarter per wave, ballot + prefix), the results
//                        written to host-mapped memory last, in bulk
// No atomics anywhere; every fold is order-free (lmap_global.hpp), so the result does not depend on the schedule.
#include "lmap_global.hpp"
#include "wave_reduce.hpp"

namespace rspl {
namespace lmap {
namespace {

constexpr int T = 256, NW = 4, kXcds = 8;
typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
constexpr int kPitch = kGSlab + 2;  // doubles per LDS row: 528 bytes, 16-byte aligned; the 16 rows x 2 k of one
                                    // half-wave's ds_read_b64 fall on 32 distinct bank pairs of the 64
constexpr int kUnits = kGSlab / 2;  // 16-byte units per row and slab
constexpr int kLoads = kGQTile * kUnits / T;  // 16-byte loads per thread, matrix and slab
static_assert(kGQTile == kGGroup && kGQTile * kUnits % T == 0 && kDesc % kGSlab == 0, "staging geometry");

__global__ __launch_bounds__(T) void lmap_gpack_kernel(GArgs a) {
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int i = blockIdx.x * NW + (threadIdx.x >> 6);  // < Kpad: the grid is Kpad / NW
  const GParam P = a.host_params[f];
  int n1 = *P.n1;
  n1 = n1 < 0 ? 0 : (n1 > a.K ? a.K : n1);
  if (i == 0 && lane == 0) {
    a.params[f] = P;
    a.n1c[f] = n1;
  }
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  if (i < n1) {
    const double* src = P.feat + RSPL_FEATURE_ROWS * (size_t)i + 3 + 4 * lane;  // 8-byte aligned only
    s0 = src[0]; s1 = src[1]; s2 = src[2]; s3 = src[3];
  }
  double2* dst = reinterpret_cast<double2*>(a.qpack + ((size_t)f * a.Kpad + i) * kDesc) + 2 * lane;
  dst[0] = make_double2(s0, s1);
  dst[1] = make_double2(s2, s3);
}

__device__ __forceinline__ double shfl_xor_f64(double v, int m) { return __shfl_xor(v, m, 64); }

__global__ __launch_bounds__(T) void lmap_gsearch_kernel(GArgs a, int n_local) {
  __shared__ double As[kGQTile * kPitch];
  __shared__ double Bs[kGGroup * kPitch];
  __shared__ double cmin[NW][kGGroup];
  __shared__ int carg[NW][kGGroup];

  // Blocks are dealt to the 8 XCDs round-robin by linear index: block b runs on XCD b % 8.  The query tiles of one
  // chunk take consecutive slots of ONE XCD, so the chunk's bank rows are fetched into one L2, not into eight.
  const int xcd = blockIdx.x % kXcds, slot = blockIdx.x / kXcds;
  const int qt = slot % a.n_qtiles, chunk = (slot / a.n_qtiles) * kXcds + xcd, f = blockIdx.y;
  if (chunk * a.chunk_rows >= n_local) return;  // block-uniform: the grid is padded to a multiple of 8 chunks
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int n1 = a.n1c[f];
  const int q0 = qt * kGQTile;
  if (q0 >= n1) return;  // block-uniform: the merge reads the query tiles below n1 only
  const int c0 = chunk * a.chunk_rows;
  const int c1 = c0 + a.chunk_rows < n_local ? c0 + a.chunk_rows : n_local;  // c0 < n_local: the grid's size

  const int lr = lane & 15, lq = lane >> 4;
  // staging: unit u = tid + T j of a slab is row u / 16, 16-byte column u % 16
  const int srow = tid / kUnits, scol = tid % kUnits;
  const double* qsrc[kLoads];
#pragma unroll
  for (int j = 0; j < kLoads; j++)
    qsrc[j] = a.qpack + ((size_t)f * a.Kpad + q0 + srow + (T / kUnits) * j) * kDesc + 2 * scol;

  GBest kb[4];  // keypoint q0 + 16 wv + lq + 4 r over this lane's columns of the chunk

  for (int g0 = c0; g0 < c1; g0 += kGGroup) {
    const double* bsrc[kLoads];
#pragma unroll
    for (int j = 0; j < kLoads; j++) {
      int p = g0 + srow + (T / kUnits) * j;
      p = p < n_local ? p : n_local - 1;  // a padding column reads a valid row; it is masked by index below
      bsrc[j] = a.bank + (size_t)a.local_row[p] * kDesc + 2 * scol;
    }
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};

    v2d ra[kLoads], rb[kLoads];
#pragma unroll
    for (int j = 0; j < kLoads; j++) {
      ra[j] = *reinterpret_cast<const v2d*>(qsrc[j]);
      rb[j] = *reinterpret_cast<const v2d*>(bsrc[j]);
    }
#pragma unroll 1
    for (int s = 0; s < kDesc / kGSlab; s++) {
      __syncthreads();  // the previous slab's reads (and the previous group's cmin reads) are done
#pragma unroll
      for (int j = 0; j < kLoads; j++) {
        const int o = (srow + (T / kUnits) * j) * kPitch + 2 * scol;
        *reinterpret_cast<v2d*>(As + o) = ra[j];
        *reinterpret_cast<v2d*>(Bs + o) = rb[j];
      }
      __syncthreads();
      if (s + 1 < kDesc / kGSlab) {
#pragma unroll
        for (int j = 0; j < kLoads; j++) {
          ra[j] = *reinterpret_cast<const v2d*>(qsrc[j] + (s + 1) * kGSlab);
          rb[j] = *reinterpret_cast<const v2d*>(bsrc[j] + (s + 1) * kGSlab);
        }
      }
      // A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]: both images are [row][k]
      const double* ap = As + (16 * wv + lr) * kPitch + lq;
      const double* bp = Bs + lr * kPitch + lq;
#pragma unroll
      for (int ks = 0; ks < kGSlab / 4; ks++) {
        const double av = ap[4 * ks];
#pragma unroll
        for (int t = 0; t < 4; t++)
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[16 * t * kPitch + 4 * ks], acc[t], 0, 0, 0);
      }
    }

    // C/D: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int p = g0 + 16 * t + lr;
      const bool pv = p < n_local;
      GMin cm;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = q0 + 16 * wv + lq + 4 * r;
        const double d = distance_of(acc[t][r]);
        if (pv) kb[r].visit(d, p);
        if (i < n1) cm.visit(d, i);
      }
#pragma unroll
      for (int m = 16; m <= 32; m <<= 1) {
        const double ov = shfl_xor_f64(cm.v, m);
        const int oi = __shfl_xor(cm.idx, m, 64);
        cm.visit(ov, oi);
      }
      if (lq == 0) {
        cmin[wv][16 * t + lr] = cm.v;
        carg[wv][16 * t + lr] = cm.idx;
      }
    }
    __syncthreads();
    if (tid < kGGroup) {
      GMin cm;
#pragma unroll
      for (int w = 0; w < NW; w++) cm.visit(cmin[w][tid], carg[w][tid]);
      const size_t o = ((size_t)f * a.n_qtiles + qt) * a.Lpad + g0 + tid;  // g0 + tid < Lpad
      a.pp_min[o] = cm.v;
      a.pp_arg[o] = cm.idx;
    }
  }

  // per keypoint: across the 16 lanes of the row, once
#pragma unroll
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int m = 1; m <= 8; m <<= 1) {
      const double ob = shfl_xor_f64(kb[r].best, m), os = shfl_xor_f64(kb[r].second, m);
      const int oi = __shfl_xor(kb[r].idx, m, 64);
      kb[r].merge(ob, os, oi);
    }
    if (lr == 0) {
      const size_t o = ((size_t)f * a.max_chunks + chunk) * a.Kpad + q0 + 16 * wv + lq + 4 * r;
      a.pk_best[o] = kb[r].best;
      a.pk_second[o] = kb[r].second;
      a.pk_arg[o] = kb[r].idx;
    }
  }
}

// blocks [0, Kpad / NW): one wave per keypoint folds its per-chunk partials, the lanes striding over the chunks;
// the blocks after them: one thread per local point folds its per-query-tile partials
__global__ __launch_bounds__(T) void lmap_gfold_kernel(GArgs a, int n_local, int n_chunks) {
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int n1 = a.n1c[f];
  const int kblocks = a.Kpad / NW;
  if ((int)blockIdx.x < kblocks) {
    const int i = blockIdx.x * NW + (tid >> 6);
    if (i >= n1) return;  // wave-uniform; no barrier in this kernel
    GBest b;
    const size_t o = (size_t)f * a.max_chunks * a.Kpad + i;
    for (int c = lane; c < n_chunks; c += 64)
      b.merge(a.pk_best[o + (size_t)c * a.Kpad], a.pk_second[o + (size_t)c * a.Kpad], a.pk_arg[o + (size_t)c * a.Kpad]);
#pragma unroll
    for (int m = 1; m <= 32; m <<= 1) {
      const double ob = shfl_xor_f64(b.best, m), os = shfl_xor_f64(b.second, m);
      const int oi = __shfl_xor(b.idx, m, 64);
      b.merge(ob, os, oi);
    }
    if (lane == 0) {
      const size_t ok = (size_t)f * a.K + i;
      a.arg[ok] = b.idx == INT_MAX ? -1 : b.idx;
      a.best[ok] = b.best;
      a.second[ok] = b.second;
    }
    return;
  }
  const int p = ((int)blockIdx.x - kblocks) * T + tid;
  if (p >= n_local) return;
  const int nqt = (n1 + kGQTile - 1) / kGQTile;  // the query tiles the search ran
  GMin m;
  const size_t o = (size_t)f * a.n_qtiles * a.Lpad + p;
  for (int q = 0; q < nqt; q++) m.visit(a.pp_min[o + (size_t)q * a.Lpad], a.pp_arg[o + (size_t)q * a.Lpad]);
  const int kb = m.idx == INT_MAX ? -1 : m.idx;
  a.kbest[(size_t)f * a.L + p] = kb;
  a.o_kbest[(size_t)f * a.L + p] = kb;  // host-mapped: coalesced, once
}

__global__ __launch_bounds__(T) void lmap_gmerge_kernel(GArgs a, int n_local) {
  __shared__ int wpass[NW], wmatch[NW];
  const int f = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int K = a.K, n1 = a.n1c[f];
  const size_t ok = (size_t)f * K, ol = (size_t)f * a.L;

  // pass, mutual, and the matches in keypoint order: wave w owns the w-th contiguous quarter of the keypoints
  const int span = (n1 + NW * 64 - 1) / (NW * 64) * 64;
  const int w0 = wv * span < n1 ? wv * span : n1;
  const int w1 = w0 + span < n1 ? w0 + span : n1;
  int npass = 0, nmatch = 0;
  for (int c = w0; c < w1; c += 64) {
    const int i = c + lane;
    int mt = -1;
    bool pass = false;
    if (i < w1) {
      const int ar = a.arg[ok + i];
      pass = ar >= 0 && global_pass(a.best[ok + i], a.second[ok + i], a.max_distance, a.max_ratio);
      if (pass && (!a.mutual || a.kbest[ol + ar] == i)) mt = ar;
      a.match[ok + i] = mt;
    }
    npass += __popcll(__ballot(pass));
    nmatch += __popcll(__ballot(mt >= 0));
  }
  if (lane == 0) {
    wpass[wv] = npass;
    wmatch[wv] = nmatch;
  }
  __syncthreads();
  int base = 0, n_pass = 0, n_matched = 0;
#pragma unroll
  for (int w = 0; w < NW; w++) {
    if (w < wv) base += wmatch[w];
    n_pass += wpass[w];
    n_matched += wmatch[w];
  }
  for (int c = w0; c < w1; c += 64) {
    const int i = c + lane;
    const bool m = i < w1 && a.match[ok + i] >= 0;
    const unsigned long long bal = __ballot(m);
    if (m) a.m_kp[ok + base + wave::lanes_below(bal)] = i;
    base += __popcll(bal);
  }
  __syncthreads();

  // the results go to host-mapped memory last, in bulk
  const GParam& P = a.params[f];
  for (int i = tid; i < n1; i += T) {
    a.o_arg[ok + i] = a.arg[ok + i];
    a.o_best[ok + i] = a.best[ok + i];
    a.o_second[ok + i] = a.second[ok + i];
    a.o_match[ok + i] = a.match[ok + i];
  }
  for (int j = tid; j < n_matched; j += T) {
    const int i = a.m_kp[ok + j], p = a.match[ok + i];
    const double* r = P.feat + RSPL_FEATURE_ROWS * (size_t)i;
    a.o_m_kp[ok + j] = i;
    a.o_m_local[ok + j] = p;
    a.o_m_id[ok + j] = a.local_id[p];
    a.o_m_pos[3 * (ok + j)] = a.local_pos[3 * (size_t)p];
    a.o_m_pos[3 * (ok + j) + 1] = a.local_pos[3 * (size_t)p + 1];
    a.o_m_pos[3 * (ok + j) + 2] = a.local_pos[3 * (size_t)p + 2];
    a.o_m_xy[2 * (ok + j)] = r[1];
    a.o_m_xy[2 * (ok + j) + 1] = r[2];
  }
  if (tid == 0) {
    GOut* o = a.out + f;
    o->n1 = n1;
    o->n_local = n_local;
    o->n_pass = n_pass;
    o->n_matched = n_matched;
  }
}

}  // namespace

hipError_t global_search(const GArgs& a, int batch, int n_local, hipStream_t s) {
  lmap_gpack_kernel<<<dim3(a.Kpad / NW, batch), T, 0, s>>>(a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int n_chunks = (n_local + a.chunk_rows - 1) / a.chunk_rows;  // <= max_chunks: n_local <= L
  if (n_local > 0) {
    const int padded = (n_chunks + kXcds - 1) / kXcds * kXcds;
    lmap_gsearch_kernel<<<dim3(padded * a.n_qtiles, batch), T, 0, s>>>(a, n_local);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  lmap_gfold_kernel<<<dim3(a.Kpad / NW + (n_local + T - 1) / T, batch), T, 0, s>>>(a, n_local, n_chunks);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  lmap_gmerge_kernel<<<batch, T, 0, s>>>(a, n_local);
  return hipGetLastError();
}

}  // namespace lmap
}  // namespace rspl
