#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rspl {
namespace sg {

// C[m][n] = epi(alpha * sum_k A[m][k] B[k][n] + bias[n]) for m < M, n < N, per batch z.
//   A columns [0, ksplit) come from A, [ksplit, K) from A2 (both row stride lda).
//   B is [K][N] (ldb) or, with b_nt, [N][K] (ldb).
//   epi: 0 = none, 1 = ReLU, 2 = residual (C += result).
//   mcount / ncount (device, may be null) override M / N per batch.
struct GemmArgs {
  const float* A;
  const float* A2;
  int lda, ksplit;
  const float* B;
  int ldb, b_nt;
  const float* bias;
  float* C;
  int ldc;
  int M, N, K;
  float alpha;
  int epi;
  long long sA, sB, sC;
  const int* mcount;
  const int* ncount;
  const _Float16* hB;  // RSPL_PREC_FP16: weights as fp16 [N][K] (k contiguous), row stride ldbh
  int ldbh;
  int count_stride;  // ints between consecutive batches in mcount/ncount
};

// fp16 GEMM (RSPL_PREC_FP16, final_proj): C32 = A B^T + bias, A [M][K] fp16 (columns [ksplit, K)
// from A2 when set), B [N][K] fp16 (the transposed weights), K <= 512 and a multiple of 64.
struct GemmHArgs {
  const _Float16* A;
  const _Float16* A2;
  int lda, lda2, ksplit;
  const _Float16* B;
  int ldb;
  const float* bias;
  int M, N, K;
  float* C32;
  int ldc32;
};


// One fused AttentionalGNN layer (fp16 engine): attention -> [x | message] MLP -> residual ->
// the next layer's Q / K / V^T, per 32-token tile of one image (layer_kernel).  QK / Vt of the
// running layer are read (all tokens of the source image), the next layer's are written to the
// other buffer of the ping-pong pair.
struct LayerArgs {
  const _Float16* Qc;    // [T][256] q of this layer (head-contiguous), row-major
  const _Float16* Kc;    // k of this layer, MFMA-fragment order per (set, head, 32-key tile, k-step)
  const _Float16* Vc;    // v of this layer, fragment order per (set, head, key tile, d-half, key-half)
  _Float16* Qn;          // the next layer's (written unless last)
  _Float16* Kn;
  _Float16* Vn;
  float* X;              // [T][256] fp32 residual stream
  _Float16* Xh;          // [T][256] fp16 shadow
  const _Float16* W1;    // mlp.0 (merge folded in), [512 n][512 k] in B-fragment order (to_frag)
  const float* b1;
  const _Float16* W2;    // mlp.3 [256][512], fragment order
  const float* b2;
  const _Float16* Wq;    // next layer's q | k | v [768][256] (head-contiguous rows), fragment order
  const float* bq;
  const int* n0;
  const int* n1;
  int nmax, nt;          // tokens per image set; 32-key tiles per set in Kc / Vc (ldv / 32)
  int cross, last;
  int qkv_only;          // prologue: only phase (4) from the current x (layer 0's q / k / v)
  int nsets, xps, tpx;   // set by gnn_layer: token sets, XCDs per set (0 = plain grid), tiles per XCD
};

struct PrepArgs {
  const double* f0;   // [B][stride][259]
  const double* f1;
  const int* n0;      // device counts [B]
  const int* n1;
  int stride;         // features per batch entry
  int normalize;      // apply PointMatching::NormalizeKeypoints
  int width, height;
  int nmax;
  float* kin;         // [B][2][nmax][16] keypoint-encoder input (x, y, score, 0...)
  float* X;           // [B][2][nmax][256] descriptors
  int B;
};

struct AttnArgs {
  const float* qkv;   // [B][2][nmax][768] = Q | K | V, head-contiguous channels
  float* O;           // [B][2][nmax][256]
  const int* n0;
  const int* n1;
  int nmax;
  int cross;          // 0: self (source = same image), 1: cross
};

struct BinsArgs {
  float* cpl;         // [B][(nmax+1)^2], row stride nmax+1
  const int* n0;
  const int* n1;
  const float* alpha; // bin_score (device scalar)
  int nmax;
};

struct SinkArgs {
  const float* cpl;   // couplings [B][ld*ld]
  float* Z;           // [B][ld*ld]
  float* cplT;        // [B][ld*ld] transposed column slabs (scratch; only when the slabs exceed LDS)
  unsigned long long* ug;  // [B][ld] tagged u granules {f32 bits, tag}; scaling form: [B][2][G][ld] partial sums;
                           // wide kernel: its hop-1 buffers (SinkPlan::ug_granules in all)
  unsigned long long* vg;  // [B][ld] tagged v granules; wide kernel: its hop-2 buffers
  unsigned seq;       // per-call tag base (never 0; granules start zeroed)
  unsigned spin_limit;  // bounded polls per granule before the exchange is declared timed out
  int inject;         // debug: workgroup 0 of pair 0 reports a timeout at iteration 0
  unsigned* err;      // [B] sticky timeout flags (host-mapped)
  const int* n0;
  const int* n1;
  // nmax, iters and sleep keep the kernarg offsets they were tuned at (80, 88, 96 of 112 bytes): packed, the
  // scaling-form kernels load and schedule differently and the Sinkhorn stage measured 1.4 % slower at C3.  The
  // reserved words are never read.
  int nmax, reserved0, iters, reserved1;
  int sleep;          // scaling-form kernels: s_sleep(1) units between re-polls (run_sinkhorn: 1)
  int reserved2[2];
};
static_assert(sizeof(SinkArgs) == 112 && offsetof(SinkArgs, nmax) == 80 && offsetof(SinkArgs, sleep) == 96,
              "SinkArgs: kernarg layout the Sinkhorn kernels were tuned at");

// Which Sinkhorn kernel a handle runs, decided once at create (sinkhorn_plan) and handed to every launch.
//   Slab / SlabScratch: sinkhorn_kernel, row and column slabs in LDS / read from global (cpl, cplT)
//   Sc / Sc10: sinkhorn_sc_kernel, nmax + 1 <= 448 (rpw 8, 4, 2 or 1 rows per wave) / <= 640 (rpw 3)
//   Wide: sinkhorn_w_kernel, 640 < nmax + 1 <= 2112
enum class SinkKind { Slab, SlabScratch, Sc, Sc10, Wide };
struct SinkPlan {
  SinkKind kind;
  int G;    // workgroups per pair
  int rpw;  // rows per wave of the scaling-form kernels (0: slab kernel)
  size_t ug_granules, vg_granules;  // exchange buffers of the handle (all max_batch pairs)
};
// kind_override: nullptr / "sc" / "slab" (RSPL_SG_SINK); G_override: 0 or the workgroups per pair (RSPL_SG_SINK_G),
// which applies to Sc, Sc10 and an explicit "slab".  Pure host arithmetic.  False: max_batch exceeds what ncu CUs
// keep co-resident.
bool sinkhorn_plan(int nmax, int B, int ncu, const char* kind_override, int G_override, SinkPlan* out);

struct DecodeArgs {
  const float* Z;     // [B][ld*ld]
  const int* n0;
  const int* n1;
  int nmax;
  int* max0;          // [B][nmax]
  float* val0;
  int* max1;
  int32_t* idx0;      // [B][nmax]
  int32_t* idx1;
  double* ms0;
  double* ms1;
  float threshold;
};

hipError_t gemm(const GemmArgs& a, int batch, hipStream_t s);
// Wt[n][k] = (fp16) W[k][n] for a [K][N] fp32 weight (one-time, at create)
hipError_t to_half_t(const float* W, int K, int N, _Float16* Wt, hipStream_t s);
hipError_t to_frag(const _Float16* Wt, int N, int K, _Float16* out, hipStream_t s);
hipError_t gemm_h(const GemmHArgs& a, hipStream_t s);
hipError_t gnn_layer(const LayerArgs& a, int B, hipStream_t s);
// fp32 -> fp16, n elements
hipError_t to_half(const float* x, _Float16* y, size_t n, hipStream_t s);
hipError_t prep(const PrepArgs& a, hipStream_t s);
hipError_t attention(const AttnArgs& a, int B, hipStream_t s);
hipError_t bins(const BinsArgs& a, int B, hipStream_t s);
// t0 / t1 (may be null): events stamped with the kernel's own start / end (hipExtLaunchKernelGGL)
// hipErrorInvalidValue if the plan's G does not fit the kernel its kind names (nothing is launched)
hipError_t sinkhorn(const SinkArgs& a, const SinkPlan& plan, int B, hipStream_t s, hipEvent_t t0 = nullptr,
                    hipEvent_t t1 = nullptr);
hipError_t decode(const DecodeArgs& a, int B, hipStream_t s);

}  // namespace sg
}  // namespace rspl
