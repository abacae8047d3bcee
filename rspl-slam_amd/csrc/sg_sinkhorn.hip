// SuperGlue optimal-transport tail on gfx950 (CDNA4): dustbins, log-optimal-transport (three Sinkhorn kernel
// families and the plan that chooses among them) and decode.  Launchers follow their kernels.
//
// Reference semantics (convert2onnx/superglue.py; src/super_glue.cpp):
//   log_optimal_transport :176-205, decode (argmax / mutual / exp / 0.2) super_glue.cpp:258-367.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstring>

#include "sg_kernels.hpp"

namespace rspl {
namespace sg {

// ---------------------------------------------------------------------------
// Dustbin couplings (superglue.py:191-196): column n, row m and the corner = bin_score.
// ---------------------------------------------------------------------------
__global__ void bins_kernel(BinsArgs a) {
  const int p = blockIdx.y;
  const int m = a.n0[p], n = a.n1[p], ld = a.nmax + 1;
  float* C = a.cpl + (size_t)p * ld * ld;
  const float al = *a.alpha;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= m + n; i += gridDim.x * blockDim.x) {
    if (i < m) C[(size_t)i * ld + n] = al;        // bins0
    else C[(size_t)m * ld + (i - m)] = al;         // bins1 + corner
  }
}

hipError_t bins(const BinsArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(bins_kernel, dim3((2 * a.nmax + 256) / 256, B), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Persistent log-domain Sinkhorn (superglue.py:176-205).
// G workgroups per pair (one per CU, co-resident); workgroup g owns a slab of
// rows AND a slab of columns of the couplings, both held in LDS when they fit
// (the column slab transposed, so both passes read contiguous LDS rows).
// Per iteration (u = log_mu - LSE_row(C + v); v = log_nu - LSE_col(C + u)):
//   row pass over the own rows -> publish own u as tagged granules -> all-gather u
//   column pass over the own columns -> publish own v -> all-gather v.
// Two hand-offs of (N+1) 8-byte granules {f32 bits, tag} per workgroup and
// iteration (a single write-through store each; no flags, no counters).  One
// buffer per vector suffices: a workgroup can only publish u(it+1) after every
// workgroup has published v(it), i.e. finished reading u(it).  Spins are bounded:
// a timed-out workgroup raises the pair's sticky error flag (host-mapped, read by
// rspl_sg_status) and leaves the loop, so every wave reaches the kernel end.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// DPP all-reduce over a wave64: quad swaps + half-row/row mirrors (in-row), then the
// four row results combined through readlane (uniform).  Fixed structure: deterministic.
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float rdlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = fmaxf(v, dppf<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dppf<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dppf<0x141>(v));  // row_half_mirror
  v = fmaxf(v, dppf<0x140>(v));  // row_mirror
  return fmaxf(fmaxf(rdlane(v, 0), rdlane(v, 16)), fmaxf(rdlane(v, 32), rdlane(v, 48)));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += dppf<0xB1>(v);
  v += dppf<0x4E>(v);
  v += dppf<0x141>(v);
  v += dppf<0x140>(v);
  return (rdlane(v, 0) + rdlane(v, 16)) + (rdlane(v, 32) + rdlane(v, 48));
}

__device__ __forceinline__ void st_sc1(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<unsigned*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float* p) {
  return __uint_as_float(
      __hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

constexpr int kSinkThreads = 1024;  // 16 waves: one wave per slab row / column in flight

__device__ __forceinline__ unsigned long long sk_granule(float v, unsigned tag) {
  return ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v);
}

// LSE over len values x[k] + w[k] (x, w in LDS, or x global) of NR rows at once by one wave
// (independent chains interleaved: the DPP reductions and exps of the rows overlap); rows of
// up to 512 values stay in registers between the max and the exp pass.  Lane-uniform results.
template <int NR>
__device__ __forceinline__ void wave_lse(const float* const (&x)[NR], const float* w, int len, int lane,
                                         float (&out)[NR]) {
  float mx[NR], s[NR];
  if (len <= 512) {
    float t[NR][8];
#pragma unroll
    for (int r = 0; r < NR; r++)
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const int j = lane + 64 * q;
        t[r][q] = j < len ? x[r][j] + w[j] : -INFINITY;
      }
#pragma unroll
    for (int r = 0; r < NR; r++) {
      mx[r] = t[r][0];
#pragma unroll
      for (int q = 1; q < 8; q++) mx[r] = fmaxf(mx[r], t[r][q]);
    }
#pragma unroll
    for (int r = 0; r < NR; r++) mx[r] = wave_max_dpp(mx[r]);
#pragma unroll
    for (int r = 0; r < NR; r++) {
      s[r] = 0.f;
#pragma unroll
      for (int q = 0; q < 8; q++) s[r] += (lane + 64 * q) < len ? expf(t[r][q] - mx[r]) : 0.f;
    }
  } else {
#pragma unroll
    for (int r = 0; r < NR; r++) mx[r] = -INFINITY;
    for (int j0 = 0; j0 < len; j0 += 512)
#pragma unroll
      for (int r = 0; r < NR; r++)
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int j = j0 + lane + 64 * q;
          if (j < len) mx[r] = fmaxf(mx[r], x[r][j] + w[j]);
        }
#pragma unroll
    for (int r = 0; r < NR; r++) {
      mx[r] = wave_max_dpp(mx[r]);
      s[r] = 0.f;
    }
    for (int j0 = 0; j0 < len; j0 += 512)
#pragma unroll
      for (int r = 0; r < NR; r++)
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int j = j0 + lane + 64 * q;
          if (j < len) s[r] += expf(x[r][j] + w[j] - mx[r]);
        }
  }
#pragma unroll
  for (int r = 0; r < NR; r++) s[r] = wave_sum_dpp(s[r]);
#pragma unroll
  for (int r = 0; r < NR; r++) out[r] = logf(s[r]) + mx[r];
}

// One LSE pass over the n rows of a slab (stride ld) by the workgroup's waves: wave wv takes rows
// wv and wv + NW together.  Lane 0 of the owning wave gets each row's LSE in fn(row, lse).
template <typename F>
__device__ __forceinline__ void slab_lse(const float* slab, int ld, const float* w, int len, int n, int wv, int lane,
                                         F&& fn) {
  constexpr int NW = kSinkThreads / 64;
  for (int r = wv; r < n; r += 2 * NW) {
    if (r + NW < n) {
      const float* const xs[2] = {slab + (size_t)r * ld, slab + (size_t)(r + NW) * ld};
      float o[2];
      wave_lse<2>(xs, w, len, lane, o);
      fn(r, o[0]);
      fn(r + NW, o[1]);
    } else {
      const float* const xs[1] = {slab + (size_t)r * ld};
      float o[1];
      wave_lse<1>(xs, w, len, lane, o);
      fn(r, o[0]);
    }
  }
}

// All-gather of a vector published as tagged granules: dst[j] for j in [0, len) outside the
// caller's own range [o0, o1).  Every thread polls its granules (all loads in flight, only
// the stale ones re-read), bounded by spin_limit.  Returns true on timeout.
__device__ __forceinline__ bool sk_gather(const unsigned long long* src, float* dst, int len, int o0, int o1,
                                          unsigned tag, unsigned spin_limit) {
  bool timed_out = false;
  for (int j = threadIdx.x; j < len; j += kSinkThreads) {
    if (j >= o0 && j < o1) continue;
    unsigned long long gv = __hip_atomic_load(src + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    while ((unsigned)(gv >> 32) != tag) {
      if (++spins > spin_limit) {
        timed_out = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      gv = __hip_atomic_load(src + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    dst[j] = __uint_as_float((unsigned)gv);
  }
  return timed_out;
}

template <bool SLAB_IN_LDS>
__global__ __launch_bounds__(kSinkThreads) void sinkhorn_kernel(SinkArgs a) {
  extern __shared__ float sm[];
  const int p = blockIdx.y, g = blockIdx.x, G = gridDim.x;
  const int m = a.n0[p], n = a.n1[p];
  if (m <= 0 || n <= 0) return;
  const int R = m + 1, Cc = n + 1, ld = a.nmax + 1, ldp = (ld + 3) & ~3;
  const int rs = (R + G - 1) / G, cs = (Cc + G - 1) / G;
  const int r0 = min(R, g * rs), nr = min(R, r0 + rs) - r0;
  const int c0 = min(Cc, g * cs), nc = min(Cc, c0 + cs) - c0;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* Cg = a.cpl + (size_t)p * ld * ld;
  float* u = sm;                                   // [ld] full u
  float* v = u + ldp;                              // [ld] full v
  int* flag = reinterpret_cast<int*>(v + ldp);     // [2] timeout broadcast: u exchange, v exchange
  float* Rs;                                       // [nr][ld] own rows
  float* Cs;                                       // [nc][ld] own columns, transposed
  if constexpr (SLAB_IN_LDS) {
    Rs = v + ldp + 4;
    Cs = Rs + (size_t)rs * ld;
  } else {  // slabs too large for LDS: rows read in place, columns from a transposed scratch copy
    Rs = const_cast<float*>(Cg) + (size_t)r0 * ld;
    Cs = a.cplT + (size_t)p * ld * ld + (size_t)c0 * ld;
  }
  if constexpr (SLAB_IN_LDS) {
    for (int i = tid; i < nr * Cc; i += kSinkThreads) {
      const int r = i / Cc, j = i - r * Cc;
      Rs[r * ld + j] = Cg[(size_t)(r0 + r) * ld + j];
    }
  }
  if (nc > 0)
    for (int i = tid; i < R * nc; i += kSinkThreads) {  // consecutive threads: consecutive columns of a row
      const int r = i / nc, c = i - r * nc;
      Cs[(size_t)c * ld + r] = Cg[(size_t)r * ld + c0 + c];
    }
  for (int j = tid; j < Cc; j += kSinkThreads) v[j] = 0.f;
  for (int j = tid; j < R; j += kSinkThreads) u[j] = 0.f;  // iters == 0: Z = C - norm (u = v = 0)
  // log_mu / log_nu (superglue.py:198-200), float arithmetic as the module
  const float fm = (float)m, fn = (float)n;
  const float norm = -logf(fm + fn);
  const float lmu_bin = logf(fn) + norm, lnu_bin = logf(fm) + norm;
  if (tid < 2) flag[tid] = 0;
  __syncthreads();  // also orders the transposed scratch copy (workgroup-private) before its reads
  unsigned long long* ug = a.ug + (size_t)p * ld;
  unsigned long long* vg = a.vg + (size_t)p * ld;
  // one flag slot per exchange: a slot is rewritten only after a barrier every thread passes
  // after reading it, so all threads take the same branch
  bool failed = false;
  for (int it = 0; it < a.iters; it++) {
    const unsigned tag = (a.seq << 12) | (unsigned)(it + 1);
    // u_i = log_mu_i - LSE_j(C_ij + v_j), own rows, one wave per row
    slab_lse(Rs, ld, v, Cc, nr, wv, lane, [&](int r, float lse) {
      if (lane == 0) {
        const float ui = ((r0 + r) < m ? norm : lmu_bin) - lse;
        u[r0 + r] = ui;
        __hip_atomic_store(ug + r0 + r, sk_granule(ui, tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    });
    bool to = sk_gather(ug, u, R, r0, r0 + nr, tag, a.spin_limit);
    if (a.inject && p == 0 && g == 0 && it == 0) to = true;  // fault injection (rspl_sg_debug_inject)
    if (to) flag[0] = 1;
    __syncthreads();
    if (flag[0]) { failed = true; break; }
    // v_j = log_nu_j - LSE_i(C_ij + u_i), own columns, one wave per column
    slab_lse(Cs, ld, u, R, nc, wv, lane, [&](int c, float lse) {
      if (lane == 0) {
        const float vj = ((c0 + c) < n ? norm : lnu_bin) - lse;
        v[c0 + c] = vj;
        __hip_atomic_store(vg + c0 + c, sk_granule(vj, tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    });
    if (sk_gather(vg, v, Cc, c0, c0 + nc, tag, a.spin_limit)) flag[1] = 1;
    __syncthreads();
    if (flag[1]) { failed = true; break; }
  }
  if (failed) {
    if (tid == 0) __hip_atomic_store(a.err + p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  // Z = ((couplings + u) + v) - norm (superglue.py:203, :219), own rows
  float* Z = a.Z + (size_t)p * ld * ld;
  for (int i = tid; i < nr * Cc; i += kSinkThreads) {
    const int r = i / Cc, j = i - r * Cc;
    Z[(size_t)(r0 + r) * ld + j] = ((Rs[(size_t)r * ld + j] + u[r0 + r]) + v[j]) - norm;
  }
}

// ---------------------------------------------------------------------------
// Row-block layout of the register-resident Sinkhorn (superglue.py:176-205), one exchange per
// iteration.  G workgroups per pair; workgroup g holds WHOLE rows [r0, r0 + nr) of the couplings in
// registers: wave w owns rows w + 16 k (k < RPW), lane L columns L + 64 q (q < kRbQ).
// Since every wave holds full rows and a replicated v, the row pass
//   u_i = log_mu_i - LSE_j(C_ij + v_j)
// is wave-local (no barrier, no exchange).  The column pass
//   v_j = log_nu_j - LSE_i(C_ij + u_i)
// reduces each lane's columns over its wave's rows in registers, the 16 waves through LDS,
// and the G workgroups through one all-gather of per-column partials (tagged 8-byte
// granules, double-buffered by iteration parity).  Every workgroup merges the G partials
// in the same order (g = 0 .. G-1), so all hold a bit-identical v.  Parity reuse is safe:
// workgroup g publishes iteration it + 2 into slot (it & 1) only after every peer has
// published it + 1, which each peer does only after reading all of iteration it.
// (Rounds 2-4 ran these passes in the log domain, an exp per element and iteration; the
// scaling form below replaced that kernel.)
// ---------------------------------------------------------------------------
constexpr int kRbQ = 7;                 // 7 x 64 = 448 >= nmax + 1 columns per lane set
// exp for the LSE terms: FX = false -> expf; FX = true -> v_exp_f32 on the split product
// d*log2(e) = a + e (a rounded, e its fma residual) corrected to first order: 2^a (1 + e ln 2);
// arguments are <= 0 here (shifted by the max), below -150 the result is 0 as with expf
template <bool FX>
__device__ __forceinline__ float sk_exp(float d) {
  if constexpr (!FX) {
    return expf(d);
  } else {
    d = d < -150.f ? -150.f : d;  // -inf (masked rows / columns) -> exactly 0 below; NaN stays NaN
    const float a = d * 1.44269504f;
    const float e = fmaf(d, 1.44269504f, -a) + d * 1.9259630e-8f;
    const float r = __builtin_amdgcn_exp2f(a);
    return fmaf(r, e * 0.693147181f, r);
  }
}

// ---------------------------------------------------------------------------
// Scaling-form Sinkhorn (the default for nmax + 1 <= 640): the same iterations as
// log_sinkhorn_iterations (superglue.py:176-183) written on the scalings U = exp(u - a),
// V = exp(v - b) of absorbed log potentials a, b (stabilised Sinkhorn):
//   K_ij = exp(C_ij + a_i + b_j)  (registers),   U_i = mu_i / sum_j K_ij V_j,
//   V_j = nu_j / sum_i K_ij U_i,   u = a + log U,   v = b + log V,
// so an iteration is two mat-vecs of register-resident K -- no exp per element.  Iteration 0's
// row pass runs in the log domain exactly as the module (max-shifted LSE, v = 0) and seeds a = u,
// which bounds K by mu (<= 1).  A scaling that leaves [2^-60, 2^60] is absorbed into a / b and K
// is recomputed from C: rows per workgroup (a is workgroup-local), columns on every workgroup
// alike (V is bit-identical everywhere, so every workgroup decides the same).  Layout, exchange
// and determinism as the row-block layout above: G workgroups per pair hold whole rows (wave w rows
// w + 16 k, lane L columns L + 64 q), the row pass is wave-local, the column sums go through LDS
// across waves and ONE all-gather of per-column partial sums across workgroups per iteration,
// merged in the same order everywhere.  Z = ((C + u) + v) - norm from C re-read at the end.
// ---------------------------------------------------------------------------
// orders this wave's LDS writes before its later LDS reads
__device__ __forceinline__ void wave_barrier_lds() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int RPW, int GM, int Q>  // Q: 64-column lane sets (7: nmax + 1 <= 448, 10: <= 640)
__global__ __launch_bounds__(kSinkThreads) void sinkhorn_sc_kernel(SinkArgs a) {
  __shared__ float ps[16][Q * 64];   // per-wave column partial sums
  __shared__ float vs[Q * 64];       // merged V
  __shared__ int flag[4];               // 0: exchange timeout, 1: column absorb, 2 + (it & 1): row absorb
  __shared__ float as[16 * RPW];        // absorbed row potentials a (row wv + 16 k), read on absorption / at the end
  __shared__ float bs[Q * 64];       // absorbed column potentials b (identical on every workgroup)
  const int p = blockIdx.y, g = blockIdx.x, G = gridDim.x;
  const int m = a.n0[p], n = a.n1[p];
  if (m <= 0 || n <= 0) return;
  const int R = m + 1, Cc = n + 1, ld = a.nmax + 1;
  const int rs = (R + G - 1) / G;
  const int r0 = min(R, g * rs), nr = min(R, r0 + rs) - r0;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* Cg = a.cpl + (size_t)p * ld * ld;
  const int nk = min(RPW, max(0, (nr - wv + 15) / 16));  // the wave's rows inside the slab
  float x[RPW][Q];
#pragma unroll
  for (int k = 0; k < RPW; k++) {
    const int r = wv + 16 * k;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int j = lane + 64 * q;
      x[k][q] = (r < nr && j < Cc) ? Cg[(size_t)(r0 + r) * ld + j] : -INFINITY;
    }
  }
  // log_mu / log_nu (superglue.py:198-200), float arithmetic as the module; mu / nu = exp of them
  const float fm = (float)m, fn = (float)n;
  const float norm = -logf(fm + fn);
  const float lmu_bin = logf(fn) + norm, lnu_bin = logf(fm) + norm;
  const float mu_in = expf(norm), mu_bin = expf(lmu_bin), nu_bin = expf(lnu_bin);
  constexpr float kLo = 8.6736174e-19f, kHi = 1.1529215e18f;  // 2^-60, 2^60
  if (tid < 4) flag[tid] = 0;
  // iteration 0, row pass in the log domain (v = 0): a = u
  float ur[RPW];
  {
    float mx[RPW], sm[RPW];
#pragma unroll
    for (int k = 0; k < RPW; k++) {
      mx[k] = x[k][0];
#pragma unroll
      for (int q = 1; q < Q; q++) mx[k] = fmaxf(mx[k], x[k][q]);
    }
#pragma unroll
    for (int k = 0; k < RPW; k++) mx[k] = wave_max_dpp(mx[k]);
#pragma unroll
    for (int k = 0; k < RPW; k++) {
      sm[k] = 0.f;
      if (k < nk)
#pragma unroll
        for (int q = 0; q < Q; q++) sm[k] += sk_exp<true>(x[k][q] - mx[k]);
    }
#pragma unroll
    for (int k = 0; k < RPW; k++) sm[k] = wave_sum_dpp(sm[k]);
#pragma unroll
    for (int k = 0; k < RPW; k++) {
      const int r = wv + 16 * k;
      // (no iterations: u = v = 0, Z = C - norm as superglue.py:202-205 -- no seed)
      if (lane == 0)
        as[wv + 16 * k] = r < nr && a.iters > 0 ? ((r0 + r) < m ? norm : lmu_bin) - (logf(sm[k]) + mx[k]) : 0.f;
      ur[k] = 1.f;
    }
  }
  float vr[Q];
#pragma unroll
  for (int q = 0; q < Q; q++) {
    bs[lane + 64 * q] = 0.f;  // every wave writes the same zeros
    vr[q] = 1.f;
  }
  wave_barrier_lds();
  // K = exp(C + a + b), masked entries exactly 0
  auto build_k = [&](bool reload) {
#pragma unroll
    for (int k = 0; k < RPW; k++) {
      const int r = wv + 16 * k;
#pragma unroll
      for (int q = 0; q < Q; q++) {
        const int j = lane + 64 * q;
        const bool in = r < nr && j < Cc;
        const float c = reload ? (in ? Cg[(size_t)(r0 + r) * ld + j] : 0.f) : x[k][q];
        x[k][q] = in ? sk_exp<true>((c + as[wv + 16 * k]) + bs[j]) : 0.f;
      }
    }
  };
  build_k(false);
  __syncthreads();
  bool failed = false;
  for (int it = 0; it < a.iters; it++) {
    const unsigned tag = (a.seq << 12) | (unsigned)(it + 1);
    if (it > 0) {  // row pass: U_i = mu_i / sum_j K_ij V_j (wave-local)
      float sm[RPW];
#pragma unroll
      for (int k = 0; k < RPW; k++) {
        sm[k] = 0.f;
        if (k < nk)
#pragma unroll
          for (int q = 0; q < Q; q++) sm[k] = fmaf(x[k][q], vr[q], sm[k]);
      }
#pragma unroll
      for (int k = 0; k < RPW; k++) sm[k] = wave_sum_dpp(sm[k]);
      bool out = false;
#pragma unroll
      for (int k = 0; k < RPW; k++) {
        const int r = wv + 16 * k;
        ur[k] = r < nr ? ((r0 + r) < m ? mu_in : mu_bin) / sm[k] : 0.f;
        out |= r < nr && !(ur[k] >= kLo && ur[k] <= kHi);
      }
      if (out && lane == 0) flag[2 + (it & 1)] = 1;
    }
    // column partials over the wave's rows, then over the 16 waves
#pragma unroll
    for (int q = 0; q < Q; q++) {
      float cs = 0.f;
#pragma unroll
      for (int k = 0; k < RPW; k++)
        if (k < nk) cs = fmaf(x[k][q], ur[k], cs);
      ps[wv][lane + 64 * q] = cs;
    }
    __syncthreads();
    if (tid == 0) flag[2 + ((it + 1) & 1)] = 0;  // next iteration's row flag (its readers are past)
    unsigned long long* slot = a.ug + (size_t)(p * 2 + (it & 1)) * G * ld;
    // two adjacent lanes per column: lane `half` sums waves 8 half .. 8 half + 7 and polls the
    // peers h with (h & 1) == half; both lanes form the same total (fp addition commutes)
    // (more than 512 columns: every thread holds two column halves; both are published before
    // either is polled, so the exchange stays one round trip)
    constexpr int NP = (Q * 128 + kSinkThreads - 1) / kSinkThreads;
    float own2[NP];
#pragma unroll
    for (int u = 0; u < NP; u++) {
      const int tt = tid + u * kSinkThreads;
      own2[u] = 0.f;
      if (tt < 2 * Cc) {
        const int j = tt >> 1, half = tt & 1;
        float S = 0.f;
#pragma unroll
        for (int w = 0; w < 8; w++) S += ps[8 * half + w][j];
        own2[u] = S + __shfl_xor(S, 1);
        if (!half)
          __hip_atomic_store(slot + (size_t)g * ld + j, sk_granule(own2[u], tag), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      }
    }
#pragma unroll
    for (int u = 0; u < NP; u++) {
      const int tt = tid + u * kSinkThreads;
      if (tt >= 2 * Cc) continue;
      const int j = tt >> 1, half = tt & 1;
      const float own = own2[u];
      constexpr int GH = GM / 2;
      float l[GH];
      unsigned long long gv[GH];
      unsigned pend = 0;
#pragma unroll
      for (int k = 0; k < GH; k++) {
        const int h = 2 * k + half;
        l[k] = 0.f;
        if (h < G) {
          if (h == g) l[k] = own;
          else pend |= 1u << k;
        }
      }
      bool to = a.inject && p == 0 && g == 0 && it == 0;  // fault injection (rspl_sg_debug_inject)
      unsigned spins = 0;
      while (pend && !to) {
#pragma unroll
        for (int k = 0; k < GH; k++)
          if (pend >> k & 1)
            gv[k] = __hip_atomic_load(slot + (size_t)(2 * k + half) * ld + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < GH; k++)
          if ((pend >> k & 1) && (unsigned)(gv[k] >> 32) == tag) {
            l[k] = __uint_as_float((unsigned)gv[k]);
            pend &= ~(1u << k);
          }
        if (!pend) break;
        if (++spins > a.spin_limit) { to = true; break; }
        for (int z = 0; z < a.sleep; z++) __builtin_amdgcn_s_sleep(1);
      }
      if (to) flag[0] = 1;
      float T = 0.f;
#pragma unroll
      for (int k = 0; k < GH; k++) T += l[k];
      T = T + __shfl_xor(T, 1);
      const float V = (j < n ? mu_in : nu_bin) / T;  // nu_j = mu_in for j < n: exp(norm)
      if (!half) {
        vs[j] = V;
        if (!(V >= kLo && V <= kHi)) flag[1] = 1;
      }
    }
    __syncthreads();
    if (flag[0]) { failed = true; break; }
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int j = lane + 64 * q;
      vr[q] = j < Cc ? vs[j] : 1.f;
    }
    const bool col_abs = flag[1] != 0, row_abs = flag[2 + (it & 1)] != 0;
    if (col_abs || row_abs) {  // rare: absorb the scalings into the log potentials, rebuild K from C
      __syncthreads();  // no wave still reads as / bs of the current K
      if (row_abs) {
#pragma unroll
        for (int k = 0; k < RPW; k++) {
          if (lane == 0) as[wv + 16 * k] += logf(ur[k] > 0.f ? ur[k] : 1.f);
          ur[k] = 1.f;
        }
      }
      if (col_abs) {
        for (int j = tid; j < Q * 64; j += kSinkThreads) bs[j] += logf(vs[j] > 0.f && j < Cc ? vs[j] : 1.f);
#pragma unroll
        for (int q = 0; q < Q; q++) vr[q] = 1.f;
      }
      __syncthreads();
      build_k(true);
      __syncthreads();  // every thread has read flag[1] before it is cleared
      if (tid == 0) flag[1] = 0;
      __syncthreads();
    }
  }
  if (failed) {
    if (tid == 0) __hip_atomic_store(a.err + p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  // Z = ((couplings + u) + v) - norm (superglue.py:203, :219), own rows; u = a + log U, v = b + log V
  float* Z = a.Z + (size_t)p * ld * ld;
#pragma unroll
  for (int k = 0; k < RPW; k++) {
    const int r = wv + 16 * k;
    if (r >= nr) continue;
    const float u = as[wv + 16 * k] + logf(ur[k]);
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int j = lane + 64 * q;
      if (j < Cc) Z[(size_t)(r0 + r) * ld + j] = ((Cg[(size_t)(r0 + r) * ld + j] + u) + (bs[j] + logf(vr[q]))) - norm;
    }
  }
}

// ---------------------------------------------------------------------------
// Wide scaling-form Sinkhorn (640 < nmax + 1 <= 64 Q: C5's 2048 keypoints), the same iteration as
// sinkhorn_sc_kernel (K = exp(C + a + b) register resident for whole rows, plain sums, scalings absorbed
// into the log potentials outside [2^-60, 2^60]) on G = ceil(ld / (8 RPW)) workgroups of 512 threads per
// pair: wave w owns rows w + 8 k (k < RPW), lane L columns L + 64 q.  An all-gather of per-column
// partials would move G x ld granules into every workgroup per iteration (G ~ 65), so the column pass
// exchanges in TWO hops:
//   hop 1 (reduce-scatter): every workgroup publishes its partial sum of column j to the column's owner
//     o = j / cs (cs = ceil(ld / G) <= 64 columns per owner), laid out [parity][owner][source][cs] so an
//     owner's inputs are one contiguous run; the owner sums its columns over the G sources in a fixed
//     order (source subsets g = w (mod 8) per wave, then the 8 wave sums in wave order) and forms V_j;
//   hop 2 (broadcast): the owner publishes V_j, every workgroup reads all of V into LDS.
// Every workgroup therefore holds a bit-identical V (and takes the same column absorption decisions).
// Parity reuse: a workgroup writes hop 1 of iteration it + 2 only after reading all of V(it + 1), which
// an owner publishes only after it has read every hop-1 input of it + 1 (and of it before that); the
// owner writes V(it + 2) only after every source's hop 1 of it + 2, which follows their reads of V(it).
// ---------------------------------------------------------------------------
constexpr int kWThreads = 512;  // 8 waves: two per SIMD at <= 256 VGPRs, the partial-sum table fits LDS
constexpr int kWideRPW = 4, kWideQ = 33;  // 32 rows per workgroup, 2112 columns

static int sinkhorn_wide_groups(int nmax) { return (nmax + 1 + 8 * kWideRPW - 1) / (8 * kWideRPW); }
static bool sinkhorn_wide_ok(int nmax, int G) {
  const int ld = nmax + 1;
  return ld > 640 && ld <= kWideQ * 64 && G == sinkhorn_wide_groups(nmax) && (ld + G - 1) / G <= 64;
}
// exchange buffers in granules per pair: hop 1 [2][G][G][cs] (-> ug), hop 2 [2][G * cs] (-> vg)
static size_t sinkhorn_wide_hop1_len(int nmax) {
  const int ld = nmax + 1, G = sinkhorn_wide_groups(nmax), cs = (ld + G - 1) / G;
  return (size_t)2 * G * G * cs;
}
static size_t sinkhorn_wide_hop2_len(int nmax) {
  const int ld = nmax + 1, G = sinkhorn_wide_groups(nmax), cs = (ld + G - 1) / G;
  return (size_t)2 * G * cs;
}

template <int RPW, int Q>
__global__ __launch_bounds__(kWThreads) void sinkhorn_w_kernel(SinkArgs a) {
  constexpr int NW = kWThreads / 64;
  __shared__ float ps[NW][Q * 64];  // per-wave column partial sums
  __shared__ float vs[Q * 64];      // V (identical on every workgroup)
  __shared__ float bs[Q * 64];      // absorbed column potentials b
  __shared__ float as[NW * RPW];    // absorbed row potentials a (row wv + NW k)
  __shared__ float red[NW][64];     // owner: per-wave sums over its source subset
  __shared__ int flag[4];           // 0: exchange timeout, 1: column absorb, 2 + (it & 1): row absorb
  const int p = blockIdx.y, g = blockIdx.x, G = gridDim.x;
  const int m = a.n0[p], n = a.n1[p];
  if (m <= 0 || n <= 0) return;
  const int R = m + 1, Cc = n + 1, ld = a.nmax + 1;
  const int rs = NW * RPW, cs = (ld + G - 1) / G;
  const int r0 = min(R, g * rs), nr = min(R, r0 + rs) - r0;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* Cg = a.cpl + (size_t)p * ld * ld;
  const int nk = min(RPW, max(0, (nr - wv + NW - 1) / NW));  // the wave's rows inside the slab
  // row r of the slab into v[q] = C[r0 + r][lane + 64 q]: unconditional loads off one row pointer (the
  // row clamped into the matrix, the last lane set's column clamped to ld - 1), masked afterwards --
  // per-element conditional loads would keep an address per element live
  auto load_row = [&](int r, float (&v)[Q]) {
    const float* rp = Cg + (size_t)min(r0 + r, ld - 1) * ld;
#pragma unroll
    for (int q = 0; q < Q - 1; q++) v[q] = rp[lane + 64 * q];
    v[Q - 1] = rp[min(lane + 64 * (Q - 1), ld - 1)];
  };
  float x[RPW][Q];
#pragma unroll
  for (int k = 0; k < RPW; k++) {
    const int r = wv + NW * k;
    load_row(r, x[k]);
#pragma unroll
    for (int q = 0; q < Q; q++) x[k][q] = (r < nr && lane + 64 * q < Cc) ? x[k][q] : -INFINITY;
  }
  // log_mu / log_nu (superglue.py:198-200), float arithmetic as the module; mu / nu = exp of them
  const float fm = (float)m, fn = (float)n;
  const float norm = -logf(fm + fn);
  const float lmu_bin = logf(fn) + norm, lnu_bin = logf(fm) + norm;
  const float mu_in = expf(norm), mu_bin = expf(lmu_bin), nu_bin = expf(lnu_bin);
  constexpr float kLo = 8.6736174e-19f, kHi = 1.1529215e18f;  // 2^-60, 2^60
  if (tid < 4) flag[tid] = 0;
  // iteration 0, row pass in the log domain (v = 0): a = u
  float ur[RPW];
  {
    float mx[RPW], sm[RPW];
#pragma unroll
    for (int k = 0; k < RPW; k++) {
      mx[k] = x[k][0];
#pragma unroll
      for (int q = 1; q < Q; q++) mx[k] = fmaxf(mx[k], x[k][q]);
    }
#pragma unroll
    for (int k = 0; k < RPW; k++) mx[k] = wave_max_dpp(mx[k]);
#pragma unroll
    for (int k = 0; k < RPW; k++) {
      sm[k] = 0.f;
      if (k < nk)
#pragma unroll
        for (int q = 0; q < Q; q++) sm[k] += sk_exp<true>(x[k][q] - mx[k]);
    }
#pragma unroll
    for (int k = 0; k < RPW; k++) sm[k] = wave_sum_dpp(sm[k]);
#pragma unroll
    for (int k = 0; k < RPW; k++) {
      const int r = wv + NW * k;
      // (no iterations: u = v = 0, Z = C - norm as superglue.py:202-205 -- no seed)
      if (lane == 0)
        as[wv + NW * k] = r < nr && a.iters > 0 ? ((r0 + r) < m ? norm : lmu_bin) - (logf(sm[k]) + mx[k]) : 0.f;
      ur[k] = 1.f;
    }
  }
  for (int j = tid; j < Q * 64; j += kWThreads) {
    bs[j] = 0.f;
    vs[j] = 1.f;
  }
  __syncthreads();
  // K = exp(C + a + b), masked entries exactly 0
  auto build_k = [&](bool reload) {
#pragma unroll
    for (int k = 0; k < RPW; k++) {
      const int r = wv + NW * k;
      if (reload) load_row(r, x[k]);
      const float ak = as[wv + NW * k];
#pragma unroll
      for (int q = 0; q < Q; q++) {
        const int j = lane + 64 * q;
        const bool in = r < nr && j < Cc;
        x[k][q] = in ? sk_exp<true>((x[k][q] + ak) + bs[j]) : 0.f;
      }
    }
  };
  build_k(false);
  unsigned long long* h1 = a.ug + (size_t)p * 2 * G * G * cs;  // [2][owner][source][cs]
  unsigned long long* h2 = a.vg + (size_t)p * 2 * G * cs;      // [2][G * cs]
  const int c0 = g * cs, nc = max(0, min(Cc, c0 + cs) - c0);   // the columns this workgroup owns
  bool failed = false;
  for (int it = 0; it < a.iters; it++) {
    const unsigned tag = (a.seq << 12) | (unsigned)(it + 1);
    const int par = it & 1;
    if (it > 0) {  // row pass: U_i = mu_i / sum_j K_ij V_j (wave-local)
      float sm[RPW];
#pragma unroll
      for (int k = 0; k < RPW; k++) sm[k] = 0.f;
#pragma unroll
      for (int q = 0; q < Q; q++) {
        const float v = vs[lane + 64 * q];
#pragma unroll
        for (int k = 0; k < RPW; k++)
          if (k < nk) sm[k] = fmaf(x[k][q], v, sm[k]);
      }
#pragma unroll
      for (int k = 0; k < RPW; k++) sm[k] = wave_sum_dpp(sm[k]);
      bool out = false;
#pragma unroll
      for (int k = 0; k < RPW; k++) {
        const int r = wv + NW * k;
        ur[k] = r < nr ? ((r0 + r) < m ? mu_in : mu_bin) / sm[k] : 0.f;
        out |= r < nr && !(ur[k] >= kLo && ur[k] <= kHi);
      }
      if (out && lane == 0) flag[2 + (it & 1)] = 1;
    }
    // column partials over the wave's rows, then over the 8 waves
#pragma unroll
    for (int q = 0; q < Q; q++) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < RPW; k++)
        if (k < nk) s = fmaf(x[k][q], ur[k], s);
      ps[wv][lane + 64 * q] = s;
    }
    __syncthreads();
    if (tid == 0) flag[2 + ((it + 1) & 1)] = 0;  // next iteration's row flag (its readers are past)
    // hop 1: this workgroup's partial of column j to its owner
    for (int j = tid; j < Cc; j += kWThreads) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < NW; w++) s += ps[w][j];
      const int o = j / cs;
      __hip_atomic_store(h1 + (((size_t)par * G + o) * G + g) * cs + (j - o * cs), sk_granule(s, tag),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // owner: lane = owned column, wave wv sums the sources g' = wv, wv + 8, ... in order
    bool to = a.inject && p == 0 && g == 0 && it == 0;  // fault injection (rspl_sg_debug_inject)
    if (lane < nc) {
      constexpr int kSrc = 9;  // <= 9 sources per wave: G <= 72 (ld <= 2112 at 32 rows per workgroup)
      const unsigned long long* src = h1 + ((size_t)par * G + g) * G * cs + lane;
      float l[kSrc];
      unsigned long long gv[kSrc];
      unsigned pend = 0;
#pragma unroll
      for (int i = 0; i < kSrc; i++) {
        l[i] = 0.f;
        if (wv + NW * i < G) pend |= 1u << i;
      }
      unsigned spins = 0;
      while (pend && !to) {
#pragma unroll
        for (int i = 0; i < kSrc; i++)
          if (pend >> i & 1) gv[i] = __hip_atomic_load(src + (size_t)(wv + NW * i) * cs, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int i = 0; i < kSrc; i++)
          if ((pend >> i & 1) && (unsigned)(gv[i] >> 32) == tag) {
            l[i] = __uint_as_float((unsigned)gv[i]);
            pend &= ~(1u << i);
          }
        if (!pend) break;
        if (++spins > a.spin_limit) { to = true; break; }
        for (int z = 0; z < a.sleep; z++) __builtin_amdgcn_s_sleep(1);
      }
      float T = 0.f;
#pragma unroll
      for (int i = 0; i < kSrc; i++) T += l[i];
      red[wv][lane] = T;
    }
    if (to) flag[0] = 1;
    __syncthreads();
    if (wv == 0 && lane < nc) {
      float T = 0.f;
#pragma unroll
      for (int w = 0; w < NW; w++) T += red[w][lane];
      const int j = c0 + lane;
      const float V = (j < n ? mu_in : nu_bin) / T;  // nu_j = mu_in for j < n: exp(norm)
      __hip_atomic_store(h2 + (size_t)par * G * cs + j, sk_granule(V, tag), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    // hop 2: every column's V from its owner
    bool to2 = false;
    for (int j = tid; j < Cc; j += kWThreads) {
      const unsigned long long* q = h2 + (size_t)par * G * cs + j;
      unsigned long long gv = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unsigned spins = 0;
      while ((unsigned)(gv >> 32) != tag && !to2) {
        if (++spins > a.spin_limit) { to2 = true; break; }
        for (int z = 0; z < a.sleep; z++) __builtin_amdgcn_s_sleep(1);
        gv = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const float V = __uint_as_float((unsigned)gv);
      vs[j] = V;
      if (!(V >= kLo && V <= kHi)) flag[1] = 1;
    }
    if (to2) flag[0] = 1;
    __syncthreads();
    if (flag[0]) { failed = true; break; }
    const bool col_abs = flag[1] != 0, row_abs = flag[2 + (it & 1)] != 0;
    if (col_abs || row_abs) {  // rare: absorb the scalings into the log potentials, rebuild K from C
      if (row_abs) {
#pragma unroll
        for (int k = 0; k < RPW; k++) {
          if (lane == 0) as[wv + NW * k] += logf(ur[k] > 0.f ? ur[k] : 1.f);
          ur[k] = 1.f;
        }
      }
      if (col_abs)
        for (int j = tid; j < Q * 64; j += kWThreads) {
          bs[j] += logf(vs[j] > 0.f && j < Cc ? vs[j] : 1.f);
          vs[j] = 1.f;
        }
      __syncthreads();
      build_k(true);
      __syncthreads();  // every thread has read flag[1] before it is cleared
      if (tid == 0) flag[1] = 0;
      __syncthreads();
    }
  }
  if (failed) {
    if (tid == 0) __hip_atomic_store(a.err + p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  // Z = ((couplings + u) + v) - norm (superglue.py:203, :219), own rows; u = a + log U, v = b + log V
  float* Z = a.Z + (size_t)p * ld * ld;
#pragma unroll
  for (int k = 0; k < RPW; k++) {
    const int r = wv + NW * k;
    if (r >= nr) continue;
    const float u = as[wv + NW * k] + logf(ur[k]);
    float c[Q];
    load_row(r, c);
    float* zr = Z + (size_t)(r0 + r) * ld;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int j = lane + 64 * q;
      if (j < Cc) zr[j] = ((c[q] + u) + (bs[j] + logf(vs[j]))) - norm;
    }
  }
}

// (sinkhorn_sc_kernel and sinkhorn_w_kernel repeat ~150 lines of each other on purpose: both already spill, and sharing
// their bodies moves register allocation -- merging them needs a tuning pass of its own.)

// ---------------------------------------------------------------------------
// The plan: which kernel a handle of (nmax, B) runs on ncu CUs, on how many workgroups per pair, and the exchange
// buffers that takes.  All B * G workgroups must be co-resident (one per CU).
// ---------------------------------------------------------------------------
constexpr size_t kSinkLdsMax = 150 * 1024;  // slab budget per workgroup (160 KB LDS per CU)

// LDS bytes of one slab-kernel workgroup (with or without the row / column slabs)
static size_t sinkhorn_lds_bytes(int nmax, int G, bool slabs) {
  const size_t ld = nmax + 1, ldp = (ld + 3) & ~size_t(3), per = (ld + G - 1) / G;
  return sizeof(float) * (2 * ldp + 4 + (slabs ? 2 * per * ld : 0));
}

// rows per wave of sinkhorn_sc_kernel<RPW, GM, kRbQ> for G workgroups per pair (0: no instantiation fits)
static int sinkhorn_rb_rpw(int nmax, int G) {
  const int ld = nmax + 1, rs = (ld + G - 1) / G;
  if (ld > kRbQ * 64 || G < 1) return 0;
  if (G <= 4 && rs <= 16 * 8) return 8;
  if (G <= 8 && rs <= 16 * 4) return 4;
  if (G <= 16 && rs <= 16 * 2) return 2;
  if (G <= 32 && rs <= 16) return 1;
  return 0;
}

// sinkhorn_sc_kernel<3, 16, 10> (448 < nmax + 1 <= 640, three rows per wave): G <= 16 workgroups of <= 48 rows
constexpr int kSc10RPW = 3;
static bool sinkhorn_sc10_ok(int nmax, int G) {
  const int ld = nmax + 1;
  return ld > kRbQ * 64 && ld <= 640 && G >= 1 && G <= 16 && (ld + G - 1) / G <= kSc10RPW * 16;
}

bool sinkhorn_plan(int nmax, int B, int ncu, const char* kind_override, int G_override, SinkPlan* out) {
  const int ld = nmax + 1, gmax = std::max(1, ncu / B);
  const bool slab = kind_override && !strcmp(kind_override, "slab");
  SinkPlan pl{};
  pl.ug_granules = pl.vg_granules = (size_t)B * ld;
  // the slab kernel: ~kRows rows + columns per workgroup, and at least enough workgroups that both slabs fit LDS
  constexpr int kRows = 9;  // 45 workgroups per pair at N = 400 (round-2 A/B: 32 vs 48)
  int G = std::max(1, (ld + kRows - 1) / kRows);
  while (G < ld && sinkhorn_lds_bytes(nmax, G, true) > kSinkLdsMax) G++;
  if (slab && G_override) G = G_override;
  pl.G = std::min(G, gmax);
  pl.kind = sinkhorn_lds_bytes(nmax, pl.G, true) > kSinkLdsMax ? SinkKind::SlabScratch : SinkKind::Slab;
  if (!slab) {  // the scaling form where one of its kernels takes (nmax, G); each holds whole rows in registers
    // nmax + 1 <= 448: 8 workgroups per pair, or the next count up that an instantiation takes
    int g = std::min(G_override ? G_override : 8, gmax);
    while (g <= 32 && g * B <= ncu && !sinkhorn_rb_rpw(nmax, g)) g++;
    if (g * B <= ncu && sinkhorn_rb_rpw(nmax, g)) {
      pl.kind = SinkKind::Sc;
      pl.rpw = sinkhorn_rb_rpw(nmax, g);
    } else if (g = G_override ? G_override : (ld + 47) / 48; g * B <= ncu && sinkhorn_sc10_ok(nmax, g)) {
      pl.kind = SinkKind::Sc10;  // 448 < nmax + 1 <= 640 (e.g. C4's 600 keypoints): workgroups of <= 48 rows
      pl.rpw = kSc10RPW;
    } else if (g = sinkhorn_wide_groups(nmax); g * B <= ncu && sinkhorn_wide_ok(nmax, g)) {
      pl.kind = SinkKind::Wide;  // 640 < nmax + 1 <= 2112 (C5's 2048 keypoints): 32 rows per workgroup, two hops
      pl.rpw = kWideRPW;
      pl.ug_granules = (size_t)B * sinkhorn_wide_hop1_len(nmax);
      pl.vg_granules = (size_t)B * sinkhorn_wide_hop2_len(nmax);
    }
    if (pl.rpw) {
      pl.G = g;
      if (pl.kind != SinkKind::Wide) pl.ug_granules = (size_t)B * 2 * g * ld;  // [B][2][G][ld] partial sums
    }
  }
  if (!pl.rpw && B * pl.G > ncu) return false;  // the slab workgroups of max_batch pairs do not fit the device
  *out = pl;
  return true;
}

hipError_t sinkhorn(const SinkArgs& a, const SinkPlan& pl, int B, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {
  if (pl.G < 1 || pl.G > 1024) return hipErrorInvalidValue;
  dim3 grid(pl.G, B);
  // each case checks that G fits the instantiation it launches: never a mismatched grid
  switch (pl.kind) {
    case SinkKind::Wide:
      if (!sinkhorn_wide_ok(a.nmax, pl.G)) return hipErrorInvalidValue;
      hipExtLaunchKernelGGL((sinkhorn_w_kernel<kWideRPW, kWideQ>), grid, dim3(kWThreads), 0, s, t0, t1, 0, a);
      break;
    case SinkKind::Sc10:
      if (!sinkhorn_sc10_ok(a.nmax, pl.G)) return hipErrorInvalidValue;
      hipExtLaunchKernelGGL((sinkhorn_sc_kernel<kSc10RPW, 16, 10>), grid, dim3(kSinkThreads), 0, s, t0, t1, 0, a);
      break;
    case SinkKind::Sc:
      if (sinkhorn_rb_rpw(a.nmax, pl.G) != pl.rpw) return hipErrorInvalidValue;
      switch (pl.rpw) {
#define RSPL_SK_SC(R, M)                                                                                     \
  case R:                                                                                                    \
    hipExtLaunchKernelGGL((sinkhorn_sc_kernel<R, M, kRbQ>), grid, dim3(kSinkThreads), 0, s, t0, t1, 0, a);   \
    break;
        RSPL_SK_SC(8, 4)
        RSPL_SK_SC(4, 8)
        RSPL_SK_SC(2, 16)
        RSPL_SK_SC(1, 32)
#undef RSPL_SK_SC
        default: return hipErrorInvalidValue;
      }
      break;
    case SinkKind::Slab: {
      const size_t full = sinkhorn_lds_bytes(a.nmax, pl.G, true);
      if (full > kSinkLdsMax) return hipErrorInvalidValue;
      static size_t attr = 0;
      if (attr < full) {
        hipError_t e = hipFuncSetAttribute((const void*)sinkhorn_kernel<true>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)full);
        if (e != hipSuccess) return e;
        attr = full;
      }
      hipExtLaunchKernelGGL((sinkhorn_kernel<true>), grid, dim3(kSinkThreads), (uint32_t)full, s, t0, t1, 0, a);
      break;
    }
    case SinkKind::SlabScratch:  // slabs too large for LDS: rows in place, columns from the cplT copy
      if (!a.cplT) return hipErrorInvalidValue;
      hipExtLaunchKernelGGL((sinkhorn_kernel<false>), grid, dim3(kSinkThreads),
                            (uint32_t)sinkhorn_lds_bytes(a.nmax, pl.G, false), s, t0, t1, 0, a);
      break;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// decode (super_glue.cpp:339-367).  Pass 1: row / column argmax (strict '<'
// from -FLT_MAX: first maximum wins).  Pass 2: mutual check, exp, threshold.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void argmax_kernel(DecodeArgs a) {
  const int p = blockIdx.z, ld = a.nmax + 1;
  const int m = a.n0[p], n = a.n1[p];
  const float* Z = a.Z + (size_t)p * ld * ld;
  {  // rows: one wave per row
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (i >= m) return;
    float best = -FLT_MAX;
    int idx = 0;
    for (int j = lane; j < n; j += 64) {
      const float x = Z[(size_t)i * ld + j];
      if (best < x) { best = x; idx = j; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(idx, o);
      if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if (lane == 0) {
      a.max0[(size_t)p * a.nmax + i] = idx;
      a.val0[(size_t)p * a.nmax + i] = best;
    }
  }
}

// column argmax: 64 columns x 16 row groups per block; groups combined in LDS with the
// same strict '<' scan semantics (the smallest row index among equal maxima wins)
__global__ __launch_bounds__(1024) void col_argmax_kernel(DecodeArgs a) {
  __shared__ float bv[16][64];
  __shared__ int bi[16][64];
  const int p = blockIdx.z, ld = a.nmax + 1;
  const int m = a.n0[p], n = a.n1[p];
  const float* Z = a.Z + (size_t)p * ld * ld;
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c;
  float best = -FLT_MAX;
  int idx = 0;
  if (j < n) {
    const int per = (m + 15) / 16, i0 = rg * per, i1 = min(m, i0 + per);
#pragma unroll 8
    for (int i = i0; i < i1; i++) {
      const float x = Z[(size_t)i * ld + j];
      if (best < x) { best = x; idx = i; }
    }
    if (i0 >= i1) idx = 0x7fffffff;
  }
  bv[rg][c] = best;
  bi[rg][c] = idx;
  __syncthreads();
  if (rg == 0 && j < n) {
    float b = -FLT_MAX;
    int id = 0;
    bool any = false;
    for (int g = 0; g < 16; g++) {
      if (bi[g][c] == 0x7fffffff) continue;
      if (!any || b < bv[g][c]) { b = bv[g][c]; id = bi[g][c]; any = true; }
    }
    a.max1[(size_t)p * a.nmax + j] = id;
  }
}

__device__ __forceinline__ bool mutual0_of(const DecodeArgs& a, int p, int i, int m, int n) {
  if (n <= 0 || m <= 0) return false;
  const int j = a.max0[(size_t)p * a.nmax + i];
  return a.max1[(size_t)p * a.nmax + j] == i;
}

__global__ __launch_bounds__(256) void finalize_kernel(DecodeArgs a) {
  const int p = blockIdx.z;
  const int m = a.n0[p], n = a.n1[p];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.y == 0) {
    if (t >= m) return;
    const bool mu = mutual0_of(a, p, t, m, n);
    const double ms = mu ? (double)expf(a.val0[(size_t)p * a.nmax + t]) : 0.0;  // std::exp(float)
    const bool valid = mu && ms > (double)a.threshold;
    a.ms0[(size_t)p * a.nmax + t] = ms;
    a.idx0[(size_t)p * a.nmax + t] = valid ? a.max0[(size_t)p * a.nmax + t] : -1;
  } else {
    if (t >= n) return;
    bool mu1 = false;
    int i = 0;
    if (m > 0) {
      i = a.max1[(size_t)p * a.nmax + t];
      mu1 = a.max0[(size_t)p * a.nmax + i] == t;
    }
    double ms1 = 0.0;
    bool valid1 = false;
    if (mu1) {
      const bool mu0 = mutual0_of(a, p, i, m, n);
      const double ms0 = mu0 ? (double)expf(a.val0[(size_t)p * a.nmax + i]) : 0.0;
      ms1 = ms0;
      valid1 = mu0 && ms0 > (double)a.threshold;
    }
    a.ms1[(size_t)p * a.nmax + t] = ms1;
    a.idx1[(size_t)p * a.nmax + t] = valid1 ? i : -1;
  }
}

hipError_t decode(const DecodeArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(argmax_kernel, dim3((a.nmax * 64 + 255) / 256, 1, B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(col_argmax_kernel, dim3((a.nmax + 63) / 64, 1, B), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(finalize_kernel, dim3((a.nmax + 255) / 256, 2, B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sg
}  // namespace rspl
