// Local BA (see ba_device.hpp), Schur complement and the reduced camera system: the Schur chunks over the
// edge-pair lists, the pose-pair sums, and the four solvers of the reduced system with the one place
// that picks between them (launch_solve / launch_global_solve).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_kernels.hpp"
#include "ba_launch.hpp"
#include "ba_linearize.hpp"
#include "ba_solve_reg.hpp"

namespace rspl {
namespace ba {

// orders this wave's LDS writes before its later LDS reads (lanes exchange through LDS)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Schur complement, stage 1: one wave per chunk (pose pair, landmark range) walks its
// segment of the edge-pair lists, forming Y = Hpl_e1 Dinv_g on the fly:
//   [0,36)  [e1==e2] Hpp_e1 - Y Hpl_e2^T,   [36,42) [e1==e2] bp_e1,   [42,48) [e1==e2] Y bl_g
// then the wave sums its 64 lanes in lane order (LDS transpose).

// larger systems, stage 2: one thread per (pose pair, entry) scatters the pair sums.
//   S_ab = [a==b] lambda I + pair sum,  bp_a,  bs_a = bp_a - sum Y bl  (solved in place in x)
__global__ __launch_bounds__(256) void pair_final_kernel(Active A, Sys S, double lambda) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.npairs * 42) return;
  const int pr = idx / 42, v = idx - 42 * pr;
  const int a = A.pairs[2 * pr], b = A.pairs[2 * pr + 1], n = 6 * A.K;
  const double s = S.pairfin[48 * pr + v];
  if (v < 36) {
    const int r = v / 6, cc = v - 6 * r;
    const double val = s + ((a == b && r == cc) ? lambda : 0.0);
    S.S[(size_t)(6 * a + r) * n + 6 * b + cc] = val;
    if (a != b) S.S[(size_t)(6 * b + cc) * n + 6 * a + r] = val;
  } else if (a == b) {
    const int r = v - 36;
    S.bp[6 * a + r] = s;
    S.x[6 * a + r] = s - S.pairfin[48 * pr + v + 6];
  }
}

// ---------------------------------------------------------------------------
// Reduced camera system: Schur assembly + dense LDL^T + solve in one 256-thread workgroup,
// matrix in LDS (odd row stride), n = 6K <= kCholLdsMax.
//   assembly: S_ab = [a==b] lambda I + the pair's chunk sum (reduced by its last chunk),
//             written straight into the lower triangle; bp_a alongside, and bs as an extra
//             bordered row n;
//   factor:   blocked by the 6x6 pose blocks, K steps of LDL^T (pivots need a reciprocal
//             only: v_rcp_f64 + Newton, no sqrt / divide chains):
//             (1) wave 0 factors the diagonal block in registers (every lane, uniform),
//             (2) panel rows solve x L_dd^T = a (one lane per row, the rhs row included:
//                 it ends as z = D^-1 L^-1 bs, so there is no forward substitution),
//             (3) rank-6 update of the trailing lower triangle (16x16 thread grid);
//   solve:    backward substitution L^T x = z in wave 0, LDS-resident;
//   poses:    the candidate T <- exp(xp) T and the pose part of the LM scale.
// ---------------------------------------------------------------------------
constexpr int kCholLdsMax = 192;  // packed lower triangle (n+1)(n+2)/2 + 3n + 15 n/6 doubles <= 160 KB of LDS

// packed row-major lower triangle: element (r, c <= r)
__device__ __forceinline__ int pk(int r, int c) { return r * (r + 1) / 2 + c; }

// 1/d to full precision: v_rcp_f64 + two Newton steps (no divide sequence on the chain)
__device__ __forceinline__ double rcp64(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(r, fma(-d, r, 1.0), r);
  return fma(r, fma(-d, r, 1.0), r);
}

// LDL^T of the 6x6 SPD diagonal block at (c0, c0) of the packed lower triangle Al: unit L
// (strictly-lower, packed row-major into L6), D (d6) and 1/D (r6); false unless every pivot is > 0
__device__ __forceinline__ bool ldl6(const double* Al, int c0, double (&L6)[15], double (&d6)[6], double (&r6)[6]) {
  double a[6][6];
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int k = 0; k <= i; k++) a[i][k] = Al[pk(c0 + i, c0 + k)];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const double d = a[j][j];
    ok = ok && d > 0;
    const double r = rcp64(d);
    d6[j] = d;
    r6[j] = r;
    double u[6];
#pragma unroll
    for (int i = j + 1; i < 6; i++) u[i] = a[i][j];
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      const double l = u[i] * r;
      a[i][j] = l;
#pragma unroll
      for (int k = j + 1; k <= i; k++) a[i][k] -= l * u[k];
    }
  }
#pragma unroll
  for (int i = 0, q = 0; i < 6; i++)
#pragma unroll
    for (int k = 0; k < i; k++, q++) L6[q] = a[i][k];
  return ok;
}

// pose pair index -> (a, b), a <= b, row-major upper triangle of K poses
__device__ __forceinline__ void pair_of(int pr, int K, int& a, int& b) {
  int base = 0;
  a = 0;
  while (pr >= base + (K - a)) {
    base += K - a;
    a++;
  }
  b = a + (pr - base);
}

__global__ __launch_bounds__(256) void schur_solve_kernel(Problem P, Active A, Sys S, int n, double lambda) {
  extern __shared__ double Al[];     // rows 0..n, packed lower triangle: the matrix + the bordered rhs row n
  __shared__ int bad;
  if (S.lm) {  // device-side LM: damping and bank from the control
    LmView v;
    if (!lm_view(S, v)) return;
    lambda = v.lambda;
    if (v.cur) bank_state(P);
  }
  const int K = n / 6;
  double* z = Al + pk(n, 0);         // row n: bs -> z = D^-1 L^-1 bs -> solution x
  double* rdg = Al + pk(n + 1, 0);   // [n] 1/D
  double* ddg = rdg + n;                    // [n] D
  double* Ldg = ddg + n;                    // [K][15] strictly-lower parts of the (unit) diagonal blocks
  double* bpl = Ldg + 15 * K;               // [n] pose gradient bp (for the LM scale)
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  const int pose_a = tid < P.np ? A.pidx[tid] : -1;  // the pose part of the LM scale (lane = pose)
  if (tid == 0) prof_stamp(S, 0);
  // assembly: every thread issues its pairfin loads (8 at a time) before writing LDS; the
  // fail flag is checked after them (it would otherwise gate every load)
  const int nent = A.npairs * 42;
  for (int q0 = tid; q0 < nent; q0 += 8 * 256) {
    double v1[8], v2[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int idx = q0 + u * 256;
      const int pr = idx / 42, v = idx - 42 * pr;
      v1[u] = idx < nent ? S.pairfin[48 * pr + v] : 0.0;
      v2[u] = (idx < nent && v >= 36) ? S.pairfin[48 * pr + v + 6] : 0.0;
    }
    if (*S.fail) return;  // uniform: a landmark block failed to invert
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int idx = q0 + u * 256;
      if (idx >= nent) break;
      const int pr = idx / 42, v = idx - 42 * pr;
      int pa, pb;
      pair_of(pr, K, pa, pb);
      if (v < 36) {
        const int r = v / 6, cc = v - 6 * r;
        if (pa == pb) {
          if (cc <= r) Al[pk(6 * pa + r, 6 * pa + cc)] = v1[u] + (r == cc ? lambda : 0.0);
        } else {
          Al[pk(6 * pb + cc, 6 * pa + r)] = v1[u];
        }
      } else if (pa == pb) {
        const int r = v - 36;
        bpl[6 * pa + r] = v1[u];
        z[6 * pa + r] = v1[u] - v2[u];
      }
    }
  }
  __syncthreads();
  if (tid == 0) prof_stamp(S, 1);
  // factor: blocked by the 6x6 pose blocks; the rhs row n is factored along (its panel rows
  // become z = D^-1 L^-1 bs: no separate forward substitution)
  const int wv = tid >> 6, lane = tid & 63, fy = tid >> 4, fx = tid & 15;
  for (int s = 0; s < K; s++) {
    const int c0 = 6 * s, r0 = c0 + 6;
    if (wv == 0) {  // (1) diagonal block (every lane, uniform) + (2) panel rows, one per lane
      double L6[15], d6[6], r6[6];
      const bool ok = ldl6(Al, c0, L6, d6, r6);
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 15; q++) Ldg[15 * s + q] = L6[q];
#pragma unroll
        for (int k = 0; k < 6; k++) {
          rdg[c0 + k] = r6[k];
          ddg[c0 + k] = d6[k];
        }
        if (!ok) bad = 1;
      }
      for (int i = r0 + lane; i <= n; i += 64) {  // x = a L_dd^-T D^-1 (unit L: no divides)
        double* row = Al + pk(i, c0);
        double w[6];
#pragma unroll
        for (int k = 0; k < 6; k++) w[k] = row[k];
#pragma unroll
        for (int k = 0, q = 0; k < 6; k++) {
#pragma unroll
          for (int l = 0; l < k; l++, q++) w[k] -= w[l] * L6[q];
        }
#pragma unroll
        for (int k = 0; k < 6; k++) row[k] = w[k] * r6[k];
      }
    }
    __syncthreads();
    if (tid == 0 && s < 2) prof_stamp(S, 5 + 2 * s);  // step s: pivot block + panel done
    if (bad) {  // LDS flag after the barrier: uniform
      if (tid == 0) atomicOr(S.fail, 1);
      return;
    }
    for (int i = r0 + fy; i <= n; i += 16) {  // (3) trailing update A22 -= X D X^T (+ the rhs row)
      double wi[6];
#pragma unroll
      for (int l = 0; l < 6; l++) wi[l] = Al[pk(i, c0 + l)] * ddg[c0 + l];
      const int kmax = min(i, n - 1);
      for (int k = r0 + fx; k <= kmax; k += 16) {
        const double* xk = Al + pk(k, c0);
        double t = Al[pk(i, k)];
#pragma unroll
        for (int l = 0; l < 6; l++) t -= wi[l] * xk[l];
        Al[pk(i, k)] = t;
      }
    }
    __syncthreads();
    if (tid == 0 && s < 2) prof_stamp(S, 6 + 2 * s);  // step s: trailing update done
  }
  if (wv != 0) return;
  if (tid == 0) prof_stamp(S, 2);
  // backward substitution L^T x = z in wave 0 (LDS in program order within the wave)
  for (int s = K - 1; s >= 0; s--) {
    const int c0 = 6 * s;
    double xb[6];
#pragma unroll
    for (int k = 5; k >= 0; k--) {
      double v = z[c0 + k];
#pragma unroll
      for (int l = k + 1; l < 6; l++) v -= Ldg[15 * s + l * (l - 1) / 2 + k] * xb[l];
      xb[k] = v;
    }
    for (int i = lane; i < c0; i += 64) {
      double v = z[i];
#pragma unroll
      for (int l = 0; l < 6; l++) v -= Al[pk(c0 + l, i)] * xb[l];
      z[i] = v;
    }
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < 6; k++) z[c0 + k] = xb[k];
  }
  for (int i = lane; i < n; i += 64) S.x[i] = z[i];
  if (tid == 0) prof_stamp(S, 3);
  // the pose part of the LM scale x.(lambda x + bp) (lane = pose; the candidate poses are formed
  // by update_errors_kernel)
  double sc = 0;
  if (lane < P.np && pose_a >= 0)
#pragma unroll
    for (int k = 0; k < 6; k++) sc += z[6 * pose_a + k] * (lambda * z[6 * pose_a + k] + bpl[6 * pose_a + k]);
  sc = wave::xsum64(sc);
  if (lane == 0) S.out[4] = sc;
  if (tid == 0) prof_stamp(S, 4);
}

// ---------------------------------------------------------------------------
// 10 < K <= kRegMaxK (C5's 30-keyframe window, n = 174): rspl::ba::solve_reg (ba_solve_reg.hpp) -- the matrix as
// fp64 MFMA accumulator tiles on SIMDs 1..3, the pivot chain alone on SIMD 0, look-ahead between the two, one
// 768-thread workgroup.  (Replaced the round-5 block-per-thread register kernel: 108 -> 95 us per solve at K = 29 in
// tools/experiments/solve_bench.hip, results within 1e-14 of it.)
// ---------------------------------------------------------------------------
// lane l's double, read by every lane (l uniform)
__device__ __forceinline__ double readlane64(double v, int l) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

constexpr int kRegMaxK = kSolveRegMaxK;

struct BaSolveStamp {  // RSPL_BA_PROF slots of the solve (ba.cpp report_prof)
  const Sys& S;
  __device__ void at(int slot) const {
    if (threadIdx.x == 0) prof_stamp(S, slot);
  }
  __device__ void step(int s, int) const {
    if (threadIdx.x == 0 && s < 2) prof_stamp(S, 5 + 2 * s);
  }
  __device__ void wave(int, int) const {}
};

__global__ __launch_bounds__(kSolveRegThreads) void schur_reg_kernel(Problem P, Active A, Sys S, int n, double lambda) {
  extern __shared__ double lds_sr[];
  if (S.lm) {  // device-side LM: damping from the control
    LmView v;
    if (!lm_view(S, v)) return;
    lambda = v.lambda;
  }
  solve_reg(S.pairfin, n / 6, lambda, S.x, S.out + 4, S.fail, A.pidx, P.np, lds_sr, BaSolveStamp{S});
}

// ---------------------------------------------------------------------------
// Reduced camera system for n = 6K <= 60 (K <= kWaveSolveMaxK optimised poses: the C3 window)
// in ONE wavefront, no workgroup barrier.  Lane i owns row i of S in registers (a[0, N): only
// k <= i is meaningful) and the bordered rhs entry z_i.  Right-looking LDL^T column by column:
//   pivot d_j = a_jj by readlane (every lane, uniform), l_ij = a_ij / d_j (lanes i > j),
//   column j's unscaled entries w_kj broadcast through LDS, a_ik -= l_ij w_kj for every k > j
//   (entries above the diagonal are never read), z_i -= l_ij z_j (forward substitution fused);
// then y = D^-1 z and the backward substitution L^T x = y, column i of L read back from LDS into
// registers so the dependent chain is readlane + fma per row.  Assembly reads the pose-pair sums
// (pairfin) straight into the rows; the candidate poses and the pose part of the LM scale follow.
// Returns false (nothing written) when the landmark inversion failed upstream or a pivot is <= 0.
// ---------------------------------------------------------------------------
constexpr int kWaveSolveMaxK = 10;

struct WaveSolveLds {
  double W[2][64][6];  // the panel's unscaled column entries w_ij of row i, double-buffered by block parity
  double Lm[60][61];   // Lm[j][i] = l_ij (column j of L); odd stride
};

// pose pair index of (c, a), c <= a, row-major upper triangle of K poses
__device__ __forceinline__ int pair_index(int c, int a, int K) { return c * K - c * (c - 1) / 2 + (a - c); }

template <int N>
__device__ __forceinline__ void solve_wave(Problem P, const Active& A, const Sys& S, double lambda, WaveSolveLds& w,
                                           bool coherent) {
  constexpr int K = N / 6;
  const int lane = threadIdx.x & 63;
  const int pa = lane / 6, r = lane - 6 * pa;
  const bool row = lane < N;
  auto ld = [&](int idx) {
    return coherent ? __hip_atomic_load(S.pairfin + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : S.pairfin[idx];
  };
  double a[N];
  double z = 0.0, bpl = 0.0;
  {
    const int dg = 48 * pair_index(pa, pa, K);
    // branch-free: every lane issues all N loads (lanes / entries outside the lower triangle read
    // slot 0 and discard it), so the loads go out back to back without exec-mask branches
#pragma unroll
    for (int k = 0; k < N; k++) {
      const int c = k / 6, cc = k - 6 * (k / 6);
      const bool valid = row && k <= lane;  // then c <= pa
      int idx = c == pa ? dg + r * 6 + cc : 48 * pair_index(c, pa, K) + cc * 6 + r;
      idx = valid ? idx : 0;
      const double v = ld(idx);
      a[k] = valid ? v : 0.0;
    }
    if (row) {
      bpl = ld(dg + 36 + r);
      z = bpl - ld(dg + 42 + r);
    }
  }
  const int failed = coherent ? __hip_atomic_load(S.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *S.fail;
  if (failed) return;  // uniform: a landmark block failed to invert
  if (lane == 0) prof_stamp(S, 1);
  // damping on the diagonal (a[k] with k == lane: select, static register index)
#pragma unroll
  for (int k = 0; k < N; k++) a[k] += (k == lane) ? lambda : 0.0;
  // Right-looking LDL^T blocked by the 6x6 pose blocks.  Panel b (pivots j = 6b .. 6b + 5): each lane
  // updates its own row's panel entries, the column entries of the panel's later rows broadcast by
  // readlane (no LDS on the pivot chain); then the lane's unscaled panel entries w_ij go to LDS once
  // (one wave_sync per pose block instead of per pivot) and every lane applies the rank-6 update
  // a_ik -= sum_j l_ij w_kj to its later columns k, j ascending -- the same FMAs in the same order as
  // the unblocked elimination.
  bool ok = true;
#pragma unroll
  for (int b = 0; b < K; b++) {
    double l6[6], w6[6];
#pragma unroll
    for (int jj = 0; jj < 6; jj++) {
      const int j = 6 * b + jj;
      const double dj = readlane64(a[j], j);
      ok = ok && dj > 0.0;
      const double rj = rcp64(dj);
      const double wij = a[j];
      const double l = lane > j ? wij * rj : 0.0;
      w6[jj] = wij;
      l6[jj] = l;
      w.Lm[j][lane] = l;
      const double zj = readlane64(z, j);
      z = fma(-l, zj, z);
#pragma unroll
      for (int c = j + 1; c < 6 * b + 6; c++) a[c] = fma(-l, readlane64(wij, c), a[c]);
    }
    if (b + 1 < K) {
#pragma unroll
      for (int jj = 0; jj < 6; jj++) w.W[b & 1][lane][jj] = w6[jj];
      wave_sync();
#pragma unroll
      for (int kb = b + 1; kb < K; kb++) {  // one later pose block (6 columns) at a time
        double wk[6][6];
#pragma unroll
        for (int c = 0; c < 6; c++)
#pragma unroll
          for (int jj = 0; jj < 6; jj++) wk[c][jj] = w.W[b & 1][6 * kb + c][jj];
#pragma unroll
        for (int c = 0; c < 6; c++)
#pragma unroll
          for (int jj = 0; jj < 6; jj++) a[6 * kb + c] = fma(-l6[jj], wk[c][jj], a[6 * kb + c]);
      }
    }
  }
  if (!ok) {
    if (lane == 0) atomicOr(S.fail, 1);
    return;
  }
  if (lane == 0) prof_stamp(S, 2);
  // y = D^-1 z; backward L^T x = y (lane i: y_i -= L_ki x_k for k > i, k descending)
  double dgl = 1.0;
#pragma unroll
  for (int k = 0; k < N; k++) dgl = k == lane ? a[k] : dgl;
  double y = z * rcp64(dgl);
  double lt[N];
#pragma unroll
  for (int k = 0; k < N; k++) lt[k] = row && k > lane ? w.Lm[lane][k] : 0.0;
#pragma unroll
  for (int k = N - 1; k >= 0; k--) {
    const double xk = readlane64(y, k);
    y = fma(-lt[k], xk, y);  // lt[k] == 0 for k <= lane
  }
  const double x = y;
  if (lane == 0) prof_stamp(S, 3);
  if (row) S.x[lane] = x;
  // the pose part of the LM scale x.(lambda x + bp) (the candidate poses: update_errors_kernel)
  double sc = row ? x * (lambda * x + bpl) : 0.0;
  sc = wave::xsum64(sc);
  if (lane == 0) S.out[4] = sc;
}

// standalone single-wave solve (sharded path: after the pairfin all-reduce)
template <int N>
__global__ __launch_bounds__(64) void schur_wave_kernel(Problem P, Active A, Sys S, double lambda) {
  __shared__ WaveSolveLds w;
  if (S.lm) {
    LmView v;
    if (!lm_view(S, v)) return;
    lambda = v.lambda;
    if (v.cur) bank_state(P);
  }
  solve_wave<N>(P, A, S, lambda, w, false);
}

// one edge pair's Schur terms with D = (Hll_g + lambda I)^-1, landmark dimension LD (3: points, 4: lines
// or a mixed range; 6 x 4 operands, the 4th column of a point's Hpl is zero): Y = Hpl_e1 D,
// acc -= Y Hpl_e2^T; diag (e1 == e2) adds Hpp_e1, bp_e1 and Y bl_g.  LOWER (a diagonal pose pair):
// only the block's lower triangle (cc <= r) -- the only part any solver reads of a diagonal block.
// Same products in the same order as the zero-padded 4-dim form.
template <int LD, bool LOWER>
__device__ __forceinline__ void schur_pair(const double (&H1)[6 * LD], const double (&B)[6 * LD], bool diag,
                                           const double (&Hp)[21], const double (&bpv)[6], const double (&blv)[LD],
                                           const double (&D)[LD * LD], double (&acc)[48]) {
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double y[LD];
#pragma unroll
    for (int q = 0; q < LD; q++) {
      double t = H1[r * LD] * D[q];
#pragma unroll
      for (int c = 1; c < LD; c++) t += H1[r * LD + c] * D[c * LD + q];
      y[q] = t;
    }
#pragma unroll
    for (int cc = 0; cc < (LOWER ? r + 1 : 6); cc++) {
      double t = y[0] * B[cc * LD];
#pragma unroll
      for (int q = 1; q < LD; q++) t += y[q] * B[cc * LD + q];
      acc[r * 6 + cc] -= t;
    }
    if (LOWER && diag) {
#pragma unroll
      for (int cc = 0; cc <= r; cc++) acc[r * 6 + cc] += Hp[pk6(cc, r)];
      acc[36 + r] += bpv[r];
      double t = y[0] * blv[0];
#pragma unroll
      for (int q = 1; q < LD; q++) t += y[q] * blv[q];
      acc[42 + r] += t;
    }
  }
}

// A chunk's walk over its edge-pair segment [beg, end), lane-strided, software-pipelined: the pair
// indices two passes ahead and every operand of the next pass are requested before this pass's
// arithmetic (ping-pong operand sets), so a wave waits on one memory round trip per segment rather than
// per pass.  LD 3: a range of point landmarks only (3x3 D, 6x3 Hpl); 4: a range holding lines.  LOWER: a
// diagonal pose pair (e1 == e2 pairs add Hpp / bp / Y bl; lower triangle only).
// Register budget: only the off-diagonal point chunks (most of them) keep the PairOps operand set; the
// diagonal chunks take e1 == e2 without a copy of H1, and line ranges invert the landmark block before
// their edge operands are requested, so the kernel fits 256 VGPRs with no AGPRs (was 255 + 52): a
// chunk wave then fits on a SIMD beside one front-end wave (a fp16 conv or GNN layer wave, <= 224
// registers) instead of waiting for the SIMD to drain.  The same FMAs in the same order as before.
template <int LD>
struct PairOps {
  double D[LD * LD], H1[6 * LD], H2[6 * LD], Hp[21], bpv[6], blv[LD];  // D: Hll of the landmark
  bool diag, live, pt;
};

template <int LD, bool LOWER>
__device__ __forceinline__ void load_pair(const Lin& L, const Active& A, const Sys& S, int nq, int4 q,
                                          PairOps<LD>& o) {
  static_assert(!LOWER && LD == 3, "off-diagonal pose pairs of point ranges only (chunk_loop takes the others)");
  const int e1 = q.x, e2 = q.y, g = q.z;
  o.diag = false;
  o.live = !(A.elevel && (A.elevel[e1] | A.elevel[e2]));  // else zero records: no contribution
  const double* dg = S.Hll + 16 * g;  // the landmark block (inverted in use_pair)
#pragma unroll
  for (int i = 0; i < LD * LD; i++) o.D[i] = dg[i];
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c < LD; c++) {
      o.H1[r * LD + c] = L.Hpl[18 * e1 + r * 3 + c];
      o.H2[r * LD + c] = L.Hpl[18 * e2 + r * 3 + c];
    }
  o.pt = g < nq;
}

template <int LD, bool LOWER>
__device__ __forceinline__ void use_pair(const PairOps<LD>& o, double lambda, bool& bad, double (&acc)[48]) {
  if (!o.live) return;
  double D[LD * LD];  // (Hll + lambda I)^-1 (Gauss-Jordan, partial pivoting; points 3x3, lines 4x4)
  if constexpr (LD == 3) {
    double Hd[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Hd[i] = o.D[i] + ((i % 4 == 0) ? lambda : 0.0);
    bad |= !small_inv<3>(Hd, D);
  } else {
    bad |= !lm_dinv(o.D, o.pt, lambda, D);
  }
  // one call site with B = H2 (a copy of H1 on the diagonal): two call sites on H1 / H2 were merged
  // by the compiler into one through a selected pointer, which put both arrays in scratch memory
  schur_pair<LD, LOWER>(o.H1, o.H2, o.diag, o.Hp, o.bpv, o.blv, D, acc);
}

template <int LD, bool LOWER>
__device__ __forceinline__ void chunk_loop(const Problem& P, const Lin& L, const Active& A, const Sys& S,
                                           const DiagPose& dp, int nq, int beg, int end, int4 qn, double lambda,
                                           bool& bad, double (&acc)[48]) {
  const int lane = threadIdx.x & 63;
  for (int k = beg + lane; k < end; k += 64) {
    const int4 q = qn;
    if (k + 64 < end) qn = A.pp[k + 64];
    if constexpr (LD == 4 && LOWER) {
      // diagonal pose pairs over line ranges (a few chunks per trial): the landmark inverse first, the
      // edge operands after it (no operand in flight across the 4x4 Gauss-Jordan) -- this path otherwise
      // sets the kernel's register budget above 256 (one wave per SIMD, none beside a front-end wave)
      const int e1 = q.x, e2 = q.y, g = q.z;
      const bool live = !(A.elevel && (A.elevel[e1] | A.elevel[e2]));
      double Hd[16], D[16];
#pragma unroll
      for (int i = 0; i < 16; i++) Hd[i] = S.Hll[16 * g + i];
      bad |= live && !lm_dinv(Hd, g < nq, lambda, D);
      asm volatile("" ::: "memory");
      if (live && e1 == e2) {  // the edge with itself: H1 twice, + Hp / bp / Y bl
        double H1[24], Hp[21], bpv[6], blv[4];
        // a point edge's pose block from the state (point_pose_block; its operands requested with H1 at
        // clamped addresses), a line edge's from its records
        const bool pt = g < nq;
        const int te = P.etype[e1], ci = P.ecam[e1];
        const double* obp = pt ? P.eobs + 4 * e1 : P.eobs;
        const double* xgp = pt ? P.X + 3 * g : P.cams;
        const double ob[3] = {obp[0], obp[1], obp[2]}, Xg[3] = {xgp[0], xgp[1], xgp[2]};
        load_hpl4(L.Hpl, P.Ep, e1, H1);
#pragma unroll
        for (int i = 0; i < 4; i++) blv[i] = S.bl[4 * g + i];
        if (pt) {
          point_pose_block(P, A, te, dp.pose, dp.cams + 5 * ci, ob, Xg, Hp, bpv);
        } else {
#pragma unroll
          for (int i = 0; i < 21; i++) Hp[i] = L.Hpp[21 * e1 + i];
#pragma unroll
          for (int i = 0; i < 6; i++) bpv[i] = L.bp[6 * e1 + i];
        }
        schur_pair<LD, LOWER>(H1, H1, true, Hp, bpv, blv, D, acc);
      } else if (live) {  // two edges of one landmark on the same pose (rare)
        double H1[24], H2[24], Hp[21], bpv[6], blv[4];
        load_hpl4(L.Hpl, P.Ep, e1, H1);
        load_hpl4(L.Hpl, P.Ep, e2, H2);
        schur_pair<LD, LOWER>(H1, H2, false, Hp, bpv, blv, D, acc);
      }
    } else if constexpr (LD == 4) {  // off-diagonal pose pairs over line ranges: the inverse first as well
      const int e1 = q.x, e2 = q.y, g = q.z;
      const bool live = !(A.elevel && (A.elevel[e1] | A.elevel[e2]));
      double Hd[16], D[16];
#pragma unroll
      for (int i = 0; i < 16; i++) Hd[i] = S.Hll[16 * g + i];
      bad |= live && !lm_dinv(Hd, g < nq, lambda, D);
      asm volatile("" ::: "memory");
      if (live) {
        double H1[24], H2[24], Hp[21], bpv[6], blv[4];
        load_hpl4(L.Hpl, P.Ep, e1, H1);
        load_hpl4(L.Hpl, P.Ep, e2, H2);
        schur_pair<LD, LOWER>(H1, H2, false, Hp, bpv, blv, D, acc);
      }
    } else if constexpr (LOWER) {  // diagonal pose pairs over point ranges: e1 == e2 without an H2 copy
      // every operand in one round trip, unconditionally (the edge's pose block is formed from the state by
      // point_pose_block: the pose and cameras in dp, the edge's type / camera / observation and the point
      // requested here with the records)
      const int e1 = q.x, e2 = q.y, g = q.z;
      const bool live = !(A.elevel && (A.elevel[e1] | A.elevel[e2]));
      double Hd[9], D[9], H1[18], Hp[21], bpv[6], blv[3], ob[3], Xg[3];
#pragma unroll
      for (int i = 0; i < 9; i++) Hd[i] = S.Hll[16 * g + i];
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) H1[r * 3 + c] = L.Hpl[18 * e1 + r * 3 + c];
      const int te = P.etype[e1], ci = P.ecam[e1];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        blv[i] = S.bl[4 * g + i];
        ob[i] = P.eobs[4 * e1 + i];
        Xg[i] = P.X[3 * g + i];
      }
      if (live) {
#pragma unroll
        for (int i = 0; i < 9; i++) Hd[i] += (i % 4 == 0) ? lambda : 0.0;
        bad |= !small_inv<3>(Hd, D);
        if (e1 == e2) {
          point_pose_block(P, A, te, dp.pose, dp.cams + 5 * ci, ob, Xg, Hp, bpv);
          schur_pair<LD, LOWER>(H1, H1, true, Hp, bpv, blv, D, acc);
        } else {
          double H2[18];
#pragma unroll
          for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) H2[r * 3 + c] = L.Hpl[18 * e2 + r * 3 + c];
          schur_pair<LD, LOWER>(H1, H2, false, Hp, bpv, blv, D, acc);
        }
      }
    } else {
      PairOps<LD> o;
      load_pair<LD, LOWER>(L, A, S, nq, q, o);
      use_pair<LD, LOWER>(o, lambda, bad, acc);
    }
  }
}

// One Schur chunk (pose pair, landmark range) on one wave: walks its segment of the edge-pair
// lists, sums its 64 lanes in lane order (LDS transpose in red[64 * 49], this wave's own) and hands
// the partial off write-through to whichever chunk of the pose pair finishes last; that one sums the
// pair's chunks in chunk order (deterministic) into pairfin (write-through when `wt`: a solver in the
// same launch reads it).  vb is the chunk's virtual workgroup id (XCD-aware order).  Returns true in
// the wave that completed a pose pair.
// The chunk of virtual workgroup vb and its pair-list segment (bank-independent: requested before the
// LM control is read).  The XCD-aware order of the chunks is chunk_at's (ba_kernels.hpp).
struct ChunkSeg {
  int c, lb, beg, end;
  int pr, c0, c1;  // its pose pair and that pair's chunks
  bool pts;        // a range of point landmarks only
  int4 q0;         // the lane's first pair
};
__device__ __forceinline__ bool chunk_seg(const Active& A, int nq, int vb, ChunkSeg& cs) {
  const int lane = threadIdx.x & 63;
  ChunkGeo cg;
  if (!chunk_at(A, vb, cs.c, cg)) return false;
  cs.lb = cg.lb;
  cs.pr = cg.pr;
  cs.c0 = cg.c0;
  cs.c1 = cg.c1;
  cs.pts = cg.gend <= nq;
  cs.beg = A.pp_off[cs.c];
  cs.end = A.pp_off[cs.c + 1];
  cs.q0 = cs.beg + lane < cs.end ? A.pp[cs.beg + lane] : make_int4(0, 0, 0, 0);
  return true;
}

__device__ __forceinline__ bool chunk_wave(const Problem& P, const Lin& L, const Active& A, const Sys& S,
                                           double lambda, const ChunkSeg& cs, double* red, bool wt) {
  const int lane = threadIdx.x & 63;
  const int c = cs.c, beg = cs.beg, end = cs.end;
  if (lane == 0 && c < 4096) prof_stamp(S, kProfPc + 4 * c);
  const int pr = cs.pr;
  double acc[48];
#pragma unroll
  for (int v = 0; v < 48; v++) acc[v] = 0.0;
  // a range of point landmarks only
  // (all but the last range or two) takes the 3-dim loops, off-diagonal pose pairs without the e1 == e2 terms
  const bool pts = cs.pts;
  const int pa = A.pairs[2 * pr];
  const bool dpp = pa == A.pairs[2 * pr + 1];
  DiagPose dp;
  if (dpp) {  // a diagonal pose pair: its pose's rotation / translation and the cameras, in this wave's LDS
    const unsigned long long m = __ballot(lane < P.np && A.pidx[lane] == pa);
    if (lane == 0) {
      const SE3 T = load_T(P.T + 8 * (__ffsll((long long)m) - 1));
      double R[9];
      q_to_R(T.q, R);
#pragma unroll
      for (int i = 0; i < 9; i++) red[i] = R[i];
#pragma unroll
      for (int i = 0; i < 3; i++) red[9 + i] = T.t[i];
    }
    for (int i = lane; i < 5 * P.ncam; i += 64) red[12 + i] = P.cams[i];
    dp.pose = red;
    dp.cams = red + 12;
    wave_sync();
  }
  bool bad = false;
  if (pts && !dpp) chunk_loop<3, false>(P, L, A, S, dp, P.nq, beg, end, cs.q0, lambda, bad, acc);
  else if (pts) chunk_loop<3, true>(P, L, A, S, dp, P.nq, beg, end, cs.q0, lambda, bad, acc);
  else if (!dpp) chunk_loop<4, false>(P, L, A, S, dp, P.nq, beg, end, cs.q0, lambda, bad, acc);
  else chunk_loop<4, true>(P, L, A, S, dp, P.nq, beg, end, cs.q0, lambda, bad, acc);
  if (bad) atomicOr(S.fail, 1);
  wave_sync();  // (the cameras' LDS reads before the transpose below overwrites them)
  if (lane == 0 && c < 4096) prof_stamp(S, kProfPc + 4 * c + 1);
#pragma unroll
  for (int v = 0; v < 48; v++) red[lane * 49 + v] = acc[v];
  wave_sync();
  if (lane < 48) {  // 8 independent partial sums, combined in a fixed order
    double p8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int l = 0; l < 64; l++) p8[l & 7] += red[l * 49 + lane];
    const double s = ((p8[0] + p8[1]) + (p8[2] + p8[3])) + ((p8[4] + p8[5]) + (p8[6] + p8[7]));
    __hip_atomic_store(S.chunk + 48 * c + lane, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int c0 = cs.c0, c1 = cs.c1;
  unsigned tk = 0;
  if (lane == 0) tk = __hip_atomic_fetch_add(S.pair_ctr + pr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  tk = __shfl(tk, 0);
  if (tk != (unsigned)(c1 - c0 - 1)) {
    if (lane == 0 && c < 4096) prof_stamp(S, kProfPc + 4 * c + 2);
    return false;
  }
  if (lane == 0) __hip_atomic_store(S.pair_ctr + pr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (lane < 48) {
    double s = 0;
    for (int cb = c0; cb < c1; cb += 16) {  // 16 write-through loads in flight, summed in chunk order
      double t[16];
#pragma unroll
      for (int u = 0; u < 16; u++)
        t[u] = cb + u < c1 ? __hip_atomic_load(S.chunk + 48 * (cb + u) + lane, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)
                           : 0.0;
#pragma unroll
      for (int u = 0; u < 16; u++) s += t[u];
    }
    if (wt) __hip_atomic_store(S.pairfin + 48 * pr + lane, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else S.pairfin[48 * pr + lane] = s;
  }
  if (lane == 0 && c < 4096) prof_stamp(S, kProfPc + 4 * c + 3);
  return true;
}

// second ticket over the pose pairs (re-armed by its winner): true in the wave that finished the
// last pose pair -- every pair sum is then out (write-through)
__device__ __forceinline__ bool last_pair(const Sys& S, int npairs) {
  const int lane = threadIdx.x & 63;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unsigned tp = 0;
  if (lane == 0) tp = __hip_atomic_fetch_add(S.solve_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  tp = __shfl(tp, 0);
  if (tp != (unsigned)(npairs - 1)) return false;
  if (lane == 0) __hip_atomic_store(S.solve_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// N > 0 (6K <= 60): the pose pair finished last solves the reduced system in the same wave
// (solve_wave<N>), so the trial needs no separate solve launch.
template <int N>
__global__ __launch_bounds__(64) void pair_chunk_kernel(Problem P, Lin L, Active A, Sys S, double lambda, Lin Ls,
                                                        Sys Ss) {
  constexpr int kRedLen = 64 * 49, kSolveLen = (int)(sizeof(WaveSolveLds) / sizeof(double));
  __shared__ double smem[N > 0 && kSolveLen > kRedLen ? kSolveLen : kRedLen];
  ChunkSeg cs;
  if (!chunk_seg(A, P.nq, blockIdx.x, cs)) return;  // in flight while the control is read
  if (S.lm) {  // device-side LM: damping and bank from the control
    LmView v;
    if (!lm_view(S, v)) return;
    lambda = v.lambda;
    if (v.cur) {  // (the state too: the diagonal chunks form their point edges' pose blocks from it)
      bank_lin(L, Ls, S, Ss);
      bank_state(P);
    }
  }
  if (!chunk_wave(P, L, A, S, lambda, cs, smem, N > 0)) return;
  if constexpr (N > 0) {
    if (!last_pair(S, A.npairs)) return;
    wave_sync();  // red[] is dead: the LDS becomes the solver's
    if (threadIdx.x == 0) prof_stamp(S, 0);
    solve_wave<N>(P, A, S, lambda, *reinterpret_cast<WaveSolveLds*>(smem), true);
    if (threadIdx.x == 0) prof_stamp(S, 4);
  }
}

// larger systems: one workgroup on global memory

__global__ __launch_bounds__(256) void cholesky_kernel(Sys S, int n) {
  __shared__ double red[256];
  __shared__ int bad;
  double* A = S.S;
  double* x = S.x;
  const int tid = threadIdx.x;
  if (tid == 0) bad = *S.fail;
  __syncthreads();
  if (bad) return;
  for (int j = 0; j < n; j++) {
    if (tid == 0) {
      const double v = A[(size_t)j * n + j];
      if (!(v > 0)) bad = 1;
      else A[(size_t)j * n + j] = sqrt(v);
    }
    __syncthreads();
    if (bad) {
      if (tid == 0) atomicOr(S.fail, 1);
      return;
    }
    const double d = A[(size_t)j * n + j];
    for (int i = j + 1 + tid; i < n; i += 256) A[(size_t)i * n + j] /= d;
    __syncthreads();
    const int m = n - j - 1;
    for (int idx = tid; idx < m * m; idx += 256) {
      const int i = j + 1 + idx / m, k = j + 1 + idx % m;
      if (k <= i) A[(size_t)i * n + k] -= A[(size_t)i * n + j] * A[(size_t)k * n + j];
    }
    __syncthreads();
  }
  for (int i = 0; i < n; i++) {
    double s = 0;
    for (int k = tid; k < i; k += 256) s += A[(size_t)i * n + k] * x[k];
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) red[tid] += red[tid + st];
      __syncthreads();
    }
    if (tid == 0) x[i] = (x[i] - red[0]) / A[(size_t)i * n + i];
    __syncthreads();
  }
  for (int i = n - 1; i >= 0; i--) {
    double s = 0;
    for (int k = i + 1 + tid; k < n; k += 256) s += A[(size_t)k * n + i] * x[k];
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) red[tid] += red[tid + st];
      __syncthreads();
    }
    if (tid == 0) x[i] = (x[i] - red[0]) / A[(size_t)i * n + i];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
bool fast_path(int K) { return 6 * K > 0 && 6 * K <= kCholLdsMax; }
bool wave_path(int K) { return K > 0 && K <= kWaveSolveMaxK; }

void launch_chunks(const Problem& P, const Lin& L, const Active& A, const Sys& S, double lambda, const Lin& Ls,
                   const Sys& Ss, bool wave_fused, hipStream_t s) {
  const dim3 g(chunk_grid(A)), b(64);  // (idle slots exit)
  switch (wave_fused ? A.K : 0) {
#define RSPL_CHUNK_CASE(k) \
  case k: hipLaunchKernelGGL(pair_chunk_kernel<6 * k>, g, b, 0, s, P, L, A, S, lambda, Ls, Ss); break;
    RSPL_CHUNK_CASE(1) RSPL_CHUNK_CASE(2) RSPL_CHUNK_CASE(3) RSPL_CHUNK_CASE(4) RSPL_CHUNK_CASE(5)
    RSPL_CHUNK_CASE(6) RSPL_CHUNK_CASE(7) RSPL_CHUNK_CASE(8) RSPL_CHUNK_CASE(9) RSPL_CHUNK_CASE(10)
#undef RSPL_CHUNK_CASE
    default: hipLaunchKernelGGL(pair_chunk_kernel<0>, g, b, 0, s, P, L, A, S, lambda, Ls, Ss); break;
  }
}

static size_t schur_lds_bytes(int n) {
  return sizeof(double) * ((size_t)(n + 1) * (n + 2) / 2 + 3 * n + 15 * (n / 6));
}

static hipError_t ensure_schur_attr() {
  static bool attr = false;
  if (attr) return hipSuccess;
  hipError_t e = hipFuncSetAttribute((const void*)schur_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)schur_lds_bytes(kCholLdsMax));
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)schur_reg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)solve_reg_lds_bytes(kRegMaxK));
  if (e == hipSuccess) attr = true;
  return e;
}

// The reduced-system solver by window size K (optimised poses), chosen here and nowhere else:
//   K <= kWaveSolveMaxK (10)        the single-wave LDL^T, solve_wave<6K>: fused into the last Schur chunk
//                                   (wave_fused: nothing to launch; a 4-wave blocked LDL^T as a third launch lost
//                                   in the pipeline, profiles/r03_experiments.md), or on its own as
//                                   schur_wave_kernel<6K> when an all-reduce separates chunks and solve;
//   K <= kRegMaxK (30)              schur_reg_kernel: the matrix in registers as fp64 MFMA tiles (ba_solve_reg.hpp);
//   K <= kCholLdsMax / 6 (32)       schur_solve_kernel: the packed lower triangle in LDS.
// These three are fast_path(K) (wave_path(K): the first); each solver also forms the candidate poses.
// Larger windows take launch_global_solve and the global-memory trial tail (ba_trial.hip).
hipError_t launch_solve(const Problem& P, const Active& A, const Sys& S, double lambda, hipStream_t s,
                        bool wave_fused) {
  const int n = 6 * A.K;
  if (!fast_path(A.K)) return hipErrorInvalidValue;
  if (wave_path(A.K)) {
    if (wave_fused) return hipSuccess;
    switch (A.K) {
#define RSPL_SOLVE_CASE(k) \
  case k: hipLaunchKernelGGL(schur_wave_kernel<6 * k>, dim3(1), dim3(64), 0, s, P, A, S, lambda); break;
      RSPL_SOLVE_CASE(1) RSPL_SOLVE_CASE(2) RSPL_SOLVE_CASE(3) RSPL_SOLVE_CASE(4) RSPL_SOLVE_CASE(5)
      RSPL_SOLVE_CASE(6) RSPL_SOLVE_CASE(7) RSPL_SOLVE_CASE(8) RSPL_SOLVE_CASE(9) RSPL_SOLVE_CASE(10)
#undef RSPL_SOLVE_CASE
      default: break;
    }
    return hipSuccess;
  }
  const hipError_t e = ensure_schur_attr();
  if (e != hipSuccess) return e;
  if (A.K <= kRegMaxK)
    hipLaunchKernelGGL(schur_reg_kernel, dim3(1), dim3(kSolveRegThreads), solve_reg_lds_bytes(A.K), s, P, A, S, n,
                       lambda);
  else
    hipLaunchKernelGGL(schur_solve_kernel, dim3(1), dim3(256), schur_lds_bytes(n), s, P, A, S, n, lambda);
  return hipSuccess;
}

void launch_global_solve(const Active& A, const Sys& S, double lambda, hipStream_t s) {
  const int n = 6 * A.K;
  if (n <= 0) return;
  hipLaunchKernelGGL(pair_final_kernel, dim3((A.npairs * 42 + 255) / 256), dim3(256), 0, s, A, S, lambda);
  hipLaunchKernelGGL(cholesky_kernel, dim3(1), dim3(256), 0, s, S, n);
}

}  // namespace ba
}  // namespace rspl
