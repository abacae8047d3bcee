// Local BA (see ba_device.hpp), first pass and bookkeeping: the first linearisation and the lambda-init
// statistic, the device-LM setup launch, the Schur chunks' edge-pair lists, outlier classification, the
// final kernel and the landmark-sharded fold / post / gather.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ba_kernels.hpp"
#include "ba_linearize.hpp"

namespace rspl {
namespace ba {

// mailbox post of the lambda-init statistic (max Hessian diagonal) after the first linearisation;
// with npd > 0 it first folds in the pose blocks: per pose, the npd block partials of
// pose_diag_kernel summed in order
__global__ __launch_bounds__(256) void post_kernel(Sys S, int K, int npd, unsigned long long seq) {
  __shared__ double part[4][64];
  if (npd > 0) {  // entry q = 6 pose + diagonal index: 4 waves each sum every 4th block partial
    const int lane = threadIdx.x & 63, pt = threadIdx.x >> 6, nq6 = 6 * K;
    double mx = 0;
    for (int q0 = 0; q0 < nq6; q0 += 64) {
      const int q = q0 + lane;
      double sacc = 0;
      if (q < nq6) {
        const int pa = q / 6, i = q - 6 * pa;
        const double* src = S.partial2 + (size_t)pa * npd * 6 + i;
        for (int b = pt; b < npd; b += 4) sacc += src[(size_t)b * 6];
      }
      part[pt][lane] = sacc;
      __syncthreads();
      if (pt == 0 && q < nq6) mx = fmax(mx, fabs(((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]));
      __syncthreads();
    }
    if (pt == 0) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
      if (lane == 0) S.out[2] = fmax(S.out[2], mx);
    }
  }
  if (threadIdx.x != 0) return;
  post_mail(S.mail, S.out[0], S.out[1], S.out[2],
            (double)__hip_atomic_load(S.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), seq);
}

// one launch for both landmark families: blocks [0, nbq) point landmarks (kGroup lanes
// each), blocks [nbq, ...) line edges (one wave each).  maxd: contribute the landmark
// diagonals to S.out[2] (computeLambdaInit); speculative passes leave it alone.
__global__ __launch_bounds__(256) void linearize_kernel(Problem P, Lin L, Active A, Sys S, int nbq, int maxd) {
  if ((int)blockIdx.x < nbq) lin_point_landmarks(P, L, A, S, blockIdx.x * 256 + threadIdx.x, maxd != 0);
  else lin_lines<kLinPlain>(P, L, A, S, blockIdx.x - nbq, maxd != 0);
}

// max diagonal of the pose blocks (computeLambdaInit), first iteration only.  Block b sums
// the Hpp diagonals of its 256 edges per reduced pose (fixed tree) into partial[a][b]; the
// post kernel sums each pose's partials in block order and takes
// the max.  wt: the partials are written through (read by the last block of the same launch).
__device__ __forceinline__ void pose_diag_block(const Problem& P, const Lin& L, const Active& A, const Sys& S, bool wt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  int a = -1;
  double d[6] = {0, 0, 0, 0, 0, 0};
  if (e < A.Ea) {
    a = A.pidx[P.epose[e]];
    if (a >= 0) {
      const double* H = L.Hpp + 21 * e;
#pragma unroll
      for (int i = 0; i < 6; i++) d[i] = H[pk6(i, i)];
    }
  }
  // per pose: each wave's butterfly (poses absent from the wave skipped), then the 4 wave sums in
  // wave order -- no block barrier per pose
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __shared__ double wsum[4][32][6];
  for (int p0 = 0; p0 < A.K; p0 += 32) {
    const int pn = min(32, A.K - p0);
    for (int j = 0; j < pn; j++) {
      const int pa = p0 + j;
      double acc[6];
#pragma unroll
      for (int i = 0; i < 6; i++) acc[i] = a == pa ? d[i] : 0.0;
      if (__ballot(a == pa)) {  // wave-uniform
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
          for (int i = 0; i < 6; i++) acc[i] += __shfl_xor(acc[i], o);
      }
      if (lane < 6) wsum[wv][j][lane] = acc[lane];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 6 * pn; q += 256) {
      const int j = q / 6, i = q - 6 * j;
      const double v = ((wsum[0][j][i] + wsum[1][j][i]) + wsum[2][j][i]) + wsum[3][j][i];
      double* dst = S.partial2 + ((size_t)(p0 + j) * gridDim.x + blockIdx.x) * 6 + i;
      if (wt) __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else *dst = v;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void pose_diag_kernel(Problem P, Lin L, Active A, Sys S) {
  pose_diag_block(P, L, A, S, false);
}

// pose_diag_block over the edge range [e0, e1) (a setup block's own edges, any length; rounds of 256
// summed per wave in round order): partial b of nb into dst[(a * nb + b) * 6 + i], written through.
// The block's record stores must be complete and visible (s_waitcnt + barrier) before the call.
__device__ __forceinline__ void pose_diag_range(const Problem& P, const Lin& L, const Active& A, double* dst, int nb,
                                                int b, int e0, int e1) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __shared__ double wsum[4][32][6];
  for (int p0 = 0; p0 < A.K; p0 += 32) {
    const int pn = min(32, A.K - p0);
    for (int j = 0; j < pn; j++)
      if (lane < 6) wsum[wv][j][lane] = 0.0;
    for (int eb = e0; eb < e1; eb += 256) {  // block-uniform
      const int e = eb + threadIdx.x;
      int a = -1;
      double d[6] = {0, 0, 0, 0, 0, 0};
      if (e < e1) {
        a = A.pidx[P.epose[e]];
        if (a >= 0) {
          const double* H = L.Hpp + 21 * e;
#pragma unroll
          for (int i = 0; i < 6; i++) d[i] = H[pk6(i, i)];
        }
      }
      for (int j = 0; j < pn; j++) {
        const int pa = p0 + j;
        double acc[6];
#pragma unroll
        for (int i = 0; i < 6; i++) acc[i] = a == pa ? d[i] : 0.0;
        if (__ballot(a == pa)) {  // wave-uniform
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
            for (int i = 0; i < 6; i++) acc[i] += __shfl_xor(acc[i], o);
        }
        if (lane < 6) wsum[wv][j][lane] += acc[lane];
      }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 6 * pn; q += 256) {
      const int j = q / 6, i = q - 6 * j;
      const double v = ((wsum[0][j][i] + wsum[1][j][i]) + wsum[2][j][i]) + wsum[3][j][i];
      __hip_atomic_store(dst + ((size_t)(p0 + j) * nb + b) * 6 + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
  }
}

// pose_diag_range from the per-edge diagonals a landmark block staged in LDS (pd / pa: the block's n CSR edges,
// pose index or -1): wave w sums its quarter of the edges per (pose, entry) in edge order, the four quarters
// then in wave order -- no wait for the block's record stores, no reload
constexpr int kPdCap = 512;  // edges per landmark block staged (more: pose_diag_range)
__device__ __forceinline__ void pose_diag_lds(const Active& A, const double (*pd)[6], const int* pa, int n, double* dst,
                                              int nb, int b) {
  __shared__ double ws[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l0 = (n * wv) / 4, l1 = (n * (wv + 1)) / 4, nq = 6 * A.K;
  for (int q0 = 0; q0 < nq; q0 += 64) {
    const int q = q0 + lane, j = q / 6, i = q - 6 * j;
    double sm = 0;
    if (q < nq)
      for (int l = l0; l < l1; l += 8) {  // eight LDS reads in flight, summed in edge order
        int pv[8];
        double dv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const bool ok = l + u < l1;
          pv[u] = ok ? pa[l + u] : -1;
          dv[u] = ok ? pd[l + u][i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) sm += pv[u] == j ? dv[u] : 0.0;
      }
    ws[wv][lane] = sm;
    __syncthreads();
    if (wv == 0 && q < nq)
      __hip_atomic_store(dst + ((size_t)j * nb + b) * 6 + i, ((ws[0][lane] + ws[1][lane]) + ws[2][lane]) + ws[3][lane],
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Schur complement for damping lambda
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// Schur complement for damping lambda
// ---------------------------------------------------------------------------
// Edge-pair lists, built once per call on the device.  Chunk c = (pose pair pr, landmark
// range lb) owns the segment [pp_off[c], pp_off[c+1]) of the (e1, e2) lists; within it the
// pairs follow landmark order, then i, then j (deterministic).  Lane l of round r handles
// landmark lb * lmchunk + 64 r + l; its matches are found from bit masks over batches of 8
// CSR entries (independent loads) and placed by a wave prefix sum in lane order.
template <bool FILL>
__device__ __forceinline__ void pair_scan(const Active& A, int c, int* pp_cnt, const int* pp_off, int4* pp) {
  const int lane = threadIdx.x & 63;
  int pr, g0, g1, nr;
  if (A.dsub <= 1) {  // (every pair nchk ranges of lmchunk)
    pr = c / A.nchk;
    g0 = (c - pr * A.nchk) * A.lmchunk;
    g1 = A.nL;
    nr = A.lmchunk / 64;
  } else {
    const ChunkGeo cg = chunk_geo(A, c);
    pr = cg.pr;
    g0 = cg.g0;
    g1 = cg.g1;
    nr = (cg.g1 - cg.g0 + 63) / 64;
  }
  const int pa = A.pairs[2 * pr], pb = A.pairs[2 * pr + 1];
  int base = FILL ? pp_off[c] : 0;
  const int lim = FILL ? pp_off[c + 1] : 0;  // the segment's end: offsets counted elsewhere (the host staging) never
                                             // let a store leave the chunk's segment
  // four landmark rounds at a time: their CSR ranges, then the first eight edge poses of each (a landmark's
  // whole edge list when it has <= 8 edges, the common case), every load of a group in flight at once
  for (int r0 = 0; r0 < nr; r0 += 4) {
    int k0[4], k1[4], pz[4][8];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int g = g0 + 64 * (r0 + u) + lane;
      const bool in = r0 + u < nr && g < g1;
      const int o0 = in ? A.lm_off[g] : 0, o1 = in ? A.lm_off[g + 1] : 0;
      const bool act = in && A.lm_act[g];
      k0[u] = act ? o0 : 0;
      k1[u] = act ? o1 : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int v = 0; v < 8; v++) pz[u][v] = k1[u] > k0[u] ? A.lm_pose[min(k0[u] + v, k1[u] - 1)] : -1;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (r0 + u >= nr) break;  // uniform
      const int g = g0 + 64 * (r0 + u) + lane;
      const int e0 = k0[u], e1 = k1[u];
      int cnt = 0;
      unsigned ma1 = 0, mb1 = 0;  // the masks when the landmark has <= 8 edges (one block each)
      if (e1 - e0 <= 8) {
        unsigned ma = 0, mb = 0;
#pragma unroll
        for (int v = 0; v < 8; v++) {
          ma |= (e0 + v < e1 && pz[u][v] == pa) ? 1u << v : 0u;
          mb |= (e0 + v < e1 && pz[u][v] == pb) ? 1u << v : 0u;
        }
        cnt = ma ? __popc(ma) * __popc(mb) : 0;
        ma1 = ma;
        mb1 = mb;
      } else {
        for (int ib = e0; ib < e1; ib += 8) {  // i blocks
          unsigned ma = 0;
          for (int v = 0; v < 8 && ib + v < e1; v++) ma |= A.lm_pose[ib + v] == pa ? 1u << v : 0u;
          if (!ma) continue;
          for (int jb = e0; jb < e1; jb += 8) {  // j blocks
            unsigned mb = 0;
            for (int v = 0; v < 8 && jb + v < e1; v++) mb |= A.lm_pose[jb + v] == pb ? 1u << v : 0u;
            cnt += __popc(ma) * __popc(mb);
          }
        }
      }
      // wave exclusive prefix of the per-lane counts (lane order)
      int pre = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(pre, o);
        if (lane >= o) pre += t;
      }
      const int total = __shfl(pre, 63);
      if (FILL && cnt && e1 - e0 <= 8) {  // emit from the masks: i ascending, then j ascending
        int q = base + pre - cnt;
        for (unsigned ma = ma1; ma; ma &= ma - 1) {
          const int ea = (e0 + __ffs(ma) - 1);
          for (unsigned mb = mb1; mb; mb &= mb - 1, q++)
            if (q < lim) pp[q] = make_int4(ea, (e0 + __ffs(mb) - 1), g, 0);
        }
      } else if (FILL && cnt) {
        int q = base + pre - cnt;
        for (int ib = e0; ib < e1; ib++) {
          if (A.lm_pose[ib] != pa) continue;
          for (int jb = e0; jb < e1; jb++) {
            if (A.lm_pose[jb] != pb) continue;
            if (q < lim) pp[q] = make_int4(ib, jb, g, 0);
            q++;
          }
        }
      }
      base += total;
    }
  }
  if (!FILL && lane == 0) __hip_atomic_store(pp_cnt + c, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(64) void pair_count_kernel(Active A, int* pp_cnt) {
  pair_scan<false>(A, blockIdx.x, pp_cnt, nullptr, nullptr);
}
__global__ __launch_bounds__(64) void pair_fill_kernel(Active A, const int* pp_off, int4* pp) {
  pair_scan<true>(A, blockIdx.x, nullptr, pp_off, pp);
}
// exclusive scan of the chunk counts (one workgroup; n = npairs * nchk + 1 offsets)
__global__ __launch_bounds__(1024) void pair_offsets_kernel(const int* cnt, int* off, int n) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  const int per = (n + 1023) / 1024, b0 = min(tid * per, n), b1 = min(b0 + per, n);
  int s = 0;
  for (int i = b0; i < b1; i++) s += cnt[i];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan of the partials
    const int t = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += t;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (int i = b0; i < b1; i++) {
    off[i] = run;
    run += cnt[i];
  }
  if (tid == 1023) off[n] = part[1023];
}

// ---------------------------------------------------------------------------
// The first pass of a device-LM optimize() in one launch (was: errors, [classify,
// landmark_active,] linearize, pose_diag, post; build_pairs' count and scan in the first optimize).
//   setup_kernel -- blocks [0, nbq): kGroup lanes per landmark (every landmark).  With `level` (the
//     second optimize) the outlier levels of the landmark's edges from their last computed errors
//     (classify_edge, g2o_optimization.cc:176-213) and its activity (landmark_active); for point
//     landmarks the errors and robust cost at the current state and the linearisation (edge records,
//     Hll / bl, the landmark diagonal maximum).  Blocks [nbq, nbq + n_lblk): the line workgroups
//     (lin_lines<kLinSetup>: classification, cost and linearisation of their own edges).  The cost of
//     block b goes to S.partial[b], its edges' pose-diagonal sums to pdg.  Then the last block of the
//     launch (ticket): the cost, the maximum diagonal and the LM control (computeLambdaInit).
// ---------------------------------------------------------------------------
__device__ __forceinline__ double setup_landmark(const Problem& P, const Lin& L, const Active& A, const Sys& S, int t,
                                                 uint8_t* level, uint8_t* lm_act2, double (*pd)[6] = nullptr,
                                                 int* pa = nullptr, int pe0 = 0) {
  const int g = t / kGroup, j = t % kGroup;
  const bool in = g < A.nL, point = g < P.nq;
  double hl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0}, chi = 0;
  int live = 0;
  if (in) {
    const int k1 = A.lm_off[g + 1];
    const double* Xg = P.X + 3 * g;
    for (int k = A.lm_off[g] + j; k < k1; k += kGroup) {
      bool lev = false;
      if (level && edge_outlier(P, L, k)) {
        lev = true;
        level[k] = 1;
      }
      live |= lev ? 0 : 1;
      if (!point) continue;  // line edges: the line workgroups
      const bool pose_opt = A.lm_pose[k] >= 0;
      if (pd) pa[k - pe0] = pose_opt ? A.lm_pose[k] : -1;  // (the block's edges: its pose-diagonal partials)
      if (lev) {  // outside this phase: exact-zero records, no cost, error kept
        if (pose_opt) zero_pose_records<true>(L, k);
        if (pd)
#pragma unroll
          for (int i = 0; i < 6; i++) pd[k - pe0][i] = 0.0;
        continue;
      }
      const int te = P.etype[k];
      const SE3 T = load_T(P.T + 8 * P.epose[k]);
      const double* cm = P.cams + 5 * P.ecam[k];
      double er[4];
      const double chi2 = point_error(te, cm, obs_of(P, k, te), T, Xg, er);
#pragma unroll
      for (int q = 0; q < 4; q++) L.err[4 * k + q] = er[q];
      double cst = chi2;
      if (A.robust) {
        double r1;
        huber(chi2, pick4(P.delta, te), cst, r1);
      }
      chi += cst;
      double dg6[6] = {0, 0, 0, 0, 0, 0};
      point_edge_core<true>(P, L, A, k, te, pose_opt, T, cm, Xg, er, hl, bv, dg6);
      if (pd)
#pragma unroll
        for (int i = 0; i < 6; i++) pd[k - pe0][i] = dg6[i];
    }
  }
#pragma unroll
  for (int o = 1; o < kGroup; o <<= 1) live |= __shfl_xor(live, o);
  const bool act = level ? live != 0 : (in && A.lm_act[g] != 0);
  if (level && in && j == 0) lm_act2[g] = act ? 1 : 0;
  group_sum(hl);
  group_sum(bv);
  if (in && point && j == 0 && act) {
    double* H = S.Hll + 16 * g;
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = hl[i];
#pragma unroll
    for (int i = 9; i < 16; i++) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) S.bl[4 * g + i] = bv[i];
    S.bl[4 * g + 3] = 0.0;
    atomic_max_pos(S.out + 2, fmax(fabs(hl[0]), fmax(fabs(hl[4]), fabs(hl[8]))));
  }
  return chi;
}

__device__ __forceinline__ void prof_max(const Sys& S, int slot) {  // latest over the blocks
  if (S.prof) atomicMax(S.prof + slot, (unsigned long long)wall_clock64());
}

// The first pass in ONE launch: blocks [0, nbq) landmark groups, [nbq, nb_lm) line workgroups,
// [nb_lm, ...) the edge-pair lists' fill (or count); every landmark / line block then sums the pose diagonals of
// its own edges (pose_diag_range -> pdg) and every block takes a ticket; the last block sums the cost
// partials and the pose-diagonal partials in block order, scans the pair counts (if counted here) and writes the LM
// control (round 3 did this in a second launch; one launch measured neutral, four per call instead of six).
__global__ __launch_bounds__(256) void setup_kernel(Problem P, Lin L, Active A, Sys S, int nbq, int nb_lm,
                                                    uint8_t* level, uint8_t* lm_act2, int4* pp_fill, int* pp_cnt,
                                                    int* pp_off, double* pdg, int lm_iters, int gate, Lin Ls,
                                                    Sys Ss) {
  __shared__ double red[4];
  __shared__ double part[4][64];
  __shared__ int last;
  if (gate >= 0) {  // queued behind the previous optimize()'s trials: only once it has stopped, on its bank
    const LmCtrl* c = S.lm + gate;
    if (!c->stop) return;
    if (c->cur) {
      bank_state(P);
      bank_lin(L, Ls, S, Ss);
    }
  }
  const int b = blockIdx.x;
  if (b == 0 && threadIdx.x == 0) prof_stamp(S, 9);
  if (b >= nb_lm) {  // the first optimize: the Schur chunks' edge-pair lists, one wave per chunk -- filled
                     // against the offsets the host staging counted (pp_fill; A.pp_off: in the call's upload),
                     // or only counted (pp_cnt: a call staged on its own chain; scanned below, filled by a launch)
    const int c = (b - nb_lm) * 4 + (threadIdx.x >> 6);
    if (c < chunk_count(A)) {
      if (pp_fill) pair_scan<true>(A, c, nullptr, A.pp_off, pp_fill);
      else pair_scan<false>(A, c, pp_cnt, nullptr, nullptr);
    }
    if (threadIdx.x == 0) prof_max(S, kProfX + 4);
  } else if (b >= nbq) {
    double c = 0.0;  // set in thread 0
    lin_lines<kLinSetup>(P, L, A, S, b - nbq, true, nullptr, nullptr, 0.0, false, nullptr, level != nullptr, &c, pdg,
                         nb_lm, b);  // (its edges' pose-diagonal partials too)
    if (threadIdx.x == 0) __hip_atomic_store(S.partial + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0) prof_max(S, kProfX + 2);
  } else {
    // this block's point landmarks' edges: one CSR range; their pose diagonals staged in LDS when they fit
    __shared__ double pd[kPdCap][6];
    __shared__ int pa[kPdCap];
    const int g0 = min(b * (256 / kGroup), P.nq), g1 = min(b * (256 / kGroup) + 256 / kGroup, P.nq);
    const int e0 = A.lm_off[g0], e1 = A.lm_off[g1];
    const bool staged = e1 - e0 <= kPdCap;
    double acc[1] = {setup_landmark(P, L, A, S, b * 256 + threadIdx.x, level, lm_act2, staged ? pd : nullptr, pa, e0)};
    block_reduce<1>(acc, red);  // (its barriers also order the staged diagonals)
    if (threadIdx.x == 0) __hip_atomic_store(S.partial + b, red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0) prof_max(S, kProfX + 0);
    if (staged) {
      pose_diag_lds(A, pd, pa, e1 - e0, pdg, nb_lm, b);
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      pose_diag_range(P, L, A, pdg, nb_lm, b, e0, e1);
    }
    if (threadIdx.x == 0) prof_max(S, kProfX + 1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) last = ticket(S.counter) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  // ---- the last block ----
  if (threadIdx.x == 0) prof_stamp(S, 10);
  double cs[1] = {0.0};  // the cost: the landmark / line blocks' partials, fixed order
  for (int k = threadIdx.x; k < nb_lm; k += 256) cs[0] += __hip_atomic_load(S.partial + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  block_reduce<1>(cs, red);
  const double chi2 = red[0];
  if (pp_cnt) {  // exclusive scan of the chunks' edge-pair counts -> pp_off
    __shared__ int sc[256];
    const int tid = threadIdx.x, nc = chunk_count(A);
    const int per = (nc + 255) / 256, b0 = min(tid * per, nc), b1 = min(b0 + per, nc);
    int sm = 0;
    for (int i = b0; i < b1; i++) sm += __hip_atomic_load(pp_cnt + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sc[tid] = sm;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // Hillis-Steele inclusive scan
      const int t = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += t;
      __syncthreads();
    }
    int run = sc[tid] - sm;
    for (int i = b0; i < b1; i++) {
      pp_off[i] = run;
      run += __hip_atomic_load(pp_cnt + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 255) pp_off[nc] = sc[255];
  }
  if (threadIdx.x == 0) prof_stamp(S, 11);
  // per pose and diagonal entry q = 6 pose + i: 4 waves each sum every 4th block partial
  const int lane = threadIdx.x & 63, pt = threadIdx.x >> 6, nq6 = 6 * A.K, npd = nb_lm;
  double mx = 0;
  for (int q0 = 0; q0 < nq6; q0 += 64) {
    const int q = q0 + lane;
    double sacc = 0;
    if (q < nq6) {
      const int pa = q / 6, i = q - 6 * pa;
      const double* src = pdg + (size_t)pa * npd * 6 + i;
      for (int b0 = pt; b0 < npd; b0 += 4 * 16) {  // 16 write-through loads in flight, summed in block order
        double t[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
          const int bb = b0 + 4 * u;
          t[u] = bb < npd ? __hip_atomic_load(src + (size_t)bb * 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 16; u++) sacc += t[u];
      }
    }
    part[pt][lane] = sacc;
    __syncthreads();
    if (pt == 0 && q < nq6) mx = fmax(mx, fabs(((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]));
    __syncthreads();
  }
  if (pt != 0) return;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  if (lane != 0) return;
  __hip_atomic_store(S.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  prof_stamp(S, 12);
  // the landmark diagonal maximum (atomic max of the landmark blocks: performed device-coherently)
  const double md = fmax(__hip_atomic_load(S.out + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), mx);
  S.out[0] = chi2;
  S.out[2] = md;
  LmCtrl* ctl = S.lm;  // slot 0: the first trial's (computeLambdaInit: tau = 1e-5 x max diagonal)
  ctl->lambda = 1e-5 * md;
  ctl->ni = 2;
  ctl->chi = chi2;
  ctl->cur = 0;
  ctl->it = 0;
  ctl->qmax = 0;
  ctl->stop = 0;
  ctl->iters = lm_iters;
  ctl->trials = 0;
}

__global__ __launch_bounds__(256) void landmark_active_kernel(Active A, const uint8_t* level, uint8_t* lm_act) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= A.nL) return;
  uint8_t on = 0;
  for (int k = A.lm_off[g]; k < A.lm_off[g + 1]; k++) on |= level[(k)] == 0;
  lm_act[g] = on;
}

__device__ __forceinline__ bool edge_inlier(const Problem& P, const Lin& L, int e) {
  double chi2;
  bool depth_ok;
  edge_status(P, L, e, chi2, depth_ok);
  return chi2 <= pick4(P.th, P.etype[e]) && depth_ok;
}
__device__ __forceinline__ void classify_edge(const Problem& P, const Lin& L, int e, uint8_t* level, uint8_t* inlier,
                                              int final_pass) {
  if (final_pass) {
    inlier[e] = edge_inlier(P, L, e) ? 1 : 0;
    return;
  }
  double chi2;
  bool depth_ok;
  edge_status(P, L, e, chi2, depth_ok);
  if (chi2 > pick4(P.th, P.etype[e]) || !depth_ok) level[e] = 1;
}

__global__ __launch_bounds__(256) void classify_kernel(Problem P, Lin L, int E, uint8_t* level, uint8_t* inlier,
                                                       int final_pass) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E) classify_edge(P, L, e, level, inlier, final_pass);
}

// end of a call: final inlier flags + the final T / X / L written straight into host-mapped
// memory; the last block (ticket) posts the mailbox once every block's writes are out.  Everything crosses
// PCIe as 16-byte stores: a block owns 256 consecutive flags of the caller's order -- thread t classifies the
// edge behind flag 256 b + t (ginv: caller edge id -> CSR position, scattered device reads), 16 threads then
// store the block's flags (inl is padded to 256 bytes: the last word's bytes past E are zeros) -- and a
// thread two doubles of T / X / L.
__global__ __launch_bounds__(256) void finish_kernel(Problem P, Lin L, int E, const int* ginv, uint8_t* inl, double* Th,
                                                     double* Xh, double* Lh, Sys S, unsigned long long seq) {
  __shared__ int last;
  __shared__ uint4 fl4[16];
  if (S.lm) {  // queued behind the last optimize()'s trials (S.lm_slot: the control after the last one):
               // a no-op unless that optimize() has stopped; the current bank from its control
    const LmCtrl* c = S.lm + S.lm_slot;
    if (!c->stop) return;
    if (c->cur) bank_state(P);
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  reinterpret_cast<uint8_t*>(fl4)[threadIdx.x] = i < E && edge_inlier(P, L, ginv[i]) ? 1 : 0;
  auto put2 = [i](double* dst, const double* src, int n) {
    if (2 * i + 1 < n) *reinterpret_cast<double2*>(dst + 2 * i) = make_double2(src[2 * i], src[2 * i + 1]);
    else if (2 * i < n) dst[2 * i] = src[2 * i];
  };
  put2(Th, P.T, 8 * P.np);
  put2(Xh, P.X, 3 * P.nq);
  put2(Lh, P.L, 6 * P.nl);
  __syncthreads();
  if (threadIdx.x < 16 && blockIdx.x * 256 + 16 * (int)threadIdx.x < E)
    reinterpret_cast<uint4*>(inl)[blockIdx.x * 16 + threadIdx.x] = fl4[threadIdx.x];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned tk = __hip_atomic_fetch_add(S.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last = tk == gridDim.x - 1;
  }
  __syncthreads();
  if (!last || threadIdx.x != 0) return;
  __hip_atomic_store(S.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&S.mail->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------
// landmark sharding (rspl_ba_set_shard): the pieces between the host's all-reduces
// ---------------------------------------------------------------------------
// this rank's pose-diagonal sums (block partials of pose_diag_kernel in block order) and its
// landmark maximum, laid out for the sum all-reduce
__global__ __launch_bounds__(256) void shard_fold_kernel(Sys S, double* red, int K, int npd, int rank, int nranks) {
  const int n6 = 6 * K;
  for (int q = threadIdx.x; q < n6; q += 256) {
    double acc = 0;
    if (npd > 0) {
      const int pa = q / 6, i = q - 6 * pa;
      const double* src = S.partial2 + (size_t)pa * npd * 6 + i;
      for (int b = 0; b < npd; b++) acc += src[(size_t)b * 6];
    }
    red[q] = acc;
  }
  for (int r = threadIdx.x; r < nranks; r += 256) red[n6 + r] = r == rank ? S.out[2] : 0.0;
}

__global__ void shard_post_kernel(Sys S, const double* red, int n6, int nranks, int mode, int add_pose_scale,
                                  unsigned long long seq) {
  __shared__ double mxs[64];
  const double* so = red + n6 + nranks;  // summed {chi2, scale, fail}
  double mx = 0;
  if (mode == 0) {
    for (int q = threadIdx.x; q < n6; q += 64) mx = fmax(mx, fabs(red[q]));
    for (int r = threadIdx.x; r < nranks; r += 64) mx = fmax(mx, red[n6 + r]);
  }
  mxs[threadIdx.x] = mx;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < 64; k++) mx = fmax(mx, mxs[k]);
  const double chi2 = so[0], scale = so[1] + (add_pose_scale ? S.out[4] : 0.0), f = so[2] != 0.0 ? 1.0 : 0.0;
  if (mode == 0) S.out[2] = mx;
  S.out[0] = chi2;
  S.out[1] = scale;
  S.out[3] = f;
  post_mail(S.mail, chi2, scale, mode == 0 ? mx : S.out[2], f, seq);
}

// G = [X (owned points) | L (owned lines) | inlier flag at the global edge id of each local edge]
__global__ __launch_bounds__(256) void shard_gather_kernel(Problem P, Lin L, int E, const int* gmap, int rank,
                                                           int nranks, double* G) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nq3 = 3 * P.nq, nl6 = 6 * P.nl;
  if (i < E) {
    G[nq3 + nl6 + gmap[i]] = edge_inlier(P, L, i) ? 1.0 : 0.0;
  }
  if (i < nq3 && (i / 3) % nranks == rank) G[i] = P.X[i];
  if (i < nl6 && (P.nq + i / 6) % nranks == rank) G[nq3 + i] = P.L[i];
}

__global__ __launch_bounds__(256) void shard_finish_kernel(Problem P, int E, const double* G, uint8_t* inl,
                                                           double* Th, double* Xh, double* Lh, Sys S,
                                                           unsigned long long seq) {
  __shared__ int last;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nq3 = 3 * P.nq, nl6 = 6 * P.nl;
  if (i < E) inl[i] = G[nq3 + nl6 + i] != 0.0;
  if (i < 8 * P.np) Th[i] = P.T[i];
  if (i < nq3) Xh[i] = G[i];
  if (i < nl6) Lh[i] = G[nq3 + i];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned tk = __hip_atomic_fetch_add(S.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last = tk == gridDim.x - 1;
  }
  __syncthreads();
  if (!last || threadIdx.x != 0) return;
  __hip_atomic_store(S.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&S.mail->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
int shard_red_len(int K, int nranks) { return 6 * K + nranks + 3; }

hipError_t linearize(const Problem& P, const Lin& L, const Active& A, const Sys& S, bool with_maxdiag,
                     hipStream_t s) {
  const int nbq = (P.nq * kGroup + 255) / 256, nbl = A.n_lblk;
  if (nbq + nbl > 0)
    hipLaunchKernelGGL(linearize_kernel, dim3(nbq + nbl), dim3(256), 0, s, P, L, A, S, nbq, with_maxdiag ? 1 : 0);
  if (with_maxdiag && A.K > 0 && A.Ea > 0)
    hipLaunchKernelGGL(pose_diag_kernel, dim3((A.Ea + 255) / 256), dim3(256), 0, s, P, L, A, S);
  return hipGetLastError();
}

int setup_pdg_len(const Active& A) {
  const int nbq = A.nL > 0 ? (A.nL * kGroup + 255) / 256 : 0;
  return 6 * A.K * (nbq + A.n_lblk) + 6;
}

hipError_t setup_dev(const Problem& P, const Lin& L, const Active& A, Sys& S, uint8_t* level, uint8_t* lm_act2,
                     int lm_iters, int4* pp, int* pp_cnt, int* pp_off, double* pdg, hipStream_t s, int gate,
                     const Lin* Ls, const Sys* Ss) {
  if (gate >= 0 && (!Ls || !Ss || pp)) return hipErrorInvalidValue;
  if (pp_cnt && !pp_off) return hipErrorInvalidValue;
  if (!S.lm || lm_iters <= 0) return hipErrorInvalidValue;
  Active A0 = A;
  A0.elevel = nullptr;  // the levels are written by this launch (level != null), never read by it
  const int nc = chunk_count(A);
  if (nc == 0) pp = nullptr;
  if (!pp) pp_cnt = nullptr;
  int4* const pp_fill = pp_cnt ? nullptr : pp;  // staged offsets: the first pass fills the lists itself
  const int nbq = A.nL > 0 ? (A.nL * kGroup + 255) / 256 : 0, nb = nbq + A.n_lblk;
  const int nbp = pp ? (nc + 3) / 4 : 0;
  // at least one block: the last one writes the LM control
  hipLaunchKernelGGL(setup_kernel, dim3(std::max(nb + nbp, 1)), dim3(256), 0, s, P, L, A0, S, nbq, nb, level, lm_act2,
                     pp_fill, pp_cnt, pp_off, pdg, lm_iters, gate, Ls ? *Ls : L, Ss ? *Ss : S);
  if (pp_cnt) hipLaunchKernelGGL(pair_fill_kernel, dim3(nc), dim3(64), 0, s, A, pp_off, pp);
  return hipGetLastError();
}

hipError_t post(Sys& S, unsigned long long seq, hipStream_t s, const Active* A) {
  const int npd = (A && A->K > 0 && A->Ea > 0) ? (A->Ea + 255) / 256 : 0;
  hipLaunchKernelGGL(post_kernel, dim3(1), dim3(256), 0, s, S, A ? A->K : 0, npd, seq);
  return hipGetLastError();
}

hipError_t finish(const Problem& P, const Lin& L, int E, const int* ginv, uint8_t* inl, double* Th, double* Xh,
                  double* Lh, Sys& S, unsigned long long seq, hipStream_t s) {
  const int n = std::max(std::max(E, 4 * P.np), std::max((3 * P.nq + 1) / 2, 3 * P.nl));  // a flag / two doubles each
  hipLaunchKernelGGL(finish_kernel, dim3(std::max((n + 255) / 256, 1)), dim3(256), 0, s, P, L, E, ginv, inl, Th, Xh,
                     Lh, S, seq);
  return hipGetLastError();
}

hipError_t build_pairs(const Active& A, int* pp_cnt, int* pp_off, int4* pp, hipStream_t s) {
  const int nc = chunk_count(A);
  if (nc == 0) return hipSuccess;
  hipLaunchKernelGGL(pair_count_kernel, dim3(nc), dim3(64), 0, s, A, pp_cnt);
  hipLaunchKernelGGL(pair_offsets_kernel, dim3(1), dim3(1024), 0, s, pp_cnt, pp_off, nc);
  hipLaunchKernelGGL(pair_fill_kernel, dim3(nc), dim3(64), 0, s, A, pp_off, pp);
  return hipGetLastError();
}

hipError_t landmark_active(const Active& A, const uint8_t* level, uint8_t* lm_act, hipStream_t s) {
  if (A.nL > 0) hipLaunchKernelGGL(landmark_active_kernel, dim3((A.nL + 255) / 256), dim3(256), 0, s, A, level, lm_act);
  return hipGetLastError();
}

hipError_t classify(const Problem& P, const Lin& L, int E, uint8_t* level, uint8_t* inlier, int final_pass,
                    hipStream_t s) {
  if (E > 0) hipLaunchKernelGGL(classify_kernel, dim3((E + 255) / 256), dim3(256), 0, s, P, L, E, level, inlier,
                                final_pass);
  return hipGetLastError();
}

hipError_t shard_fold(const Active& A, Sys& S, double* red, int rank, int nranks, hipStream_t s) {
  const int npd = (A.K > 0 && A.Ea > 0) ? (A.Ea + 255) / 256 : 0;
  hipLaunchKernelGGL(shard_fold_kernel, dim3(1), dim3(256), 0, s, S, red, A.K, npd, rank, nranks);
  return hipGetLastError();
}

hipError_t shard_post(Sys& S, const double* red, int n6, int nranks, int mode, int add_pose_scale,
                      unsigned long long seq, hipStream_t s) {
  hipLaunchKernelGGL(shard_post_kernel, dim3(1), dim3(64), 0, s, S, red, n6, nranks, mode, add_pose_scale, seq);
  return hipGetLastError();
}

hipError_t shard_gather(const Problem& P, const Lin& L, int E, const int* gmap, int rank, int nranks, double* G,
                        hipStream_t s) {
  const int n = std::max(E, std::max(3 * P.nq, 6 * P.nl));
  if (n > 0)
    hipLaunchKernelGGL(shard_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, P, L, E, gmap, rank, nranks, G);
  return hipGetLastError();
}

hipError_t shard_finish(const Problem& P, int E_global, const double* G, uint8_t* inl, double* Th, double* Xh,
                        double* Lh, Sys& S, unsigned long long seq, hipStream_t s) {
  const int n = std::max(std::max(E_global, 8 * P.np), std::max(3 * P.nq, 6 * P.nl));
  hipLaunchKernelGGL(shard_finish_kernel, dim3(std::max((n + 255) / 256, 1)), dim3(256), 0, s, P, E_global, G, inl,
                     Th, Xh, Lh, S, seq);
  return hipGetLastError();
}

}  // namespace ba
}  // namespace rspl
