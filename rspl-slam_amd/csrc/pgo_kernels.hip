// Pose-graph optimisation on a tile-sparse fp64 Cholesky (loop closure).
//   pgo_linearise_kernel    one thread per edge: the blocks J^T W J (ii, ij, jj), the gradient parts, the cost, the residual
//   pgo_gradient_kernel     one thread per entry of b: -sum of the pose's gradient parts, and diag H, both through the
//                           pose -> edge table in ascending edge order
//   pgo_reduce_kernel       one workgroup: the cost in a fixed tree, then max diag H (after a linearisation) or
//                           delta^T (lambda delta + b) and max |delta| (after a trial), to host-mapped memory
//   pgo_assemble_kernel     one workgroup per filled tile: zero (ones on the padding diagonal), then every 6 x 6 block of
//                           the tile summed over its edge list in ascending edge order, lambda on the diagonal
//   pgo_factor_diag_kernel  column k: Cholesky of the diagonal tile, its lower triangle packed in one workgroup's LDS
//   pgo_trsm_kernel         column k: X L_kk^T = A for 16 rows of one tile below the diagonal per workgroup
//   pgo_update_kernel       column k: A_ij -= L_ik L_jk^T for every pair of filled tiles i >= j of the column, one
//                           workgroup per pair, 6 x 6 accumulator tiles of v_mfma_f64_16x16x4_f64 over four waves
//   pgo_substitute_kernel   one workgroup walks the columns forward (L y = b) and backward (L^T delta = y)
//   pgo_trial_kernel        one thread per pose and edge: the trial poses, and each edge's cost at them
// Workgroups meet at kernel boundaries only; no atomics, every sum has one order, so a solve repeats bit for bit.
#include "pgo_kernels.hpp"

namespace rspl {
namespace pgo {
namespace {

constexpr int T = 256;
typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(T) void pgo_linearise_kernel(DArgs a) {
  const int e = blockIdx.x * T + threadIdx.x;
  if (e >= a.n_edges) return;
  const int i = a.edge_i[e], j = a.edge_j[e];
  EdgeGeometry g;
  edge_residual(a.q + 4 * (size_t)i, a.p + 3 * (size_t)i, a.q + 4 * (size_t)j, a.p + 3 * (size_t)j,
                a.edge_q + 4 * (size_t)e, a.edge_p + 3 * (size_t)e, g);
  const double wt = a.edge_w[2 * (size_t)e], wr = a.edge_w[2 * (size_t)e + 1];
  double* blk = a.eblk + 108 * (size_t)e;
  edge_blocks(g, wt, wr, blk, blk + 36, blk + 72, a.eg + 12 * (size_t)e, a.eg + 12 * (size_t)e + 6);
  a.ecost[e] = edge_cost(g.e, wt, wr);
  for (int c = 0; c < 6; c++) a.eres[6 * (size_t)e + c] = g.e[c];
}

__global__ __launch_bounds__(T) void pgo_gradient_kernel(DArgs a) {
  const int t = blockIdx.x * T + threadIdx.x;
  if (t >= a.nt * kTile) return;
  const int f = t / kPoseDim, c = t % kPoseDim;
  double g = 0, d = 0;
  if (f < a.n_free)
    for (int m = a.pose_off[f]; m < a.pose_off[f + 1]; m++) {
      const int packed = a.pose_contrib[m], e = packed >> 1, side = packed & 1;
      g += a.eg[12 * (size_t)e + 6 * side + c];
      d += a.eblk[108 * (size_t)e + 72 * side + 7 * c];
    }
  a.b[t] = -g;
  a.hdiag[t] = d;
}

__device__ __forceinline__ double block_sum(double* sh, double v) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

__device__ __forceinline__ double block_max(double* sh, double v) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = fmax(sh[tid], sh[tid + s]);
    __syncthreads();
  }
  return sh[0];
}

// after_trial: 0 after a linearisation, 1 after a trial
__global__ __launch_bounds__(T) void pgo_reduce_kernel(DArgs a, double lambda, int after_trial) {
  __shared__ double sh[T];
  const int tid = threadIdx.x, n = a.n_free * kPoseDim;
  double c = 0;
  for (int e = tid; e < a.n_edges; e += T) c += a.ecost[e];
  c = block_sum(sh, c);
  double s0 = 0, s1 = 0;
  if (after_trial) {
    for (int t = tid; t < n; t += T) {
      const double d = a.delta[t];
      s0 += d * (lambda * d + a.b[t]);
      s1 = fmax(s1, fabs(d));
    }
    s0 = block_sum(sh, s0);
  } else {
    for (int t = tid; t < n; t += T) s1 = fmax(s1, a.hdiag[t]);
  }
  s1 = block_max(sh, s1);
  if (tid == 0) {
    a.out->cost = c;
    a.out->pred = s0;
    a.out->max_step = after_trial ? s1 : 0.0;
    a.out->max_diag = after_trial ? 0.0 : s1;
    a.out->bad_pivot = after_trial ? *a.flag : 0;
  }
}

__global__ __launch_bounds__(T) void pgo_assemble_kernel(DArgs a, double lambda) {
  const int t = blockIdx.x, tid = threadIdx.x;
  const int I = a.tile_row[t], J = a.tile_col[t];
  double* tile = a.tiles + (size_t)t * kTileElems;
  if (t == 0 && tid == 0) *a.flag = 0;
  const int live = a.n_free * kPoseDim - I * kTile;  // rows of this tile row that hold a free pose
  for (int idx = tid; idx < kTileElems; idx += T) {
    const int r = idx / kTile, c = idx % kTile;
    tile[idx] = (I == J && r == c && r >= live) ? 1.0 : 0.0;
  }
  __syncthreads();  // the zeros are written before the blocks, which other threads write
  const int b0 = a.tile_blk_off[t], nb = a.tile_blk_off[t + 1] - b0;
  for (int item = tid; item < nb * 36; item += T) {
    const int b = b0 + item / 36, ent = item % 36, ra = ent / 6, ca = ent % 6;
    const int pos = a.blk_pos[b], lr = pos >> 4, lc = pos & 15;
    double s = 0;
    for (int m = a.blk_off[b]; m < a.blk_off[b + 1]; m++) s += block_entry(a.eblk, a.blk_contrib[m], ra, ca);
    if (I == J && lr == lc && ra == ca) s += lambda;
    tile[(lr * kPoseDim + ra) * kTile + lc * kPoseDim + ca] = s;
  }
}

__global__ __launch_bounds__(T) void pgo_factor_diag_kernel(DArgs a, int k) {
  __shared__ double Ls[kTriElems];
  if (*a.flag) return;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double* tile = a.tiles + (size_t)a.col_diag[k] * kTileElems;
  for (int idx = tid; idx < kTileElems; idx += T) {
    const int r = idx / kTile, c = idx % kTile;
    if (c <= r) Ls[tri(r, c)] = tile[idx];
  }
  __syncthreads();
  for (int c = 0; c < kTile; c++) {
    const double d = Ls[tri(c, c)];  // the same value in every thread: the branch below is uniform
    if (!(d > 0.0)) {
      if (tid == 0) *a.flag = 1;
      return;
    }
    __syncthreads();  // every thread has read the pivot
    const double ld = sqrt(d);
    if (tid == 0)
      Ls[tri(c, c)] = ld;
    else if (c + tid < kTile)
      Ls[tri(c + tid, c)] /= ld;
    __syncthreads();
    for (int r = c + 1 + ty; r < kTile; r += 16) {
      const double lrc = Ls[tri(r, c)];
      for (int c2 = c + 1 + tx; c2 <= r; c2 += 16) Ls[tri(r, c2)] -= lrc * Ls[tri(c2, c)];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < kTileElems; idx += T) {
    const int r = idx / kTile, c = idx % kTile;
    if (c <= r) tile[idx] = Ls[tri(r, c)];
  }
}

constexpr int kTrsmRows = 16, kTrsmPitch = kTile + 1;

// grid: 6 row groups per tile below the diagonal of column k
__global__ __launch_bounds__(T) void pgo_trsm_kernel(DArgs a, int k) {
  __shared__ double Ls[kTriElems];
  __shared__ double Xs[kTrsmRows * kTrsmPitch];
  if (*a.flag) return;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int sub = blockIdx.x / (kTile / kTrsmRows), grp = blockIdx.x % (kTile / kTrsmRows);
  const double* diag = a.tiles + (size_t)a.col_diag[k] * kTileElems;
  double* rows = a.tiles + (size_t)a.col_tile[a.col_off[k] + sub] * kTileElems + (size_t)grp * kTrsmRows * kTile;
  for (int idx = tid; idx < kTileElems; idx += T) {
    const int r = idx / kTile, c = idx % kTile;
    if (c <= r) Ls[tri(r, c)] = diag[idx];
  }
  for (int idx = tid; idx < kTrsmRows * kTile; idx += T) Xs[(idx / kTile) * kTrsmPitch + idx % kTile] = rows[idx];
  __syncthreads();
  double* x = Xs + ty * kTrsmPitch;  // this thread's row; its 16 threads share the columns
  for (int c = 0; c < kTile; c++) {
    if (tx == 0) x[c] /= Ls[tri(c, c)];
    __syncthreads();
    const double xc = x[c];
    for (int c2 = c + 1 + tx; c2 < kTile; c2 += 16) x[c2] -= xc * Ls[tri(c2, c)];
    __syncthreads();
  }
  for (int idx = tid; idx < kTrsmRows * kTile; idx += T) rows[idx] = Xs[(idx / kTile) * kTrsmPitch + idx % kTile];
}

constexpr int kSlab = 32, kPitch = kSlab + 2;  // lmap_global.hip's LDS image: [row][k], 16-byte aligned rows
constexpr int kUnits = kSlab / 2, kLoads = kTile * kUnits / T;
constexpr int kSub = kTile / 16, kSubPerWave = kSub * kSub / 4;
static_assert(kTile * kUnits % T == 0 && kSub * kSub % 4 == 0 && kTile % kSlab == 0, "update geometry");

// grid (n, n) over the n tiles below the diagonal of column k: block (x, y), x >= y, owns the pair
__global__ __launch_bounds__(T) void pgo_update_kernel(DArgs a, int k) {
  __shared__ double As[kTile * kPitch];
  __shared__ double Bs[kTile * kPitch];
  if (blockIdx.x < blockIdx.y) return;
  if (*a.flag) return;
  const int off = a.col_off[k];
  const int I = a.col_row[off + blockIdx.x], J = a.col_row[off + blockIdx.y];
  const int ct = a.tile_map[I * a.nt + J];
  if (ct < 0) return;  // never: the symbolic factorisation filled it
  const double* A = a.tiles + (size_t)a.col_tile[off + blockIdx.x] * kTileElems;
  const double* B = a.tiles + (size_t)a.col_tile[off + blockIdx.y] * kTileElems;
  double* C = a.tiles + (size_t)ct * kTileElems;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;

  v4d acc[kSubPerWave];
#pragma unroll
  for (int n = 0; n < kSubPerWave; n++) acc[n] = v4d{0.0, 0.0, 0.0, 0.0};

  for (int s = 0; s < kTile / kSlab; s++) {
    __syncthreads();  // the previous slab's reads are done
#pragma unroll
    for (int j = 0; j < kLoads; j++) {
      const int u = tid + T * j, row = u / kUnits, col = u % kUnits;
      const size_t g = (size_t)row * kTile + s * kSlab + 2 * col;
      *reinterpret_cast<v2d*>(As + row * kPitch + 2 * col) = *reinterpret_cast<const v2d*>(A + g);
      *reinterpret_cast<v2d*>(Bs + row * kPitch + 2 * col) = *reinterpret_cast<const v2d*>(B + g);
    }
    __syncthreads();
    // A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]: both images are [row][k]
#pragma unroll
    for (int ks = 0; ks < kSlab / 4; ks++) {
#pragma unroll
      for (int n = 0; n < kSubPerWave; n++) {
        const int st = wv * kSubPerWave + n, ti = st / kSub, tj = st % kSub;
        const double av = As[(16 * ti + lr) * kPitch + 4 * ks + lq];
        const double bv = Bs[(16 * tj + lr) * kPitch + 4 * ks + lq];
        acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[n], 0, 0, 0);
      }
    }
  }
  // C/D: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int n = 0; n < kSubPerWave; n++) {
    const int st = wv * kSubPerWave + n, ti = st / kSub, tj = st % kSub;
#pragma unroll
    for (int r = 0; r < 4; r++) C[(16 * ti + lq + 4 * r) * kTile + 16 * tj + lr] -= acc[n][r];
  }
}

__global__ __launch_bounds__(T) void pgo_substitute_kernel(DArgs a) {
  __shared__ double Ls[kTriElems];
  __shared__ double ys[kTile], xs[kTile];
  if (*a.flag) return;
  const int tid = threadIdx.x, nt = a.nt;
  for (int t = tid; t < nt * kTile; t += T) a.y[t] = a.b[t];
  __syncthreads();
  // L y = b, column by column: solve the diagonal tile, then take the column's tiles off the rows below
  for (int k = 0; k < nt; k++) {
    const double* diag = a.tiles + (size_t)a.col_diag[k] * kTileElems;
    for (int idx = tid; idx < kTileElems; idx += T) {
      const int r = idx / kTile, c = idx % kTile;
      if (c <= r) Ls[tri(r, c)] = diag[idx];
    }
    if (tid < kTile) ys[tid] = a.y[k * kTile + tid];
    __syncthreads();
    for (int c = 0; c < kTile; c++) {
      const double xc = ys[c] / Ls[tri(c, c)];
      if (tid == c) xs[c] = xc;
      if (tid > c && tid < kTile) ys[tid] -= Ls[tri(tid, c)] * xc;
      __syncthreads();
    }
    if (tid < kTile) a.y[k * kTile + tid] = xs[tid];
    const int off = a.col_off[k], n_sub = a.col_off[k + 1] - off;
    for (int w = tid; w < n_sub * kTile; w += T) {
      const int sub = w / kTile, r = w % kTile;
      const double* row = a.tiles + (size_t)a.col_tile[off + sub] * kTileElems + (size_t)r * kTile;
      double s = 0;
      for (int c = 0; c < kTile; c++) s += row[c] * xs[c];
      a.y[a.col_row[off + sub] * kTile + r] -= s;
    }
    __syncthreads();
  }
  // L^T delta = y, from the last column back
  for (int k = nt - 1; k >= 0; k--) {
    const double* diag = a.tiles + (size_t)a.col_diag[k] * kTileElems;
    for (int idx = tid; idx < kTileElems; idx += T) {
      const int r = idx / kTile, c = idx % kTile;
      if (c <= r) Ls[tri(r, c)] = diag[idx];
    }
    if (tid < kTile) {
      const int off = a.col_off[k], n_sub = a.col_off[k + 1] - off;
      double s = 0;
      for (int sub = 0; sub < n_sub; sub++) {
        const double* col = a.tiles + (size_t)a.col_tile[off + sub] * kTileElems + tid;
        const double* x = a.delta + a.col_row[off + sub] * kTile;
        for (int r = 0; r < kTile; r++) s += col[(size_t)r * kTile] * x[r];
      }
      ys[tid] = a.y[k * kTile + tid] - s;
    }
    __syncthreads();
    for (int c = kTile - 1; c >= 0; c--) {
      const double xc = ys[c] / Ls[tri(c, c)];
      if (tid == c) xs[c] = xc;
      if (tid < c) ys[tid] -= Ls[tri(c, tid)] * xc;
      __syncthreads();
    }
    if (tid < kTile) a.delta[k * kTile + tid] = xs[tid];
    __syncthreads();
  }
}

__device__ __forceinline__ void trial_pose(const DArgs& a, int i, double* q, double* p) {
  const int f = a.pose_free[i];
  if (f >= 0) {
    pose_update(a.q + 4 * (size_t)i, a.p + 3 * (size_t)i, a.delta + kPoseDim * (size_t)f, q, p);
  } else {
    for (int c = 0; c < 4; c++) q[c] = a.q[4 * (size_t)i + c];
    for (int c = 0; c < 3; c++) p[c] = a.p[3 * (size_t)i + c];
  }
}

__global__ __launch_bounds__(T) void pgo_trial_kernel(DArgs a) {
  if (*a.flag) return;
  const int t = blockIdx.x * T + threadIdx.x;
  if (t < a.n_poses) {
    double q[4], p[3];
    trial_pose(a, t, q, p);
    for (int c = 0; c < 4; c++) a.tq[4 * (size_t)t + c] = q[c];
    for (int c = 0; c < 3; c++) a.tp[3 * (size_t)t + c] = p[c];
  }
  if (t < a.n_edges) {
    double qi[4], pi[3], qj[4], pj[3];
    trial_pose(a, a.edge_i[t], qi, pi);
    trial_pose(a, a.edge_j[t], qj, pj);
    EdgeGeometry g;
    edge_residual(qi, pi, qj, pj, a.edge_q + 4 * (size_t)t, a.edge_p + 3 * (size_t)t, g);
    a.ecost[t] = edge_cost(g.e, a.edge_w[2 * (size_t)t], a.edge_w[2 * (size_t)t + 1]);
  }
}

inline int blocks(int n) { return (n + T - 1) / T; }

}  // namespace

#define PGO_LAUNCHED()                     \
  do {                                     \
    const hipError_t e = hipGetLastError(); \
    if (e != hipSuccess) return e;         \
  } while (0)

hipError_t launch_linearise(const DArgs& a, hipStream_t s) {
  if (a.n_edges > 0) {
    pgo_linearise_kernel<<<blocks(a.n_edges), T, 0, s>>>(a);
    PGO_LAUNCHED();
  }
  if (a.nt > 0) {
    pgo_gradient_kernel<<<blocks(a.nt * kTile), T, 0, s>>>(a);
    PGO_LAUNCHED();
  }
  pgo_reduce_kernel<<<1, T, 0, s>>>(a, 0.0, 0);
  return hipGetLastError();
}

hipError_t launch_assemble(const DArgs& a, int n_filled, double lambda, hipStream_t s) {
  pgo_assemble_kernel<<<n_filled, T, 0, s>>>(a, lambda);
  return hipGetLastError();
}

hipError_t launch_factor(const DArgs& a, const int32_t* host_col_off, hipStream_t s) {
  for (int k = 0; k < a.nt; k++) {
    pgo_factor_diag_kernel<<<1, T, 0, s>>>(a, k);
    PGO_LAUNCHED();
    const int n = host_col_off[k + 1] - host_col_off[k];
    if (n == 0) continue;
    pgo_trsm_kernel<<<n * (kTile / kTrsmRows), T, 0, s>>>(a, k);
    PGO_LAUNCHED();
    pgo_update_kernel<<<dim3(n, n), T, 0, s>>>(a, k);
    PGO_LAUNCHED();
  }
  return hipSuccess;
}

hipError_t launch_substitute(const DArgs& a, hipStream_t s) {
  pgo_substitute_kernel<<<1, T, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_trial(const DArgs& a, double lambda, hipStream_t s) {
  const int n = a.n_poses > a.n_edges ? a.n_poses : a.n_edges;
  pgo_trial_kernel<<<blocks(n), T, 0, s>>>(a);
  PGO_LAUNCHED();
  pgo_reduce_kernel<<<1, T, 0, s>>>(a, lambda, 1);
  return hipGetLastError();
}

}  // namespace pgo
}  // namespace rspl
