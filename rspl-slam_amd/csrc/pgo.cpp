// Pose-graph optimisation (loop closure): C ABI rspl_pgo_* over pgo_kernels.hip.
//   Plan          the free-pose numbering, the tile-level symbolic Cholesky, and the tables both sides gather through
//   lm_solve      the LM rule, once, over a backend: DeviceSide launches the kernels and synchronises once per trial,
//                 HostSide (rspl_pgo_debug_host) runs the same pgo_solve.hpp text on plain C++ tiles
// The reference has no such stage; tests/pgo_ref.py restates the contract.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "pgo_kernels.hpp"

using namespace rspl;
using pgo::kPoseDim;
using pgo::kTile;
using pgo::kTileElems;
using pgo::kTilePoses;

namespace {

struct Plan {
  int n_poses = 0, n_edges = 0, n_free = 0, nt = 0, n_struct = 0, n_filled = 0;
  std::vector<int32_t> pose_free;
  std::vector<int32_t> tile_map, tile_row, tile_col;
  std::vector<int32_t> tile_blk_off, blk_pos, blk_off, blk_contrib;
  std::vector<int32_t> pose_off, pose_contrib;
  std::vector<int32_t> col_diag, col_off, col_tile, col_row;
};

struct BlockRef {
  int32_t tile, fa, fb, edge, kind;  // edge -1: the block exists (a free pose's diagonal) with nothing to add yet
  bool operator<(const BlockRef& o) const {
    if (tile != o.tile) return tile < o.tile;
    if (fa != o.fa) return fa < o.fa;
    if (fb != o.fb) return fb < o.fb;
    return edge < o.edge;
  }
};

int find_root(std::vector<int32_t>& parent, int x) {
  while (parent[x] != x) {
    parent[x] = parent[parent[x]];
    x = parent[x];
  }
  return x;
}

int check_problem(const rspl_pgo_problem* P) {
  RSPL_CHECK_ARG(P, "rspl_pgo: NULL problem");
  RSPL_CHECK_ARG(P->n_poses > 0 && P->n_edges >= 0, "rspl_pgo: %d poses, %d edges", P->n_poses, P->n_edges);
  RSPL_CHECK_ARG(P->pose_q && P->pose_p && P->pose_fixed, "rspl_pgo: NULL pose array");
  RSPL_CHECK_ARG(P->n_edges == 0 || (P->edge_i && P->edge_j && P->edge_q && P->edge_p && P->edge_w),
                 "rspl_pgo: NULL edge array");
  if (P->n_poses > pgo::kMaxPoses) {
    set_error("rspl_pgo: %d poses exceed %d", P->n_poses, pgo::kMaxPoses);
    return RSPL_E_CAPACITY;
  }
  return RSPL_OK;
}

// the refusals of the contract, then the plan
int make_plan(const rspl_pgo_problem& P, Plan& pl) {
  const int n = P.n_poses, E = P.n_edges;
  pl.n_poses = n;
  pl.n_edges = E;
  pl.pose_free.assign(n, -1);
  int n_fixed = 0, nf = 0;
  for (int i = 0; i < n; i++) {
    if (P.pose_fixed[i])
      n_fixed++;
    else
      pl.pose_free[i] = nf++;
  }
  RSPL_CHECK_ARG(n_fixed > 0, "rspl_pgo: no fixed pose");
  std::vector<int32_t> parent(n);
  std::iota(parent.begin(), parent.end(), 0);
  std::vector<char> has_edge(n, 0);
  for (int e = 0; e < E; e++) {
    const int i = P.edge_i[e], j = P.edge_j[e];
    RSPL_CHECK_ARG(i >= 0 && i < n && j >= 0 && j < n, "rspl_pgo: edge %d (%d, %d) out of range", e, i, j);
    RSPL_CHECK_ARG(i != j, "rspl_pgo: edge %d joins pose %d to itself", e, i);
    has_edge[i] = has_edge[j] = 1;
    const int a = find_root(parent, i), b = find_root(parent, j);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
  }
  std::vector<char> anchored(n, 0);
  for (int i = 0; i < n; i++)
    if (P.pose_fixed[i]) anchored[find_root(parent, i)] = 1;
  for (int i = 0; i < n; i++)
    RSPL_CHECK_ARG(P.pose_fixed[i] || !has_edge[i] || anchored[find_root(parent, i)],
                   "rspl_pgo: the component of free pose %d holds no fixed pose (gauge freedom)", i);

  pl.n_free = nf;
  const int nt = pl.nt = (nf + kTilePoses - 1) / kTilePoses;
  // structure: every diagonal tile, and the tile of every edge between two free poses
  std::vector<char> filled((size_t)nt * nt, 0);
  for (int t = 0; t < nt; t++) filled[(size_t)t * nt + t] = 1;
  std::vector<BlockRef> refs;
  refs.reserve(nf + 3 * (size_t)E);
  for (int f = 0; f < nf; f++) refs.push_back({0, f, f, -1, 0});
  std::vector<std::vector<int32_t>> per_pose(nf);
  for (int e = 0; e < E; e++) {
    const int fi = pl.pose_free[P.edge_i[e]], fj = pl.pose_free[P.edge_j[e]];
    if (fi >= 0) {
      refs.push_back({0, fi, fi, e, pgo::kBlockII});
      per_pose[fi].push_back(2 * e);
    }
    if (fj >= 0) {
      refs.push_back({0, fj, fj, e, pgo::kBlockJJ});
      per_pose[fj].push_back(2 * e + 1);
    }
    if (fi >= 0 && fj >= 0) {
      if (fi > fj)
        refs.push_back({0, fi, fj, e, pgo::kBlockIJ});
      else
        refs.push_back({0, fj, fi, e, pgo::kBlockIJT});
      filled[(size_t)(std::max(fi, fj) / kTilePoses) * nt + std::min(fi, fj) / kTilePoses] = 1;
    }
  }
  pl.n_struct = (int)std::count(filled.begin(), filled.end(), (char)1);
  // symbolic Cholesky at tile level: every pair of filled tiles of column k fills their product's tile
  std::vector<int32_t> rows;
  for (int k = 0; k < nt; k++) {
    rows.clear();
    for (int I = k + 1; I < nt; I++)
      if (filled[(size_t)I * nt + k]) rows.push_back(I);
    for (size_t x = 0; x < rows.size(); x++)
      for (size_t y = 0; y <= x; y++) filled[(size_t)rows[x] * nt + rows[y]] = 1;
  }
  // storage: tile columns in order, rows ascending inside a column
  pl.tile_map.assign((size_t)nt * nt, -1);
  pl.col_diag.assign(nt, 0);
  pl.col_off.assign(nt + 1, 0);
  for (int J = 0; J < nt; J++) {
    for (int I = J; I < nt; I++) {
      if (!filled[(size_t)I * nt + J]) continue;
      const int t = (int)pl.tile_row.size();
      pl.tile_map[(size_t)I * nt + J] = t;
      pl.tile_row.push_back(I);
      pl.tile_col.push_back(J);
      if (I == J) {
        pl.col_diag[J] = t;
      } else {
        pl.col_tile.push_back(t);
        pl.col_row.push_back(I);
      }
    }
    pl.col_off[J + 1] = (int)pl.col_tile.size();
  }
  pl.n_filled = (int)pl.tile_row.size();
  // block -> edge-list table, per tile, the edges of a block ascending
  for (BlockRef& r : refs) r.tile = pl.tile_map[(size_t)(r.fa / kTilePoses) * nt + r.fb / kTilePoses];
  std::sort(refs.begin(), refs.end());
  pl.tile_blk_off.assign(pl.n_filled + 1, 0);
  for (size_t x = 0; x < refs.size(); x++) {
    const BlockRef& r = refs[x];
    if (x == 0 || refs[x - 1].tile != r.tile || refs[x - 1].fa != r.fa || refs[x - 1].fb != r.fb) {
      pl.blk_pos.push_back(((r.fa % kTilePoses) << 4) | (r.fb % kTilePoses));
      pl.blk_off.push_back((int)pl.blk_contrib.size());
      pl.tile_blk_off[r.tile + 1]++;
    }
    if (r.edge >= 0) pl.blk_contrib.push_back(4 * r.edge + r.kind);
  }
  pl.blk_off.push_back((int)pl.blk_contrib.size());
  for (int t = 0; t < pl.n_filled; t++) pl.tile_blk_off[t + 1] += pl.tile_blk_off[t];
  pl.pose_off.assign(nf + 1, 0);
  for (int f = 0; f < nf; f++) {
    pl.pose_contrib.insert(pl.pose_contrib.end(), per_pose[f].begin(), per_pose[f].end());
    pl.pose_off[f + 1] = (int)pl.pose_contrib.size();
  }
  return RSPL_OK;
}

struct Trial {
  double cost = 0, pred = 0, max_step = 0;
  bool bad_pivot = false;
};

void fill_plan_counts(const Plan& pl, rspl_pgo_result* r) {
  r->n_free = pl.n_free;
  r->n_tiles = pl.n_struct;
  r->n_filled_tiles = pl.n_filled;
}

// The LM rule of the contract over a backend S: linearise(&F, &max_diag), trial(lambda, &t), accept(), fetch(q, p).
template <class S>
int lm_solve(S& side, const Plan& pl, const rspl_pgo_params* params, rspl_pgo_result* res) {
  const int max_it = params && params->max_iterations > 0 ? params->max_iterations : 30;
  const double step_tol = params && params->step_tol > 0 ? params->step_tol : 1e-10;
  fill_plan_counts(pl, res);
  res->iterations = res->trials = 0;
  res->status = RSPL_PGO_CONVERGED;
  double F = 0, max_diag = 0;
  int rc = side.linearise(&F, &max_diag);
  if (rc) return rc;
  res->cost_initial = res->cost_final = F;
  res->lambda = 0;
  // nothing to optimise: no free pose, or free poses that no edge touches (H = 0, b = 0)
  if (pl.n_free == 0 || max_diag == 0) return side.fetch(res->pose_q, res->pose_p);
  double lambda = 1e-5 * max_diag, nu = 2;
  int rejections = 0, iterations = 0, trials = 0;
  bool factored = false;
  int status = RSPL_PGO_MAX_ITERATIONS;
  while (iterations < max_it) {
    Trial t;
    rc = side.trial(lambda, &t);
    if (rc) return rc;
    trials++;
    double rho = 0;
    bool ok = false;
    if (!t.bad_pivot) {
      factored = true;
      if (t.pred <= pgo::kResolvable * F) {  // the cost cannot resolve this step: rho's sign would be rounding
        status = RSPL_PGO_CONVERGED;
        break;
      }
      rho = (F - t.cost) / t.pred;
      ok = rho > 0 && std::isfinite(t.cost);
    }
    if (ok) {
      side.accept();
      F = t.cost;
      const double s = 2 * rho - 1;
      lambda *= std::max(1.0 / 3.0, 1 - s * s * s);
      nu = 2;
      rejections = 0;
      iterations++;
      if (t.max_step < step_tol) {
        status = RSPL_PGO_CONVERGED;
        break;
      }
      if (iterations == max_it) break;
      double f2, d2;
      rc = side.linearise(&f2, &d2);
      if (rc) return rc;
    } else {
      lambda *= nu;
      nu *= 2;
      if (++rejections == pgo::kMaxRejections) {
        status = RSPL_PGO_STALLED;
        break;
      }
    }
  }
  res->status = status;
  res->iterations = iterations;
  res->trials = trials;
  res->cost_final = F;
  res->lambda = lambda;
  if (!factored) {
    set_error("rspl_pgo: no factorisation succeeded in %d trials (lambda %g)", trials, lambda);
    return RSPL_E_SOLVER;
  }
  return side.fetch(res->pose_q, res->pose_p);
}

// ---- the host twin -------------------------------------------------------------------------------------------
struct HostSide {
  const rspl_pgo_problem& P;
  const Plan& pl;
  std::vector<double> q, p, tq, tp, eblk, eg, ecost, tiles, b, hdiag, y, delta;

  HostSide(const rspl_pgo_problem& P_, const Plan& pl_) : P(P_), pl(pl_) {
    const size_t n = pl.n_poses, E = pl.n_edges, V = (size_t)pl.nt * kTile;
    q.assign(P.pose_q, P.pose_q + 4 * n);
    p.assign(P.pose_p, P.pose_p + 3 * n);
    tq = q;
    tp = p;
    eblk.resize(108 * E);
    eg.resize(12 * E);
    ecost.resize(E);
    tiles.resize((size_t)pl.n_filled * kTileElems);
    b.assign(V, 0);
    hdiag.assign(V, 0);
    y.assign(V, 0);
    delta.assign(V, 0);
  }

  double total_cost() const {
    double s = 0;
    for (double c : ecost) s += c;
    return s;
  }

  int linearise(double* F, double* max_diag) {
    for (int e = 0; e < pl.n_edges; e++) {
      const int i = P.edge_i[e], j = P.edge_j[e];
      pgo::EdgeGeometry g;
      pgo::edge_residual(&q[4 * (size_t)i], &p[3 * (size_t)i], &q[4 * (size_t)j], &p[3 * (size_t)j],
                         P.edge_q + 4 * (size_t)e, P.edge_p + 3 * (size_t)e, g);
      double* blk = &eblk[108 * (size_t)e];
      pgo::edge_blocks(g, P.edge_w[2 * (size_t)e], P.edge_w[2 * (size_t)e + 1], blk, blk + 36, blk + 72,
                       &eg[12 * (size_t)e], &eg[12 * (size_t)e + 6]);
      ecost[e] = pgo::edge_cost(g.e, P.edge_w[2 * (size_t)e], P.edge_w[2 * (size_t)e + 1]);
    }
    double md = 0;
    for (int f = 0; f < pl.n_free; f++)
      for (int c = 0; c < kPoseDim; c++) {
        double g = 0, d = 0;
        for (int m = pl.pose_off[f]; m < pl.pose_off[f + 1]; m++) {
          const int packed = pl.pose_contrib[m], e = packed >> 1, side = packed & 1;
          g += eg[12 * (size_t)e + 6 * side + c];
          d += eblk[108 * (size_t)e + 72 * side + 7 * c];
        }
        b[(size_t)f * kPoseDim + c] = -g;
        hdiag[(size_t)f * kPoseDim + c] = d;
        md = std::max(md, d);
      }
    *F = total_cost();
    *max_diag = md;
    return RSPL_OK;
  }

  void assemble(double lambda) {
    for (int t = 0; t < pl.n_filled; t++) {
      double* tile = &tiles[(size_t)t * kTileElems];
      const int I = pl.tile_row[t], J = pl.tile_col[t], live = pl.n_free * kPoseDim - I * kTile;
      std::fill(tile, tile + kTileElems, 0.0);
      if (I == J)
        for (int r = std::max(live, 0); r < kTile; r++) tile[r * kTile + r] = 1.0;
      for (int bk = pl.tile_blk_off[t]; bk < pl.tile_blk_off[t + 1]; bk++) {
        const int lr = pl.blk_pos[bk] >> 4, lc = pl.blk_pos[bk] & 15;
        for (int ra = 0; ra < 6; ra++)
          for (int ca = 0; ca < 6; ca++) {
            double s = 0;
            for (int m = pl.blk_off[bk]; m < pl.blk_off[bk + 1]; m++)
              s += pgo::block_entry(eblk.data(), pl.blk_contrib[m], ra, ca);
            if (I == J && lr == lc && ra == ca) s += lambda;
            tile[(lr * kPoseDim + ra) * kTile + lc * kPoseDim + ca] = s;
          }
      }
    }
  }

  bool factor() {
    for (int k = 0; k < pl.nt; k++) {
      double* L = &tiles[(size_t)pl.col_diag[k] * kTileElems];
      for (int c = 0; c < kTile; c++) {
        const double d = L[c * kTile + c];
        if (!(d > 0.0)) return false;
        const double ld = std::sqrt(d);
        L[c * kTile + c] = ld;
        for (int r = c + 1; r < kTile; r++) L[r * kTile + c] /= ld;
        for (int r = c + 1; r < kTile; r++) {
          const double lrc = L[r * kTile + c];
          for (int c2 = c + 1; c2 <= r; c2++) L[r * kTile + c2] -= lrc * L[c2 * kTile + c];
        }
      }
      const int off = pl.col_off[k], n = pl.col_off[k + 1] - off;
      for (int s = 0; s < n; s++) {
        double* X = &tiles[(size_t)pl.col_tile[off + s] * kTileElems];
        for (int r = 0; r < kTile; r++)
          for (int c = 0; c < kTile; c++) {
            const double xc = X[r * kTile + c] / L[c * kTile + c];
            X[r * kTile + c] = xc;
            for (int c2 = c + 1; c2 < kTile; c2++) X[r * kTile + c2] -= xc * L[c2 * kTile + c];
          }
      }
      for (int x = 0; x < n; x++)
        for (int yy = 0; yy <= x; yy++) {
          const double* A = &tiles[(size_t)pl.col_tile[off + x] * kTileElems];
          const double* B = &tiles[(size_t)pl.col_tile[off + yy] * kTileElems];
          double* C = &tiles[(size_t)pl.tile_map[(size_t)pl.col_row[off + x] * pl.nt + pl.col_row[off + yy]] * kTileElems];
          for (int r = 0; r < kTile; r++)
            for (int c = 0; c < kTile; c++) {
              double s = 0;
              for (int m = 0; m < kTile; m++) s += A[r * kTile + m] * B[c * kTile + m];
              C[r * kTile + c] -= s;
            }
        }
    }
    return true;
  }

  void substitute() {
    y = b;
    for (int k = 0; k < pl.nt; k++) {
      const double* L = &tiles[(size_t)pl.col_diag[k] * kTileElems];
      double* yk = &y[(size_t)k * kTile];
      for (int c = 0; c < kTile; c++) {
        yk[c] /= L[c * kTile + c];
        for (int r = c + 1; r < kTile; r++) yk[r] -= L[r * kTile + c] * yk[c];
      }
      for (int s = pl.col_off[k]; s < pl.col_off[k + 1]; s++) {
        const double* A = &tiles[(size_t)pl.col_tile[s] * kTileElems];
        double* yi = &y[(size_t)pl.col_row[s] * kTile];
        for (int r = 0; r < kTile; r++) {
          double acc = 0;
          for (int c = 0; c < kTile; c++) acc += A[r * kTile + c] * yk[c];
          yi[r] -= acc;
        }
      }
    }
    for (int k = pl.nt - 1; k >= 0; k--) {
      const double* L = &tiles[(size_t)pl.col_diag[k] * kTileElems];
      double* xk = &delta[(size_t)k * kTile];
      for (int c = 0; c < kTile; c++) {
        double acc = 0;
        for (int s = pl.col_off[k]; s < pl.col_off[k + 1]; s++) {
          const double* A = &tiles[(size_t)pl.col_tile[s] * kTileElems];
          const double* xi = &delta[(size_t)pl.col_row[s] * kTile];
          for (int r = 0; r < kTile; r++) acc += A[r * kTile + c] * xi[r];
        }
        xk[c] = y[(size_t)k * kTile + c] - acc;
      }
      for (int c = kTile - 1; c >= 0; c--) {
        xk[c] /= L[c * kTile + c];
        for (int r = 0; r < c; r++) xk[r] -= L[c * kTile + r] * xk[c];
      }
    }
  }

  void trial_pose(int i, double* qo, double* po) const {
    const int f = pl.pose_free[i];
    if (f >= 0) {
      pgo::pose_update(&q[4 * (size_t)i], &p[3 * (size_t)i], &delta[(size_t)f * kPoseDim], qo, po);
    } else {
      std::memcpy(qo, &q[4 * (size_t)i], sizeof(double) * 4);
      std::memcpy(po, &p[3 * (size_t)i], sizeof(double) * 3);
    }
  }

  int trial(double lambda, Trial* t) {
    assemble(lambda);
    if (!factor()) {
      t->bad_pivot = true;
      return RSPL_OK;
    }
    substitute();
    for (int i = 0; i < pl.n_poses; i++) trial_pose(i, &tq[4 * (size_t)i], &tp[3 * (size_t)i]);
    for (int e = 0; e < pl.n_edges; e++) {
      const int i = P.edge_i[e], j = P.edge_j[e];
      pgo::EdgeGeometry g;
      pgo::edge_residual(&tq[4 * (size_t)i], &tp[3 * (size_t)i], &tq[4 * (size_t)j], &tp[3 * (size_t)j],
                         P.edge_q + 4 * (size_t)e, P.edge_p + 3 * (size_t)e, g);
      ecost[e] = pgo::edge_cost(g.e, P.edge_w[2 * (size_t)e], P.edge_w[2 * (size_t)e + 1]);
    }
    t->cost = total_cost();
    double pred = 0, ms = 0;
    for (int k = 0; k < pl.n_free * kPoseDim; k++) {
      pred += delta[k] * (lambda * delta[k] + b[k]);
      ms = std::max(ms, std::fabs(delta[k]));
    }
    t->pred = pred;
    t->max_step = ms;
    return RSPL_OK;
  }

  void accept() {
    q.swap(tq);
    p.swap(tp);
  }

  int fetch(double* qo, double* po) {
    if (qo) std::memcpy(qo, q.data(), sizeof(double) * q.size());
    if (po) std::memcpy(po, p.data(), sizeof(double) * p.size());
    return RSPL_OK;
  }
};

}  // namespace

// ---- the handle ----------------------------------------------------------------------------------------------
struct rspl_pgo {
  rspl_pgo_config cfg{};
  int NT = 0;
  Arena arena;
  PinnedArena pinned;
  hipStream_t stream = nullptr;
  pgo::DArgs a{};
  pgo::Scalars* out = nullptr;
};

namespace {

template <class A, class P>
void carve(rspl_pgo* h, A& ar, P& pin) {
  const size_t N = h->cfg.max_poses, E = h->cfg.max_edges, TL = h->cfg.max_tiles, NT = h->NT, V = NT * kTile;
  pgo::DArgs& a = h->a;
  h->out = pin.template take<pgo::Scalars>(1, &a.out);
  a.q = ar.template take<double>(4 * N);
  a.p = ar.template take<double>(3 * N);
  a.tq = ar.template take<double>(4 * N);
  a.tp = ar.template take<double>(3 * N);
  a.pose_free = ar.template take<int32_t>(N);
  a.edge_i = ar.template take<int32_t>(E);
  a.edge_j = ar.template take<int32_t>(E);
  a.edge_q = ar.template take<double>(4 * E);
  a.edge_p = ar.template take<double>(3 * E);
  a.edge_w = ar.template take<double>(2 * E);
  a.eblk = ar.template take<double>(108 * E);
  a.eg = ar.template take<double>(12 * E);
  a.ecost = ar.template take<double>(E);
  a.eres = ar.template take<double>(6 * E);
  a.tiles = ar.template take<double>(TL * kTileElems);
  a.b = ar.template take<double>(V);
  a.hdiag = ar.template take<double>(V);
  a.y = ar.template take<double>(V);
  a.delta = ar.template take<double>(V);
  a.tile_row = ar.template take<int32_t>(TL);
  a.tile_col = ar.template take<int32_t>(TL);
  a.tile_map = ar.template take<int32_t>(NT * NT);
  a.tile_blk_off = ar.template take<int32_t>(TL + 1);
  a.blk_pos = ar.template take<int32_t>(N + E);
  a.blk_off = ar.template take<int32_t>(N + E + 1);
  a.blk_contrib = ar.template take<int32_t>(3 * E);
  a.pose_off = ar.template take<int32_t>(N + 1);
  a.pose_contrib = ar.template take<int32_t>(2 * E);
  a.col_diag = ar.template take<int32_t>(NT);
  a.col_off = ar.template take<int32_t>(NT + 1);
  a.col_tile = ar.template take<int32_t>(TL);
  a.col_row = ar.template take<int32_t>(TL);
  a.flag = ar.template take<int32_t>(1);
}

template <class T>
hipError_t upload(const T* dst, const T* src, size_t count, hipStream_t s) {
  if (count == 0) return hipSuccess;
  return hipMemcpyAsync(const_cast<T*>(dst), src, sizeof(T) * count, hipMemcpyHostToDevice, s);
}
template <class T>
hipError_t upload(const T* dst, const std::vector<T>& v, hipStream_t s) {
  return upload(dst, v.data(), v.size(), s);
}

struct DeviceSide {
  rspl_pgo* h;
  const rspl_pgo_problem& P;
  const Plan& pl;
  DeviceSide(rspl_pgo* h_, const rspl_pgo_problem& P_, const Plan& pl_) : h(h_), P(P_), pl(pl_) {}

  // the problem and the plan's tables; the host arrays are done with when this returns
  int setup() {
    pgo::DArgs& a = h->a;
    hipStream_t s = h->stream;
    const size_t n = pl.n_poses, E = pl.n_edges;
    a.n_poses = pl.n_poses;
    a.n_edges = pl.n_edges;
    a.n_free = pl.n_free;
    a.nt = pl.nt;
    RSPL_HIP(hipSetDevice(h->cfg.device));
    RSPL_HIP(upload(a.q, P.pose_q, 4 * n, s));
    RSPL_HIP(upload(a.p, P.pose_p, 3 * n, s));
    RSPL_HIP(upload(a.tq, P.pose_q, 4 * n, s));
    RSPL_HIP(upload(a.tp, P.pose_p, 3 * n, s));
    RSPL_HIP(upload(a.pose_free, pl.pose_free, s));
    RSPL_HIP(upload(a.edge_i, P.edge_i, E, s));
    RSPL_HIP(upload(a.edge_j, P.edge_j, E, s));
    RSPL_HIP(upload(a.edge_q, P.edge_q, 4 * E, s));
    RSPL_HIP(upload(a.edge_p, P.edge_p, 3 * E, s));
    RSPL_HIP(upload(a.edge_w, P.edge_w, 2 * E, s));
    RSPL_HIP(upload(a.tile_row, pl.tile_row, s));
    RSPL_HIP(upload(a.tile_col, pl.tile_col, s));
    RSPL_HIP(upload(a.tile_map, pl.tile_map, s));
    RSPL_HIP(upload(a.tile_blk_off, pl.tile_blk_off, s));
    RSPL_HIP(upload(a.blk_pos, pl.blk_pos, s));
    RSPL_HIP(upload(a.blk_off, pl.blk_off, s));
    RSPL_HIP(upload(a.blk_contrib, pl.blk_contrib, s));
    RSPL_HIP(upload(a.pose_off, pl.pose_off, s));
    RSPL_HIP(upload(a.pose_contrib, pl.pose_contrib, s));
    RSPL_HIP(upload(a.col_diag, pl.col_diag, s));
    RSPL_HIP(upload(a.col_off, pl.col_off, s));
    RSPL_HIP(upload(a.col_tile, pl.col_tile, s));
    RSPL_HIP(upload(a.col_row, pl.col_row, s));
    RSPL_HIP(hipMemsetAsync(a.flag, 0, sizeof(int32_t), s));
    RSPL_HIP(hipStreamSynchronize(s));
    return RSPL_OK;
  }

  int linearise(double* F, double* max_diag) {
    RSPL_HIP(pgo::launch_linearise(h->a, h->stream));
    RSPL_HIP(hipStreamSynchronize(h->stream));
    *F = h->out->cost;
    *max_diag = h->out->max_diag;
    return RSPL_OK;
  }

  int enqueue_solve(double lambda) {
    RSPL_HIP(pgo::launch_assemble(h->a, pl.n_filled, lambda, h->stream));
    RSPL_HIP(pgo::launch_factor(h->a, pl.col_off.data(), h->stream));
    RSPL_HIP(pgo::launch_substitute(h->a, h->stream));
    return RSPL_OK;
  }

  int trial(double lambda, Trial* t) {
    const int rc = enqueue_solve(lambda);
    if (rc) return rc;
    RSPL_HIP(pgo::launch_trial(h->a, lambda, h->stream));
    RSPL_HIP(hipStreamSynchronize(h->stream));
    t->bad_pivot = h->out->bad_pivot != 0;
    t->cost = h->out->cost;
    t->pred = h->out->pred;
    t->max_step = h->out->max_step;
    return RSPL_OK;
  }

  void accept() {
    std::swap(h->a.q, h->a.tq);
    std::swap(h->a.p, h->a.tp);
  }

  int fetch(double* qo, double* po) {
    const size_t n = pl.n_poses;
    if (qo) RSPL_HIP(hipMemcpyAsync(qo, h->a.q, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, h->stream));
    if (po) RSPL_HIP(hipMemcpyAsync(po, h->a.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream));
    RSPL_HIP(hipStreamSynchronize(h->stream));
    return RSPL_OK;
  }
};

int check_capacity(const rspl_pgo* h, const Plan& pl) {
  if (pl.n_poses > h->cfg.max_poses || pl.n_edges > h->cfg.max_edges || pl.n_filled > h->cfg.max_tiles) {
    set_error("rspl_pgo: %d poses, %d edges, %d filled tiles exceed the handle's %d, %d, %d", pl.n_poses, pl.n_edges,
              pl.n_filled, h->cfg.max_poses, h->cfg.max_edges, h->cfg.max_tiles);
    return RSPL_E_CAPACITY;
  }
  return RSPL_OK;
}

}  // namespace

extern "C" int rspl_pgo_create(const rspl_pgo_config* cfg, rspl_pgo** out) {
  RSPL_CHECK_ARG(cfg && out, "rspl_pgo_create: NULL argument");
  RSPL_CHECK_ARG(cfg->max_poses >= 1 && cfg->max_poses <= pgo::kMaxPoses, "rspl_pgo_create: max_poses %d outside 1..%d",
                 cfg->max_poses, pgo::kMaxPoses);
  RSPL_CHECK_ARG(cfg->max_edges >= 0 && cfg->max_tiles >= 1 && cfg->device >= 0,
                 "rspl_pgo_create: max_edges %d, max_tiles %d, device %d", cfg->max_edges, cfg->max_tiles, cfg->device);
  const int NT = (cfg->max_poses + kTilePoses - 1) / kTilePoses;
  rspl_pgo* h = new rspl_pgo;
  h->cfg = *cfg;
  h->cfg.max_tiles = std::min(cfg->max_tiles, NT * (NT + 1) / 2);  // more than max_poses can fill is never used
  h->NT = NT;
  Sizer sz, psz;
  carve(h, sz, psz);
  int rc = RSPL_OK;
  if (hipSetDevice(cfg->device) != hipSuccess) {
    set_error("rspl_pgo_create: hipSetDevice(%d) failed", cfg->device);
    rc = RSPL_E_DEVICE;
  }
  if (!rc) rc = h->arena.reserve(sz.used + 256);
  if (!rc) rc = h->pinned.reserve(psz.used + 256);
  if (!rc && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    set_error("rspl_pgo_create: hipStreamCreate failed");
    rc = RSPL_E_DEVICE;
  }
  if (rc) {
    rspl_pgo_destroy(h);
    return rc;
  }
  carve(h, h->arena, h->pinned);
  *out = h;
  return RSPL_OK;
}

extern "C" void rspl_pgo_destroy(rspl_pgo* h) {
  if (!h) return;
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  h->arena.release();
  h->pinned.release();
  delete h;
}

extern "C" int rspl_pgo_solve(rspl_pgo* h, const rspl_pgo_problem* problem, const rspl_pgo_params* params,
                              rspl_pgo_result* result) {
  RSPL_CHECK_ARG(h && result, "rspl_pgo_solve: NULL argument");
  int rc = check_problem(problem);
  if (rc) return rc;
  Plan pl;
  rc = make_plan(*problem, pl);
  if (rc) return rc;
  fill_plan_counts(pl, result);
  rc = check_capacity(h, pl);
  if (rc) return rc;
  DeviceSide side(h, *problem, pl);
  rc = side.setup();
  if (rc) return rc;
  return lm_solve(side, pl, params, result);
}

extern "C" int rspl_pgo_debug_host(const rspl_pgo_problem* problem, const rspl_pgo_params* params,
                                   rspl_pgo_result* result) {
  RSPL_CHECK_ARG(result, "rspl_pgo_debug_host: NULL argument");
  int rc = check_problem(problem);
  if (rc) return rc;
  Plan pl;
  rc = make_plan(*problem, pl);
  if (rc) return rc;
  HostSide side(*problem, pl);
  return lm_solve(side, pl, params, result);
}

extern "C" int rspl_pgo_debug_plan(const rspl_pgo_problem* problem, int* n_free, int* tiles_per_side, int* n_tiles,
                                   int* n_filled_tiles, int32_t* tile_map, int map_cap) {
  int rc = check_problem(problem);
  if (rc) return rc;
  Plan pl;
  rc = make_plan(*problem, pl);
  if (rc) return rc;
  if (n_free) *n_free = pl.n_free;
  if (tiles_per_side) *tiles_per_side = pl.nt;
  if (n_tiles) *n_tiles = pl.n_struct;
  if (n_filled_tiles) *n_filled_tiles = pl.n_filled;
  if (tile_map) {
    if ((size_t)map_cap < pl.tile_map.size()) {
      set_error("rspl_pgo_debug_plan: the tile map needs %zu entries, %d given", pl.tile_map.size(), map_cap);
      return RSPL_E_CAPACITY;
    }
    std::copy(pl.tile_map.begin(), pl.tile_map.end(), tile_map);
  }
  return RSPL_OK;
}

extern "C" int rspl_pgo_debug_system(rspl_pgo* h, const rspl_pgo_problem* problem, double lambda, double* e, double* b,
                                     double* H_dense, double* delta) {
  RSPL_CHECK_ARG(h, "rspl_pgo_debug_system: NULL handle");
  RSPL_CHECK_ARG(std::isfinite(lambda) && lambda >= 0, "rspl_pgo_debug_system: lambda %g", lambda);
  int rc = check_problem(problem);
  if (rc) return rc;
  Plan pl;
  rc = make_plan(*problem, pl);
  if (rc) return rc;
  rc = check_capacity(h, pl);
  if (rc) return rc;
  const size_t n = (size_t)pl.n_free * kPoseDim;
  RSPL_CHECK_ARG(!H_dense || n <= 1536, "rspl_pgo_debug_system: no dense H above 1536 unknowns (%zu)", n);
  DeviceSide side(h, *problem, pl);
  rc = side.setup();
  if (rc) return rc;
  double F, md;
  rc = side.linearise(&F, &md);
  if (rc) return rc;
  hipStream_t s = h->stream;
  if (e && pl.n_edges)
    RSPL_HIP(hipMemcpyAsync(e, h->a.eres, sizeof(double) * 6 * pl.n_edges, hipMemcpyDeviceToHost, s));
  if (b && n) RSPL_HIP(hipMemcpyAsync(b, h->a.b, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  RSPL_HIP(hipStreamSynchronize(s));
  if (n == 0) return RSPL_OK;
  if (H_dense) {
    std::vector<double> tiles((size_t)pl.n_filled * kTileElems);
    RSPL_HIP(pgo::launch_assemble(h->a, pl.n_filled, 0.0, s));
    RSPL_HIP(hipMemcpyAsync(tiles.data(), h->a.tiles, sizeof(double) * tiles.size(), hipMemcpyDeviceToHost, s));
    RSPL_HIP(hipStreamSynchronize(s));
    std::fill(H_dense, H_dense + n * n, 0.0);
    for (int t = 0; t < pl.n_filled; t++) {
      const size_t I = pl.tile_row[t], J = pl.tile_col[t];
      const double* tile = &tiles[(size_t)t * kTileElems];
      for (size_t r = 0; r < (size_t)kTile; r++)
        for (size_t c = 0; c < (size_t)kTile; c++) {
          const size_t R = I * kTile + r, Cc = J * kTile + c;
          if (R >= n || Cc >= n || Cc > R) continue;
          // a diagonal tile stores its lower triangle and the whole of each diagonal 6 x 6 block
          H_dense[R * n + Cc] = tile[r * kTile + c];
          H_dense[Cc * n + R] = tile[r * kTile + c];
        }
    }
  }
  if (delta) {
    rc = side.enqueue_solve(lambda);
    if (rc) return rc;
    int32_t bad = 0;
    RSPL_HIP(hipMemcpyAsync(&bad, h->a.flag, sizeof(bad), hipMemcpyDeviceToHost, s));
    RSPL_HIP(hipMemcpyAsync(delta, h->a.delta, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    RSPL_HIP(hipStreamSynchronize(s));
    if (bad) {
      set_error("rspl_pgo_debug_system: non-positive pivot at lambda %g", lambda);
      return RSPL_E_SOLVER;
    }
  }
  return RSPL_OK;
}
