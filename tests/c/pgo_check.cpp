// Host check of the loop-closure stage (test infrastructure): rspl_pgo_debug_host -- csrc/pgo.cpp's host twin of the
// pose-graph solver -- rspl_pgo_debug_plan, the refusals of the contract, and the three map calls
// (rspl_map_pose_graph, rspl_map_apply_pose_graph, rspl_map_loop_candidates) from C++.  It first prints sizeof /
// offsetof of the four new structs (tests/test_pgo_cpu.py compares them with the ctypes mirrors).  No device call is
// made: it runs on the CPU.  Exits non-zero on a difference.  `make -f pgo_check.mk pgo_check_san` builds it with
// the sources under ASan + UBSan (host code).
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rspl.h"

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("pgo_check: line %d: %s\n", __LINE__, #cond);  \
      failures++;                                                \
    }                                                            \
  } while (0)
#define LAYOUT(S, f) std::printf("offsetof %s.%s %zu\n", #S, #f, offsetof(S, f))

static void layouts() {
  std::printf("sizeof rspl_pgo_config %zu\n", sizeof(rspl_pgo_config));
  LAYOUT(rspl_pgo_config, max_poses); LAYOUT(rspl_pgo_config, max_edges); LAYOUT(rspl_pgo_config, max_tiles);
  LAYOUT(rspl_pgo_config, device);
  std::printf("sizeof rspl_pgo_problem %zu\n", sizeof(rspl_pgo_problem));
  LAYOUT(rspl_pgo_problem, n_poses); LAYOUT(rspl_pgo_problem, pose_q); LAYOUT(rspl_pgo_problem, pose_p);
  LAYOUT(rspl_pgo_problem, pose_fixed); LAYOUT(rspl_pgo_problem, n_edges); LAYOUT(rspl_pgo_problem, edge_i);
  LAYOUT(rspl_pgo_problem, edge_j); LAYOUT(rspl_pgo_problem, edge_q); LAYOUT(rspl_pgo_problem, edge_p);
  LAYOUT(rspl_pgo_problem, edge_w);
  std::printf("sizeof rspl_pgo_params %zu\n", sizeof(rspl_pgo_params));
  LAYOUT(rspl_pgo_params, max_iterations); LAYOUT(rspl_pgo_params, step_tol);
  std::printf("sizeof rspl_pgo_result %zu\n", sizeof(rspl_pgo_result));
  LAYOUT(rspl_pgo_result, pose_q); LAYOUT(rspl_pgo_result, pose_p); LAYOUT(rspl_pgo_result, status);
  LAYOUT(rspl_pgo_result, iterations); LAYOUT(rspl_pgo_result, trials); LAYOUT(rspl_pgo_result, n_free);
  LAYOUT(rspl_pgo_result, n_tiles); LAYOUT(rspl_pgo_result, n_filled_tiles); LAYOUT(rspl_pgo_result, cost_initial);
  LAYOUT(rspl_pgo_result, cost_final); LAYOUT(rspl_pgo_result, lambda);
}

struct Graph {
  std::vector<double> q, p, tq, tp, eq, ep, ew;
  std::vector<uint8_t> fixed;
  std::vector<int32_t> ei, ej;
  rspl_pgo_problem problem() const {
    return rspl_pgo_problem{(int)fixed.size(), q.data(), p.data(), fixed.data(), (int)ei.size(), ei.data(), ej.data(),
                            eq.data(), ep.data(), ew.data()};
  }
};

// poses on a circle turning about z (yaw only: Z is easy to write down), chain edges to the next two poses, the
// measurements exact, the initial positions off by a drift
static Graph ring(int n) {
  Graph g;
  const double kPi = 3.14159265358979323846;
  for (int i = 0; i < n; i++) {
    const double a = 2 * kPi * i / n;
    g.tq.insert(g.tq.end(), {0.0, 0.0, std::sin(0.5 * a), std::cos(0.5 * a)});
    g.tp.insert(g.tp.end(), {5 * std::cos(a), 5 * std::sin(a), 0.1 * i});
    g.fixed.push_back(i == 0);
  }
  g.q = g.tq;
  g.p = g.tp;
  for (int i = 1; i < n; i++) {
    g.p[3 * i] += 0.01 * i;
    g.p[3 * i + 1] -= 0.005 * i;
  }
  for (int i = 0; i < n; i++)
    for (int k = 1; k <= 2 && i + k < n; k++) {
      const int j = i + k;
      const double ai = 2 * kPi * i / n, aj = 2 * kPi * j / n, da = aj - ai;
      const double dx = g.tp[3 * j] - g.tp[3 * i], dy = g.tp[3 * j + 1] - g.tp[3 * i + 1], dz = g.tp[3 * j + 2] - g.tp[3 * i + 2];
      g.ei.push_back(i);
      g.ej.push_back(j);
      g.eq.insert(g.eq.end(), {0.0, 0.0, std::sin(0.5 * da), std::cos(0.5 * da)});
      g.ep.insert(g.ep.end(), {std::cos(ai) * dx + std::sin(ai) * dy, -std::sin(ai) * dx + std::cos(ai) * dy, dz});
      g.ew.insert(g.ew.end(), {1.0, 1.0});
    }
  return g;
}

static void solver() {
  Graph g = ring(40);
  rspl_pgo_problem P = g.problem();
  std::vector<double> q(4 * 40), p(3 * 40);
  rspl_pgo_result R{};
  R.pose_q = q.data();
  R.pose_p = p.data();
  CHECK(rspl_pgo_debug_host(&P, nullptr, &R) == RSPL_OK);
  CHECK(R.status == RSPL_PGO_CONVERGED && R.iterations > 0 && R.iterations <= 30 && R.trials >= R.iterations);
  CHECK(R.n_free == 39 && R.n_tiles == 5 && R.n_filled_tiles == 5);
  CHECK(R.cost_initial > 1e-3 && R.cost_final < 1e-20);
  double worst = 0;
  for (size_t k = 0; k < p.size(); k++) worst = std::fmax(worst, std::fabs(p[k] - g.tp[k]));
  for (size_t k = 0; k < q.size(); k++) worst = std::fmax(worst, std::fabs(q[k] - g.tq[k]));
  CHECK(worst < 1e-9);
  int nf = 0, nt = 0, ns = 0, nfl = 0;
  std::vector<int32_t> tm(9);
  CHECK(rspl_pgo_debug_plan(&P, &nf, &nt, &ns, &nfl, tm.data(), 9) == RSPL_OK);
  CHECK(nf == 39 && nt == 3 && ns == 5 && nfl == 5 && tm[0] == 0 && tm[3] == 1 && tm[4] == 2 && tm[6] == -1 && tm[1] == -1);
  CHECK(rspl_pgo_debug_plan(&P, nullptr, nullptr, nullptr, nullptr, tm.data(), 8) == RSPL_E_CAPACITY);
  rspl_pgo_params one{1, 0.0};
  CHECK(rspl_pgo_debug_host(&P, &one, &R) == RSPL_OK && R.status == RSPL_PGO_MAX_ITERATIONS && R.iterations == 1);

  // the refusals
  Graph b = g;
  b.fixed[0] = 0;
  P = b.problem();
  CHECK(rspl_pgo_debug_host(&P, nullptr, &R) == RSPL_E_ARG);  // no fixed pose
  b = g;
  b.ej[3] = b.ei[3];
  P = b.problem();
  CHECK(rspl_pgo_debug_host(&P, nullptr, &R) == RSPL_E_ARG);  // i == j
  b = g;
  b.ej[3] = 40;
  P = b.problem();
  CHECK(rspl_pgo_debug_host(&P, nullptr, &R) == RSPL_E_ARG);  // out of range
  b = g;  // cut the ring in two: poses 20.. lose their fixed pose
  for (size_t e = 0; e < b.ei.size(); e++)
    if (b.ei[e] < 20 && b.ej[e] >= 20) b.ei[e] = b.ej[e] - 20 > 0 ? b.ej[e] - 20 - 1 : 0, b.ej[e] = 19;
  for (size_t e = 0; e < b.ei.size(); e++)
    if (b.ei[e] == b.ej[e]) b.ei[e] = 0;
  P = b.problem();
  CHECK(rspl_pgo_debug_host(&P, nullptr, &R) == RSPL_E_ARG);  // a floating component
  CHECK(rspl_pgo_debug_host(nullptr, nullptr, &R) == RSPL_E_ARG);
  // allowed: every pose fixed
  b = g;
  std::fill(b.fixed.begin(), b.fixed.end(), (uint8_t)1);
  P = b.problem();
  CHECK(rspl_pgo_debug_host(&P, nullptr, &R) == RSPL_OK && R.status == RSPL_PGO_CONVERGED && R.iterations == 0 &&
        R.trials == 0 && R.n_free == 0 && R.cost_final == R.cost_initial && R.cost_initial > 1e-3);
  CHECK(std::memcmp(p.data(), b.p.data(), sizeof(double) * p.size()) == 0);
}

static void map_calls() {
  const double cam[5] = {400, 400, 320, 240, 40};
  rspl_map_config cfg{};
  cfg.camera = cam;
  rspl_map* m = nullptr;
  CHECK(rspl_map_create(&cfg, &m) == RSPL_OK);
  const double kps[6] = {10, 10, -1, 20, 20, -1};
  for (int f = 0; f < 4; f++) {
    double T[16] = {1, 0, 0, 1.0 * f, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    rspl_map_keyframe k{};
    k.frame_id = 10 * f;
    k.Twc = T;
    k.n_keypoints = 2;
    k.keypoints = kps;
    k.parent_id = f == 0 ? -1 : 10 * (f - 1);
    CHECK(rspl_map_add_keyframe(m, &k) == RSPL_OK);
  }
  const double X[3] = {0.5, 1, 4}, Y[3] = {3.5, 1, 4};
  CHECK(rspl_map_add_mappoint(m, 7, X, RSPL_MAP_GOOD) == RSPL_OK && rspl_map_add_mappoint(m, 8, Y, RSPL_MAP_GOOD) == RSPL_OK);
  CHECK(rspl_map_add_point_observation(m, 7, 0, 0) == RSPL_OK && rspl_map_add_point_observation(m, 7, 10, 0) == RSPL_OK);
  CHECK(rspl_map_add_point_observation(m, 7, 30, 0) == RSPL_OK && rspl_map_add_point_observation(m, 8, 30, 1) == RSPL_OK);
  int nn = 0, ne = 0;
  CHECK(rspl_map_pose_graph(m, 1 << 30, nullptr, nullptr, nullptr, 0, &nn, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                            &ne) == RSPL_E_CAPACITY && nn == 4 && ne == 3);
  int32_t ids[4], ei[3], ej[3], ew[3];
  double q[16], p[12], eq[12], ep[9];
  CHECK(rspl_map_pose_graph(m, 1 << 30, ids, q, p, 4, &nn, ei, ej, eq, ep, ew, 3, &ne) == RSPL_OK);
  CHECK(ids[0] == 0 && ids[3] == 30 && ei[0] == 0 && ej[0] == 1 && ei[2] == 2 && ej[2] == 3 && ew[1] == 0);
  CHECK(q[3] == 1.0 && p[9] == 3.0 && eq[3] == 1.0 && ep[0] == 1.0 && ep[1] == 0.0);
  // frames 10 and 30 move by (0, 2, 0) and (0, 0, 5): point 7's anchor is frame 10 (frame 0 is not listed), 8's is 30
  const int32_t moved[2] = {10, 30};
  const double nq[8] = {0, 0, 0, 1, 0, 0, 0, 1}, np[6] = {1, 2, 0, 3, 0, 5};
  CHECK(rspl_map_apply_pose_graph(m, 2, moved, nq, np) == RSPL_OK);
  double T[16], x[3];
  int type = 0, nobs = 0;
  CHECK(rspl_map_get_keyframe(m, 10, T, nullptr) == RSPL_OK && T[3] == 1.0 && T[7] == 2.0);
  CHECK(rspl_map_get_mappoint(m, 7, x, &type, &nobs, nullptr, nullptr, 0) == RSPL_OK && x[0] == 0.5 && x[1] == 3.0 && x[2] == 4.0);
  CHECK(rspl_map_get_mappoint(m, 8, x, &type, &nobs, nullptr, nullptr, 0) == RSPL_OK && x[1] == 1.0 && x[2] == 9.0);
  const int32_t unknown[1] = {11};
  CHECK(rspl_map_apply_pose_graph(m, 1, unknown, nq, np) == RSPL_E_ARG);
  // the vote of frame 30 on points 7, 8, bad and unknown ids: frames 0 and 10 get one vote each; a gap of 20 drops 10
  const int32_t pts[4] = {7, 8, -1, 99};
  int32_t cid[4], cv[4];
  int nc = 0;
  CHECK(rspl_map_loop_candidates(m, 30, 4, pts, 0, cid, cv, 4, &nc) == RSPL_OK && nc == 2 && cid[0] == 0 && cid[1] == 10 &&
        cv[0] == 1 && cv[1] == 1);
  CHECK(rspl_map_loop_candidates(m, 30, 4, pts, 20, cid, cv, 4, &nc) == RSPL_OK && nc == 1 && cid[0] == 0);
  CHECK(rspl_map_loop_candidates(m, 30, 4, pts, 0, cid, cv, 1, &nc) == RSPL_E_CAPACITY && nc == 2);
  CHECK(rspl_map_loop_candidates(m, 31, 4, pts, 0, cid, cv, 4, &nc) == RSPL_E_ARG);
  rspl_map_destroy(m);
}

int main() {
  layouts();
  solver();
  map_calls();
  if (failures) return 1;
  std::printf("pgo_check: ok\n");
  return 0;
}
