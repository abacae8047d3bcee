// Host check of the global descriptor search (test infrastructure): rspl_lmap_debug_global_host -- csrc/lmap_reloc.cpp's
// host walk of the relocalisation contract -- and the host-side refusals of rspl_lmap_global_enqueue, on descriptors made
// of a few unit entries so every distance is exact.  No device call is made: it runs on the CPU.  Exits non-zero on the
// first difference.  `make -f reloc_check.mk reloc_check_san` builds it with the sources under ASan + UBSan (host code).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rspl.h"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("reloc_check: line %d: %s\n", __LINE__, #cond);  \
      failures++;                                                  \
    }                                                              \
  } while (0)

static void unit(double* d, int e) {
  std::memset(d, 0, sizeof(double) * 256);
  d[e] = 1.0;
}

int main() {
  // bank rows 0..4: e0, e1, e1 again (identical bits), e2, e3; keypoints: e1, e0, e0 again, e7 (matches nothing)
  const int nl = 5, n1 = 4;
  std::vector<double> desc(nl * 256), F(n1 * 259, 0.0), pos(3 * nl);
  const int be[nl] = {0, 1, 1, 2, 3}, ke[n1] = {1, 0, 0, 7};
  for (int p = 0; p < nl; p++) unit(&desc[256 * p], be[p]);
  for (int i = 0; i < n1; i++) {
    unit(&F[259 * i + 3], ke[i]);
    F[259 * i + 1] = 10.0 + i;
    F[259 * i + 2] = 20.0 + i;
  }
  for (int k = 0; k < 3 * nl; k++) pos[k] = 0.5 * k;
  const int32_t ids[nl] = {40, 41, 42, 43, 44};
  rspl_lmap_global_host_problem P{n1, F.data(), nl, ids, pos.data(), desc.data()};
  rspl_lmap_global_params gp{0.35, 0.6, 1};
  std::vector<int32_t> arg(n1), match(n1), kbest(nl), mkp(n1), mloc(n1), mid(n1);
  std::vector<double> best(n1), second(n1), mpos(3 * n1), mxy(2 * n1);
  rspl_lmap_global_result R{};
  R.arg = arg.data(); R.best = best.data(); R.second = second.data(); R.match = match.data(); R.kbest = kbest.data();
  R.match_kp = mkp.data(); R.match_local = mloc.data(); R.match_id = mid.data(); R.match_pos = mpos.data();
  R.match_xy = mxy.data();
  CHECK(rspl_lmap_debug_global_host(&P, &gp, &R) == RSPL_OK);
  CHECK(R.n_keypoints == 4 && R.n_local == 5);
  // keypoint 0 (e1): rows 1 and 2 tie at 0 -> arg 1, second == best, the ratio test fails
  CHECK(arg[0] == 1 && best[0] == 0.0 && second[0] == 0.0 && match[0] == -1);
  // keypoints 1 and 2 (e0, identical): both nearest to row 0; kbest[0] is the lower, only it is mutual
  CHECK(arg[1] == 0 && arg[2] == 0 && best[1] == 0.0 && second[1] == 2.0 && kbest[0] == 1);
  CHECK(match[1] == 0 && match[2] == -1);
  // keypoint 3 (e7): every distance is 2.0: arg the lowest row, nothing passes
  CHECK(arg[3] == 0 && best[3] == 2.0 && second[3] == 2.0 && match[3] == -1);
  CHECK(R.n_pass == 2 && R.n_matched == 1 && mkp[0] == 1 && mloc[0] == 0 && mid[0] == 40);
  CHECK(mpos[0] == 0.0 && mpos[2] == 1.0 && mxy[0] == 11.0 && mxy[1] == 21.0);
  CHECK(kbest[1] == 0 && kbest[2] == 0 && kbest[3] == 0 && kbest[4] == 0);
  gp.mutual = 0;
  CHECK(rspl_lmap_debug_global_host(&P, &gp, &R) == RSPL_OK && R.n_matched == 2 && match[2] == 0 && mkp[1] == 2);
  // empty operands, NULL outputs
  rspl_lmap_global_result E{};
  P.n_keypoints = 0;
  E.kbest = kbest.data();
  CHECK(rspl_lmap_debug_global_host(&P, &gp, &E) == RSPL_OK && E.n_matched == 0 && kbest[0] == -1 && kbest[4] == -1);
  P.n_keypoints = n1;
  P.n_local = 0;
  E = rspl_lmap_global_result{};
  E.arg = arg.data(); E.best = best.data(); E.second = second.data();
  CHECK(rspl_lmap_debug_global_host(&P, &gp, &E) == RSPL_OK && arg[0] == -1 && best[3] == 4.0 && second[3] == 4.0);
  P.n_local = 1;
  CHECK(rspl_lmap_debug_global_host(&P, &gp, &E) == RSPL_OK && arg[1] == 0 && best[1] == 0.0 && second[1] == 4.0);
  CHECK(rspl_lmap_debug_global_host(nullptr, &gp, &E) == RSPL_E_ARG && rspl_lmap_debug_global_host(&P, nullptr, &E) == RSPL_E_ARG);
  int c = 0, q = 0, k = 0;
  CHECK(rspl_lmap_debug_global_plan(400, 65536, &c, &q, &k) == RSPL_OK && c % q == 0 && 256 % k == 0);
  CHECK(rspl_lmap_debug_global_plan(0, 1, &c, &q, &k) == RSPL_E_ARG);
  if (failures) return 1;
  std::printf("reloc_check: ok\n");
  return 0;
}
