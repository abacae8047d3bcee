// Host check of the local BA's host-only pieces (test infrastructure): the line-workgroup packing of the staging
// (csrc/ba_stage.cpp: pack_line_blocks into a table sized exactly by line_blocks_bound, so a sanitizer build sees an
// entry past the bound) and the window plan (csrc/ba_plan.cpp: plan_window against chunk_plan and
// set_update_geometry spelled out).  No device call is made: it runs on the CPU.  Exits non-zero on a difference.
// `make -f ba_plan_check.mk ba_plan_check_san` builds it with those sources under ASan + UBSan (host code).
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "ba_handle.hpp"

using namespace rspl;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (failures < 20) std::printf("ba_plan_check: line %d: %s (%s)\n", __LINE__, #cond, what); \
      failures++;                                                    \
    }                                                                \
  } while (0)

constexpr int kB = ba::kLineBlk;

// point landmarks with `pk` edges each, then line landmarks with the given edge counts
static void pack_case(const char* what, int nq, int pk, const std::vector<int>& line_edges) {
  const int nl = (int)line_edges.size(), nL = nq + nl;
  std::vector<int> lm_off(nL + 1, 0);
  for (int g = 0; g < nL; g++) lm_off[g + 1] = lm_off[g] + (g < nq ? pk : line_edges[g - nq]);
  const int e0 = lm_off[nq], e1 = lm_off[nL];
  const size_t bound = ba::line_blocks_bound((size_t)nl, (size_t)(e1 - e0));
  std::unique_ptr<int4[]> ltab(new int4[bound]);  // exactly the bound: an entry past it is a heap overflow
  const int n = ba::pack_line_blocks(lm_off.data(), nq, nL, ltab.get());
  CHECK(n >= 0 && (size_t)n <= bound);
  std::vector<int> covered(e1 - e0, 0);
  int prev_end = e0;
  for (int i = 0; i < n && (size_t)i < bound; i++) {
    const int4 t = ltab[i];
    const int cnt = t.y & 0xff, split = t.y >> 8;
    CHECK(split == 0 || split == 1);
    CHECK(cnt >= 1 && cnt <= kB);
    CHECK(t.x >= prev_end && t.x + cnt <= e1);  // ascending edge order, inside the line edges
    CHECK(t.z >= nq && t.z < t.w && t.w <= nL);
    if (t.z < nq || t.w > nL || t.z >= t.w) continue;
    if (split) {  // one slice of a landmark with more than kB edges, and of that landmark alone
      CHECK(t.w == t.z + 1 && line_edges[t.z - nq] > kB);
      CHECK(t.x >= lm_off[t.z] && t.x + cnt <= lm_off[t.z + 1]);
    } else {  // whole landmarks of at most kB edges each, at most kB of them, at most kB edges together
      CHECK(t.w - t.z <= kB && t.x == lm_off[t.z] && lm_off[t.w] - lm_off[t.z] == cnt);
      for (int g = t.z; g < t.w; g++) CHECK(line_edges[g - nq] <= kB);
    }
    for (int e = t.x; e < t.x + cnt && e < e1; e++)
      if (e >= e0) covered[e - e0]++;
    prev_end = t.x + cnt;
  }
  for (int e = 0; e < e1 - e0; e++) CHECK(covered[e] == 1);
}

static void check_packing() {
  const int counts[7] = {0, 1, 2, kB - 1, kB, kB + 1, 3 * kB + 1};
  for (const int nq : {0, 3}) {
    pack_case("no lines", nq, 2, {});
    pack_case("all lines empty", nq, 2, std::vector<int>(17, 0));
    std::vector<int> ones(kB + 1, 1);  // kB single-edge landmarks fill a workgroup, one more follows
    pack_case("kLineBlk single edges and one more", nq, 1, ones);
    pack_case("runs summing to kLineBlk", nq, 3, {kB - 1, 1, 2, kB - 2, kB, 1, kB - 1, 0, 0, 4, 4, kB});
    pack_case("split landmarks only", nq, 0, {kB + 1, 3 * kB + 1, 2 * kB});
    pack_case("empty landmarks between edges", nq, 1, {1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, kB + 1, 0, 1});
    for (unsigned seed = 1; seed <= 40; seed++) {
      std::mt19937 rng(seed * 7919u + (unsigned)nq);
      const int nl = 1 + (int)(rng() % (seed <= 30 ? 40u : 300u));
      std::vector<int> le(nl);
      // seeds alternate between every count and mostly small ones (long unsplit runs)
      for (int& k : le) k = counts[(seed & 1) ? rng() % 7 : (rng() % 10 < 8 ? rng() % 3 : rng() % 7)];
      char what[64];
      std::snprintf(what, sizeof(what), "seeded nq %d seed %u nl %d", nq, seed, nl);
      pack_case(what, nq, (int)(rng() % 4), le);
    }
  }
}

static void check_window_plan() {
  const int nLs[7] = {0, 1, 511, 512, 513, 3032, 20000};
  char what[96];
  for (int K = 0; K <= 32; K++)
    for (const int nL : nLs)
      for (int cap = 0; cap < 2; cap++) {  // a handle of the window's own size; the largest handle (64 poses)
        const size_t slots = cap ? ba::chunk_slots_for(20000, 64) : ba::chunk_slots_for(nL, K);
        std::snprintf(what, sizeof(what), "K %d nL %d slots %zu", K, nL, slots);
        // the old way, spelled out
        const ba::ChunkPlan cp = ba::chunk_plan(nL, K, slots);
        ba::Active R{};
        R.nchk = cp.nchk; R.lmchunk = cp.lmchunk; R.dsub = cp.dsub; R.lmsub = cp.lmsub;
        R.K = K;
        R.npairs = K * (K + 1) / 2;
        R.nL = nL;
        R.ue_bpr = -7;
        for (int upd = 0; upd < 2; upd++) {
          if (upd) ba::set_update_geometry(R);
          ba::Active A{};
          A.ue_bpr = -7;
          A.Ea = 11;  // (a field the plan does not own)
          ba::plan_window(A, nL, K, slots, upd != 0);
          CHECK(A.nchk == R.nchk && A.lmchunk == R.lmchunk && A.dsub == R.dsub && A.lmsub == R.lmsub);
          CHECK(A.K == R.K && A.npairs == R.npairs && A.nL == R.nL && A.ue_bpr == R.ue_bpr);
          CHECK(ba::chunk_count(A) == ba::chunk_count(R) && ba::chunk_grid(A) == ba::chunk_grid(R));
          CHECK(A.Ea == 11 && A.n_lblk == 0 && A.lm_off == nullptr && A.robust == 0);
        }
      }
}

int main() {
  check_packing();
  check_window_plan();
  if (failures) {
    std::printf("ba_plan_check: %d failures\n", failures);
    return 1;
  }
  std::printf("ba_plan_check: ok\n");
  return 0;
}
