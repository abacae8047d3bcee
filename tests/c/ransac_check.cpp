// Host check of csrc/ransac.hpp (test infrastructure): built with the host compiler from the header alone, no
// librspl.  Prints, as JSON, for M = 5 (PnP) and M = 7 (F-matrix) at the given counts and `iters` iterations:
//   live          the subsets draw_subset<M> takes from the live generator (the host samplers' path)
//   walk          the subsets subset_at<M> finds walking the table of raw draws reduced % count, each subset
//                 starting where the one before ended (the gather kernels' path, with their table element types)
//   walk_end      the draw position at which that walk ended
//   draws_needed  draws_needed<M> for the same count and iterations (the handles' table sizing)
#include <cstdio>
#include <vector>

#include "ransac.hpp"

using namespace rspl;

constexpr int kIters = 100, kTable = 4096;

static void print_sets(const char* name, const std::vector<int>& v, int M) {
  printf("\"%s\": [", name);
  for (size_t h = 0; h * M < v.size(); h++) {
    printf("%s[", h ? ", " : "");
    for (int i = 0; i < M; i++) printf("%s%d", i ? ", " : "", v[h * M + i]);
    printf("]");
  }
  printf("]");
}

template <int M, class D>
static void check(int count, bool first) {
  std::vector<int> live, walk;
  uint64_t s = (uint64_t)-1;
  for (int h = 0; h < kIters; h++) {
    int32_t o[M];
    if (!ransac::draw_subset<M>(s, count, o)) break;
    live.insert(live.end(), o, o + M);
  }
  const std::vector<uint32_t> raw = ransac::raw_draws(kTable);
  std::vector<D> dv(raw.size());
  for (size_t k = 0; k < raw.size(); k++) dv[k] = (D)(raw[k] % (unsigned)count);
  int pos = 0;
  for (int h = 0; h < kIters; h++) {
    int o[M];
    const int r = ransac::subset_at(dv.data(), (int)dv.size(), pos, o);
    if (!r) break;
    pos += r;
    walk.insert(walk.end(), o, o + M);
  }
  printf("%s\"%d\": {", first ? "" : ", ", count);
  print_sets("live", live, M);
  printf(", ");
  print_sets("walk", walk, M);
  printf(", \"walk_end\": %d, \"draws_needed\": %d}", pos, ransac::draws_needed<M>(raw, count, kIters));
}

int main() {
  printf("{\"5\": {");
  const int c5[] = {8, 9, 64, 300};
  for (int k = 0; k < 4; k++) check<5, int>(c5[k], k == 0);
  printf("}, \"7\": {");
  const int c7[] = {8, 9, 64};
  for (int k = 0; k < 3; k++) check<7, unsigned short>(c7[k], k == 0);
  printf("}}\n");
  return 0;
}
