// Host check of the local map tracking handle (test infrastructure): csrc/lmap.cpp's bank / local-table bookkeeping
// on a host-only handle (device < 0: no device call is made) and rspl_lmap_debug_search_host, the host instantiation
// of csrc/lmap_match.hpp, on a scene whose answers are known exactly (identity pose, power-of-two camera, descriptors
// made of a few unit entries so every dot product is exact).  Exits non-zero on the first difference.
// `make -f lmap_check.mk lmap_check_san` builds it with the library's sources under ASan + UBSan (host code only);
// it runs on the CPU.  The two rspl_track_* calls lmap.cpp chains into are stubbed below -- nothing here reaches them.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rspl.h"
#include "lmap_match.hpp"

extern "C" int rspl_track_keyframe_table(rspl_track*, int, int, double**, uint8_t**, int32_t**) { return RSPL_E_ARG; }
extern "C" int rspl_track_enqueue(rspl_track*, int, const rspl_track_frame*, void*) { return RSPL_E_ARG; }

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("lmap_check: line %d: %s\n", __LINE__, #cond);      \
      failures++;                                                     \
    }                                                                 \
  } while (0)

static std::vector<double> desc(std::initializer_list<std::pair<int, double>> e) {
  std::vector<double> d(256, 0.0);
  for (auto& kv : e) d[kv.first] = kv.second;
  return d;
}

static void bank() {
  rspl_lmap_config cfg{4, 3, 8, 1, -1, 15.0, 0.35, 0.6};
  rspl_lmap* h = nullptr;
  CHECK(rspl_lmap_create(&cfg, &h) == RSPL_OK && h);
  std::vector<double> D(3 * 256, 0.25);
  const int32_t a[3] = {7, 9, 11}, b[3] = {11, 20, 21}, c[2] = {20, 20}, neg[1] = {-3};
  int n = -1;
  CHECK(rspl_lmap_store_host(h, 0, nullptr, nullptr) == RSPL_OK);
  CHECK(rspl_lmap_set_local(h, 0, nullptr, nullptr, nullptr) == RSPL_OK);
  CHECK(rspl_lmap_store_host(h, 3, a, D.data()) == RSPL_OK && rspl_lmap_bank_size(h, &n) == RSPL_OK && n == 3);
  CHECK(rspl_lmap_store_host(h, 1, a + 1, D.data()) == RSPL_OK && rspl_lmap_bank_size(h, &n) == RSPL_OK && n == 3);
  CHECK(rspl_lmap_store_host(h, 3, b, D.data()) == RSPL_E_CAPACITY && rspl_lmap_bank_size(h, &n) == RSPL_OK && n == 3);
  CHECK(rspl_lmap_store_host(h, 1, neg, D.data()) == RSPL_E_ARG);
  CHECK(rspl_lmap_store_host(h, 2, c, D.data()) == RSPL_OK && rspl_lmap_bank_size(h, &n) == RSPL_OK && n == 4);
  const double pos[12] = {0, 0, 1, 0, 0, 2, 0, 0, 3, 0, 0, 4};
  const int32_t l0[2] = {9, 7}, l1[2] = {9, 21}, l2[4] = {7, 9, 11, 20};
  CHECK(rspl_lmap_set_local(h, 2, l0, pos, nullptr) == RSPL_OK);
  CHECK(rspl_lmap_set_local(h, 2, l1, pos, nullptr) == RSPL_E_ARG && std::strstr(rspl_last_error(), "map point 21"));
  CHECK(rspl_lmap_set_local(h, 4, l2, pos, nullptr) == RSPL_E_ARG);
  const double bad[3] = {0, NAN, 1};
  CHECK(rspl_lmap_set_local(h, 1, l0, bad, nullptr) == RSPL_E_ARG);
  CHECK(rspl_lmap_enqueue(h, 0, nullptr, nullptr) == RSPL_E_ARG);  // host-only: no device side
  CHECK(rspl_lmap_store(h, 1, a, a, D.data(), nullptr) == RSPL_E_ARG);
  rspl_lmap_destroy(h);
  rspl_lmap_destroy(nullptr);
  cfg.max_batch = 0;
  CHECK(rspl_lmap_create(&cfg, &h) == RSPL_E_ARG && !h);
}

static void search() {
  // 512 x 384, fx = fy = 256, cx = 256, cy = 192, bf = 32, identity pose, depth 2: u = 128 x + 256 exactly
  struct Kp { double x, y, ur; int pid; std::vector<double> d; };
  const std::vector<Kp> kp = {
      {100, 100, -1, -1, desc({{0, 1.0}})},               // 0: dist 0 from point 0
      {110, 100, -1, -1, desc({{0, 0.5}, {1, 0.5}})},     // 1: dot 0.5 -> dist 1
      {300, 200, -1, 77, desc({{2, 1.0}})},               // 2: holds a point: never a candidate
      {302, 200, -1, -1, desc({{2, 0.875}, {3, 0.125}})}, // 3: dot 0.875 -> dist 0.25
      {400, 300, -1, -1, desc({{4, 0.5}, {5, 0.5}})},     // 4, 5: identical descriptors, index 5 in the lower cell
      {390, 300, -1, -1, desc({{4, 0.5}, {5, 0.5}})},
  };
  std::vector<double> F(kp.size() * 259, 0.0);
  std::vector<int32_t> pid(kp.size());
  for (size_t i = 0; i < kp.size(); i++) {
    F[259 * i + 1] = kp[i].x;
    F[259 * i + 2] = kp[i].y;
    std::memcpy(&F[259 * i + 3], kp[i].d.data(), sizeof(double) * 256);
    pid[i] = kp[i].pid;
  }
  auto at = [](double u, double v, double z, double* p) {
    p[0] = (u - 256) / 256 * z; p[1] = (v - 192) / 256 * z; p[2] = z;
  };
  const int nl = 8;
  std::vector<double> pos(3 * nl), D(256 * nl, 0.0);
  std::vector<int32_t> ids = {1, 2, 77, 4, 5, 6, 7, 8};
  at(104, 100, 2, &pos[0]);   D[0] = 1.0;                          // best 0 (kp 0), second 1 (kp 1): good
  at(300, 200, 2, &pos[3]);   D[256 + 2] = 1.0;                    // kp 2 is skipped: best 0.25 (kp 3), second 4
  at(300, 200, 2, &pos[6]);                                         // id 77: the frame holds it
  at(0, 100, 2, &pos[9]);                                           // u = 0: off the image
  at(100, 100, 0, &pos[12]);                                        // z = 0: behind
  at(50, 350, 2, &pos[15]);                                         // nothing within 15 px
  at(395, 300, 2, &pos[18]);  D[256 * 6 + 4] = 1.0;                // an exact tie at dist 1: the cell order decides
  at(85, 100, 2, &pos[21]);   D[256 * 7] = 1.0;                    // kp 0 at exactly u + 15: no candidate
  rspl_lmap_host_problem P{};
  P.n_keypoints = (int)kp.size(); P.features = F.data(); P.u_right = nullptr; P.point_id = pid.data();
  P.n_local = nl; P.local_ids = ids.data(); P.local_pos = pos.data(); P.local_desc = D.data();
  for (int k = 0; k < 4; k++) P.Twc[5 * k] = 1.0;
  P.fx = P.fy = 256; P.cx = 256; P.cy = 192; P.bf = 32; P.width = 512; P.height = 384;
  P.radius = 15; P.max_distance = 0.35; P.max_ratio = 0.6;
  std::vector<int32_t> st(nl), bi(nl);
  std::vector<double> b(nl), s2(nl);
  CHECK(rspl_lmap_debug_search_host(&P, st.data(), bi.data(), b.data(), s2.data()) == RSPL_OK);
  const int want_st[nl] = {RSPL_LMAP_GOOD, RSPL_LMAP_GOOD, RSPL_LMAP_NOT_SELECTED, RSPL_LMAP_OFF_IMAGE, RSPL_LMAP_BEHIND,
                           RSPL_LMAP_NO_CANDIDATE, RSPL_LMAP_FAILED, RSPL_LMAP_NO_CANDIDATE};
  const int want_bi[nl] = {0, 3, -1, -1, -1, -1, 5, -1};
  for (int q = 0; q < nl; q++) CHECK(st[q] == want_st[q] && bi[q] == want_bi[q]);
  CHECK(b[0] == 0.0 && s2[0] == 1.0 && b[1] == 0.25 && s2[1] == 4.0 && b[6] == 1.0 && s2[6] == 1.0 && b[5] == 4.0);
  // no keypoints, no local points
  P.n_keypoints = 0;
  CHECK(rspl_lmap_debug_search_host(&P, st.data(), bi.data(), b.data(), s2.data()) == RSPL_OK && st[0] == RSPL_LMAP_NO_CANDIDATE);
  P.n_local = 0;
  CHECK(rspl_lmap_debug_search_host(&P, st.data(), bi.data(), b.data(), s2.data()) == RSPL_OK);
  // the grid key never converts a value an int cannot hold
  using rspl::lmap::cell_key;
  CHECK(cell_key(1e300, -1e300, 0.125, 0.125) == 63 * 48 && cell_key(NAN, 4.0, 0.125, 0.125) == 1);
  CHECK(cell_key(4.0, 3.999, 0.125, 0.125) == 48 && cell_key(511.75, 383.75, 0.125, 0.125) == 63 * 48 + 47);
}

int main() {
  bank();
  search();
  if (failures) return 1;
  std::printf("lmap_check: ok\n");
  return 0;
}
