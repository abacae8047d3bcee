// Host check of csrc/fld_host.hpp (test infrastructure): built with the host compiler from the header, no
// librspl, no device.  Builds the class maps of tests/test_fld_device_cpu.py in C++ (box, border ring, spiral,
// 2 x 2), runs both pieces of the host detector on each, at capacity 0 (no segment buffer) and at ample capacity,
// and exits non-zero on any count other than the one the Python restatement (oracle/fld_ref.py through
// tests/fld_parallel_ref.py) gives for the same map.  The counts do not depend on the half image, which only
// orients a segment.  `make fld_check_san` builds it with ASan + UBSan.
#include <cstdio>
#include <vector>

#include "fld_host.hpp"

using namespace rspl;

struct Map {
  int h, w;
  std::vector<uint8_t> cls;  // 2 strong, 0 candidate, 1 none
  Map(int h_, int w_, uint8_t v) : h(h_), w(w_), cls((size_t)h_ * w_, v) {}
  uint8_t& at(int r, int c) { return cls[(size_t)r * w + c]; }
};

static Map box() {  // a rectangle's outline well inside the image, one strong pixel on its top side
  Map m(24, 40, 1);
  for (int c = 7; c <= 32; c++) m.at(7, c) = m.at(16, c) = 0;
  for (int r = 7; r <= 16; r++) m.at(r, 7) = m.at(r, 32) = 0;
  m.at(7, 20) = 2;
  return m;
}

static Map ring() {  // the image border itself
  Map m(12, 12, 1);
  for (int k = 0; k < 12; k++) m.at(0, k) = m.at(11, k) = m.at(k, 0) = m.at(k, 11) = 0;
  m.at(0, 7) = 2;
  return m;
}

// fld_parallel_ref.spiral_classes: a one-pixel-wide spiral from (0, 0) inwards, one blank pixel between its
// turns, its middle pixel strong
static Map spiral(int n) {
  Map m(n, n, 1);
  std::vector<uint8_t> on((size_t)n * n, 0);
  std::vector<int> path;
  const int dirs[4][2] = {{0, 1}, {1, 0}, {0, -1}, {-1, 0}};
  int r = 0, c = 0, d = 0;
  auto inside = [&](int y, int x) { return y >= 0 && y < n && x >= 0 && x < n; };
  auto ok = [&](int k) {
    const int y = r + dirs[k][0], x = c + dirs[k][1], y2 = y + dirs[k][0], x2 = x + dirs[k][1];
    return inside(y, x) && !on[(size_t)y * n + x] && (!inside(y2, x2) || !on[(size_t)y2 * n + x2]);
  };
  on[0] = 1;
  path.push_back(0);
  for (;;) {
    if (!ok(d)) {
      d = (d + 1) % 4;
      if (!ok(d)) break;
    }
    r += dirs[d][0];
    c += dirs[d][1];
    on[(size_t)r * n + c] = 1;
    path.push_back(r * n + c);
  }
  for (int p : path) m.cls[p] = 0;
  m.cls[path[path.size() / 2]] = 2;
  return m;
}

static int failures = 0;

static void check(const char* name, const Map& m, int len_thr, int want_edges, int want) {
  const size_t hp = (size_t)m.h * m.w;
  std::vector<uint8_t> half(hp);
  for (size_t i = 0; i < hp; i++) half[i] = (uint8_t)(i * 37u + (i >> 3) * 11u);
  fld::HostScratch s;
  std::vector<float> seg(4 * (hp + 1), -1.0f);
  const int caps[2] = {0, (int)hp + 1};
  for (int cap : caps) {
    fld::edges_from_classes(m.cls.data(), m.h, m.w, s);
    int edges = 0;
    for (uint8_t e : s.edge) edges += e != 0;
    const int n = fld::segments_from_edges(half.data(), s.edge.data(), m.h, m.w, len_thr, 1.414213562, s.pts,
                                           cap ? seg.data() : nullptr, cap);
    int left = 0;
    for (uint8_t e : s.edge) left += e != 0;
    const bool ok = edges == want_edges && n == want && left == 0 && (cap == 0 || seg[4 * (size_t)n] == -1.0f);
    printf("%-7s len_thr %2d capacity %5d: %4d edge pixels (want %4d), %2d segments (want %2d), %d pixels left%s\n",
           name, len_thr, cap, edges, want_edges, n, want, left, ok ? "" : "  FAILED");
    failures += !ok;
  }
}

int main() {
  check("box", box(), 3, 68, 4);
  check("box", box(), 10, 68, 2);
  const int ring_thr[3] = {1, 3, 5};
  for (int lt : ring_thr) check("ring", ring(), lt, 24, 0);
  check("spiral", spiral(64), 10, 2077, 43);
  check("2x2", Map(2, 2, 2), 10, 0, 0);
  return failures ? 1 : 0;
}
