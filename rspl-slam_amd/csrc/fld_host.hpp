#pragma once
// The sequential line detector on the host, after Canny's classes: the order-dependent part of
// cv::resize(0.5) + fld->detect (line_processor.cc:455-466, FastLineDetector with do_merge false) as
// oracle/fld_ref.py orders it, in two pieces.  All arithmetic is fld_device.hpp's; here are only the loops
// around it.  Host only, no HIP call: rspl_lines_detect, rspl_lines_debug_fld_host, rspl_lines_debug_fld_classes
// and tests/c/fld_check.cpp run these two functions.
#include <algorithm>
#include <cstring>
#include <vector>

#include "fld_device.hpp"

namespace rspl {
namespace fld {

// buffers that keep their storage between detections
struct HostScratch {
  std::vector<uint8_t> edge;
  std::vector<int> stack;
  std::vector<uint32_t> pts;
};

// an edge map of one byte per pixel (the host's view; BitView is the device's)
struct ByteView {
  const uint8_t* e;
  int w;
  bool operator()(int x, int y) const { return e[(size_t)y * w + x] != 0; }
};

// classes (2 strong, 0 candidate, 1 none) -> s.edge (0 / 255): 8-connected hysteresis from the strong pixels
// (the edge set does not depend on the order), then the corner zeroing of OpenCV's lineDetection (top-left
// 6 x 6, bottom-right 5 x 5)
inline void edges_from_classes(const uint8_t* cls, int hh, int hw, HostScratch& s) {
  const size_t hp = (size_t)hh * hw;
  std::vector<uint8_t>& e = s.edge;
  std::vector<int>& stk = s.stack;
  e.assign(hp, 0);
  stk.clear();
  for (size_t i = 0; i < hp; i++)
    if (cls[i] == 2) {
      e[i] = 255;
      stk.push_back((int)i);
    }
  while (!stk.empty()) {
    const int i = stk.back();
    stk.pop_back();
    const int r = i / hw, c = i - r * hw;
    for (int dr = -1; dr <= 1; dr++)
      for (int dc = -1; dc <= 1; dc++) {
        const int rr = r + dr, cc = c + dc;
        if (rr < 0 || rr >= hh || cc < 0 || cc >= hw) continue;
        const size_t k = (size_t)rr * hw + cc;
        if (cls[k] == 0 && e[k] == 0) {
          e[k] = 255;
          stk.push_back((int)k);
        }
      }
  }
  for (int r = 0; r < std::min(6, hh); r++)
    for (int c = 0; c < std::min(6, hw); c++) e[(size_t)r * hw + c] = 0;
  for (int r = std::max(hh - 5, 0); r < hh; r++)
    for (int c = std::max(hw - 5, 0); c < hw; c++) e[(size_t)r * hw + c] = 0;
}

// edge map -> segments: chains from raster-order seeds (each pixel a chain takes is cleared in `e`), straight
// runs, filters and orientation against the half image.  Returns the segment count; the first `capacity` are
// written.  hh and hw below 65536 (pack_pt).
inline int segments_from_edges(const uint8_t* half, uint8_t* e, int hh, int hw, int len_thr, double dist_thr,
                               std::vector<uint32_t>& pts, float* segments, int capacity) {
  const ByteView edge{e, hw};
  int n = 0;
  for (int r = 0; r < hh; r++)
    for (int c = 0; c < hw; c++) {
      if (!edge(c, r)) continue;
      pts.clear();
      pts.push_back(pack_pt(c, r));
      e[(size_t)r * hw + c] = 0;
      int x = c, y = r, direction = 0, step = 0;
      while (chain_step(edge, hh, hw, x, y, direction, step)) {
        pts.push_back(pack_pt(x, y));
        step++;
        e[(size_t)y * hw + x] = 0;
      }
      if ((int)pts.size() < len_thr + 1) continue;
      extract_segments(pts.data(), (int)pts.size(), len_thr, dist_thr,
                       [&](int, double x1, double y1, double x2, double y2) {
                         float o[4];
                         if (!finish_segment(half, hh, hw, len_thr, x1, y1, x2, y2, o)) return;
                         if (n < capacity) memcpy(segments + 4 * (size_t)n, o, sizeof(o));
                         n++;
                       });
    }
  return n;
}

}  // namespace fld
}  // namespace rspl
