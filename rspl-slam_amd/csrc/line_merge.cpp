// LineDetector's merge passes after the detector, on the host: no HIP call in this file.
//
//   LineDetector::LineExtractor after fld->detect   src/line_processor.cc:460-490
//   LineDetector::MergeLines, MergeTwoLines,
//   FilterShortLines, PointLineDistance, AngleDiff   src/line_processor.cc:11-161, 492-665
//
// The merge is a sequential clustering over a few hundred segments per image (an angle sort, a
// neighbour search that breaks early in sorted order, BFS clusters, pairwise merges whose result
// depends on the order): it stays on the host, in the reference's float / double types.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <set>
#include <unordered_map>
#include <vector>

#include "common.hpp"

#pragma clang fp contract(off)

using namespace rspl;

namespace {

struct Seg {
  float v[4];
};

// line_processor.cc:11-24 (float lines)
void filter_short(std::vector<Seg>& ls, float thr) {
  const float t2 = thr * thr;
  size_t k = 0;
  for (const Seg& s : ls) {
    const float dx = s.v[2] - s.v[0], dy = s.v[3] - s.v[1];
    if (dx * dx + dy * dy > t2) ls[k++] = s;
  }
  ls.resize(k);
}

// line_processor.cc:41-50: float numerator; std::pow(float, int) is a double, so is the root
float point_line_distance(const Seg& l, float x0, float y0) {
  const float x1 = l.v[0], y1 = l.v[1], x2 = l.v[2], y2 = l.v[3];
  const float num = std::fabs((y2 - y1) * x0 + (x1 - x2) * y0 + ((x2 * y1) - (x1 * y2)));
  const double a = (double)(y2 - y1), b = (double)(x1 - x2);
  return (float)(num / std::sqrt(a * a + b * b));
}

// line_processor.cc:92-96
float angle_diff(float a1, float a2) {
  const float c1 = std::fabs(a2 - a1);
  const float c2 = (float)(M_PI + (double)std::min(a1, a2) - (double)std::max(a1, a2));
  return std::min(c1, c2);
}

// line_processor.cc:98-161: length-weighted centroid and angle in double; the angle of each
// segment is atan of the float slope (the float overload, atanf)
Seg merge_two(const Seg& p, const Seg& q) {
  const float ax = p.v[0], ay = p.v[1], bx = p.v[2], by = p.v[3];
  const float cx = q.v[0], cy = q.v[1], dx = q.v[2], dy = q.v[3];
  const float dlix = bx - ax, dliy = by - ay, dljx = dx - cx, dljy = dy - cy;
  const double li = std::sqrt((double)(dlix * dlix) + (double)(dliy * dliy));
  const double lj = std::sqrt((double)(dljx * dljx) + (double)(dljy * dljy));
  const double xg = (li * (double)(ax + bx) + lj * (double)(cx + dx)) / (2.0 * (li + lj));
  const double yg = (li * (double)(ay + by) + lj * (double)(cy + dy)) / (2.0 * (li + lj));
  const double thi = dlix == 0.0f ? M_PI / 2.0 : (double)atanf(dliy / dlix);
  const double thj = dljx == 0.0f ? M_PI / 2.0 : (double)atanf(dljy / dljx);
  double thr;
  if (std::fabs(thi - thj) <= M_PI / 2.0) {
    thr = (li * thi + lj * thj) / (li + lj);
  } else {
    const double tmp = thj - M_PI * (thj / std::fabs(thj));
    thr = (li * thi + lj * tmp) / (li + lj);
  }
  const double s = std::sin(thr), c = std::cos(thr);
  const double g[4] = {((double)ay - yg) * s + ((double)ax - xg) * c, ((double)by - yg) * s + ((double)bx - xg) * c,
                       ((double)cy - yg) * s + ((double)cx - xg) * c, ((double)dy - yg) * s + ((double)dx - xg) * c};
  const double lo = std::min(g[0], std::min(g[1], std::min(g[2], g[3])));
  const double hi = std::max(g[0], std::max(g[1], std::max(g[2], g[3])));
  Seg r;
  r.v[0] = (float)(lo * std::cos(thr) + xg);
  r.v[1] = (float)(lo * std::sin(thr) + yg);
  r.v[2] = (float)(hi * std::cos(thr) + xg);
  r.v[3] = (float)(hi * std::sin(thr) + yg);
  return r;
}

// line_processor.cc:492-665
std::vector<Seg> merge_lines(const std::vector<Seg>& src, float angle_thr, float dist_thr, float ep) {
  const size_t n = src.size();
  std::vector<Seg> dst;
  if (n == 0) return dst;  // the reference maps src[0] of an empty vector (undefined): empty in, empty out
  std::vector<float> ang(n), len(n);
  for (size_t i = 0; i < n; i++) {
    const float dx = src[i].v[2] - src[i].v[0], dy = src[i].v[3] - src[i].v[1];
    ang[i] = atanf(dy / dx);
    len[i] = std::sqrt(dx * dx + dy * dy);
  }
  std::vector<size_t> order(n);
  std::iota(order.begin(), order.end(), 0);
  // equal angles (axis-aligned segments, the two edges of one ridge) keep their input order: the
  // reference's std::sort leaves ties unspecified, the restatement takes them stable
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return ang[a] < ang[b]; });
  const float ep2 = ep * ep, quarter = (float)(M_PI / 4.0);
  // neighbours in the reference's push_back order: by sorted position of the other line
  std::vector<std::vector<size_t>> nbr(n);
  for (size_t i = 0; i < n; i++) {
    const size_t a = order[i];
    float x11 = src[a].v[0], y11 = src[a].v[1], x12 = src[a].v[2], y12 = src[a].v[3];
    const float a1 = ang[a];
    const bool sx = std::fabs(a1) < quarter;
    if ((sx && x12 < x11) || (!sx && y12 < y11)) {
      std::swap(x11, x12);
      std::swap(y11, y12);
    }
    for (size_t j = i + 1; j < n; j++) {
      const size_t b = order[j];
      float x21 = src[b].v[0], y21 = src[b].v[1], x22 = src[b].v[2], y22 = src[b].v[3];
      if ((sx && x22 < x21) || (!sx && y22 < y21)) {
        std::swap(x21, x22);
        std::swap(y21, y22);
      }
      if (angle_diff(a1, ang[b]) > angle_thr) {
        if (std::fabs(a1) < (M_PI_2 - (double)angle_thr)) break;  // sorted: no later line is closer
        continue;
      }
      const float m1x = 0.5f * (src[a].v[0] + src[a].v[2]), m1y = 0.5f * (src[a].v[1] + src[a].v[3]);
      const float m2x = 0.5f * (src[b].v[0] + src[b].v[2]), m2y = 0.5f * (src[b].v[1] + src[b].v[3]);
      if (point_line_distance(src[b], m1x, m1y) > dist_thr && point_line_distance(src[a], m2x, m2y) > dist_thr)
        continue;
      float cx12, cy12, cx21, cy21;
      if ((sx && x12 > x22) || (!sx && y12 > y22)) {
        cx12 = x22; cy12 = y22; cx21 = x11; cy21 = y11;
      } else {
        cx12 = x12; cy12 = y12; cx21 = x21; cy21 = y21;
      }
      bool merge = (sx && cx12 >= cx21) || (!sx && cy12 >= cy21);
      if (!merge) merge = (cx21 - cx12) * (cx21 - cx12) + (cy21 - cy12) * (cy21 - cy12) < ep2;
      if (merge) {
        nbr[a].push_back(b);
        nbr[b].push_back(a);
      }
    }
  }
  // connected components (breadth-first, each frontier in ascending line order)
  std::vector<int> code(n, -1);
  std::vector<std::vector<size_t>> clusters;
  for (size_t i = 0; i < n; i++) {
    if (code[i] >= 0) continue;
    const int c = (int)clusters.size();
    code[i] = c;
    std::vector<size_t> todo = nbr[i], cl{i};
    while (!todo.empty()) {
      std::set<size_t> next;
      for (size_t j : todo) {
        if (code[j] < 0) {
          code[j] = c;
          cl.push_back(j);
        }
        for (size_t k : nbr[j])
          if (code[k] < 0) next.insert(k);
      }
      todo.assign(next.begin(), next.end());
    }
    clusters.push_back(std::move(cl));
  }
  // sub-clusters: longest first, each unclaimed line with its direct neighbours
  std::vector<std::vector<size_t>> subs;
  for (auto& cl : clusters) {
    if (cl.size() <= 2) {
      subs.push_back(cl);
      continue;
    }
    std::stable_sort(cl.begin(), cl.end(), [&](size_t a, size_t b) { return len[a] > len[b]; });
    std::unordered_map<size_t, size_t> at;
    for (size_t k = 0; k < cl.size(); k++) at[cl[k]] = k;
    std::vector<bool> taken(cl.size(), false);
    for (size_t k = 0; k < cl.size(); k++) {
      if (taken[k]) continue;
      std::vector<size_t> sub{cl[k]};
      for (size_t m : nbr[cl[k]]) {
        taken[at[m]] = true;
        sub.push_back(m);
      }
      subs.push_back(std::move(sub));
    }
  }
  dst.reserve(subs.size());
  for (auto& sub : subs) {
    Seg l = src[sub[0]];
    for (size_t k = 1; k < sub.size(); k++) l = merge_two(l, src[sub[k]]);
    dst.push_back(l);
  }
  return dst;
}

}  // namespace

extern "C" int rspl_line_extract(const float* segments, int n, int do_merge, double* lines, int capacity, int* n_out) {
  RSPL_CHECK_ARG(n >= 0 && n_out && (n == 0 || segments) && capacity >= 0 && (capacity == 0 || lines),
                 "rspl_line_extract: bad argument");
  std::vector<Seg> src((size_t)n);
  for (int i = 0; i < n; i++)
    for (int k = 0; k < 4; k++) src[i].v[k] = segments[4 * i + k] * 2;  // detected on the half-size image
  std::vector<Seg> dst;
  if (do_merge) {
    std::vector<Seg> tmp = merge_lines(src, 0.05f, 5.f, 15.f);
    filter_short(tmp, 30.f);
    dst = merge_lines(tmp, 0.03f, 3.f, 50.f);
    filter_short(dst, 60.f);
  } else {
    dst = std::move(src);
  }
  *n_out = (int)dst.size();
  if ((int)dst.size() > capacity) {
    set_error("%zu lines exceed capacity %d", dst.size(), capacity);
    return RSPL_E_CAPACITY;
  }
  for (size_t i = 0; i < dst.size(); i++)
    for (int k = 0; k < 4; k++) lines[4 * i + k] = (double)dst[i].v[k];
  return RSPL_OK;
}
