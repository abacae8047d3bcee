// Map-side local BA: the keyframe / map-point / map-line graph the reference's Map keeps, and
// Map::LocalMapOptimization around LocalmapOptimization -- which keyframes, landmarks and
// observations enter the BA, the write-back, the outlier removal and the covisibility update.
//
// Reference (restated, not translated): src/map.cc:121-177 (UppdateMapline), :471-535
// (SearchNeighborFrames, AddFrameVertex), :537-808 (LocalMapOptimization), :810-895
// (MakeFramePair, RemoveOutliers, RemoveLineOutliers), :897-937 (UpdateFrameConnection),
// :1007-1024 (SaveKeyframeTrajectory); src/frame.cc:214-219, 372-405, 448-531 (keypoint / line
// accessors, covisibility bookkeeping); src/mappoint.cc, src/mapline.cc (observers, types).
//
// Shared pointers become ids: a frame / landmark is named by its id, and a slot of a frame's
// _mappoints / _maplines vector holds a landmark id or -1 (nullptr).  The reference orders equal
// covisibility weights (std::set<std::pair<int, FramePtr>>) by shared_ptr address, i.e. by
// allocation order; here ties are ordered by frame id (the same order when keyframes are allocated
// in id order, which is how MapBuilder creates them).
#include <algorithm>
#include <chrono>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <unordered_map>
#include <vector>

#include "common.hpp"

using rspl::set_error;

namespace {

enum { kUnTriangulated = 0, kGood = 1, kBad = 2 };  // Mappoint::Type / Mapline::Type

// The observer maps (frame id -> index) as a sorted vector: std::map's interface and ascending-key
// iteration order, without a heap node per observation (a landmark has tens of observers; the
// local-BA assembly walks every observer of every landmark of the window)
template <typename V>
struct FlatMap {
  using Item = std::pair<int, V>;
  std::vector<Item> v;
  using iterator = typename std::vector<Item>::iterator;
  using const_iterator = typename std::vector<Item>::const_iterator;
  iterator begin() { return v.begin(); }
  iterator end() { return v.end(); }
  const_iterator begin() const { return v.begin(); }
  const_iterator end() const { return v.end(); }
  size_t size() const { return v.size(); }
  bool empty() const { return v.empty(); }
  void clear() { v.clear(); }
  iterator lower(int k) {
    return std::lower_bound(v.begin(), v.end(), k, [](const Item& a, int key) { return a.first < key; });
  }
  const_iterator lower(int k) const {
    return std::lower_bound(v.begin(), v.end(), k, [](const Item& a, int key) { return a.first < key; });
  }
  iterator find(int k) {
    auto it = lower(k);
    return it != v.end() && it->first == k ? it : v.end();
  }
  const_iterator find(int k) const {
    auto it = lower(k);
    return it != v.end() && it->first == k ? it : v.end();
  }
  size_t count(int k) const { return find(k) != v.end(); }
  V& operator[](int k) {
    auto it = lower(k);
    if (it == v.end() || it->first != k) it = v.insert(it, Item(k, V{}));
    return it->second;
  }
  size_t erase(int k) {
    auto it = find(k);
    if (it == v.end()) return 0;
    v.erase(it);
    return 1;
  }
};

// id -> element pointer: a dense table for ids in [0, kDenseIds) (frame / landmark ids are counters),
// the hash map (which owns the elements; node-based, so pointers stay valid) for any other id
constexpr int kDenseIds = 1 << 22;
template <typename T>
struct IdIndex {
  std::vector<T*> dense;
  T* get(const std::unordered_map<int, T>& store, int id) const {
    if (id >= 0 && id < (int)dense.size()) return dense[id];
    if (id >= 0 && id < kDenseIds) return nullptr;  // dense range: absent
    auto it = store.find(id);
    return it == store.end() ? nullptr : const_cast<T*>(&it->second);
  }
  void put(int id, T* p) {
    if (id < 0 || id >= kDenseIds) return;
    if (id >= (int)dense.size()) dense.resize(std::max<size_t>(id + 1, dense.size() * 2), nullptr);
    dense[id] = p;
  }
};

struct MFrame {
  int id = 0;
  double ts = 0;
  double Twc[16] = {};                        // frame pose T_wc, row-major 4 x 4 (Frame::_pose)
  std::vector<std::array<double, 3>> kp;      // features rows 1-2 (x, y) and _u_right
  std::vector<int> mpt;                       // _mappoints: map-point id per keypoint or -1
  std::vector<std::array<double, 4>> ll, lr;  // _lines, _lines_right
  std::vector<uint8_t> lr_valid;              // _lines_right_valid
  std::vector<int> mpl;                       // _maplines: map-line id per line or -1
  std::vector<std::map<int, double>> pol;     // _points_on_lines
  std::map<int, int> conn;                    // _connections: frame id -> weight
  std::set<std::pair<int, int>> oconn;        // _ordered_connections: (weight, frame id)
  int parent = -1;
  int lmo = -1, lmo_fix = -1;                 // local_map_optimization_(fix_)frame_id
  int pidx = -1;                              // pose index in the last assembled problem

  // Frame::AddConnection(frame, weight) (frame.cc:458-469)
  void add_connection(int f, int w) {
    auto it = conn.find(f);
    const bool add = it == conn.end(), change = !add && it->second != w;
    if (add || change) {
      if (change) oconn.erase({it->second, f});
      conn[f] = w;
      oconn.insert({w, f});
    }
  }
  // Frame::AddConnection(set) (frame.cc:471-477)
  void set_connections(const std::set<std::pair<int, int>>& c) {
    oconn = c;
    conn.clear();
    for (auto& kv : c) conn[kv.second] = kv.first;
  }
  // Frame::DecreaseWeight (frame.cc:513-526)
  void decrease_weight(int f, int w) {
    auto it = conn.find(f);
    if (it == conn.end()) return;
    oconn.erase({it->second, f});
    const int ow = it->second;
    const bool remove = (ow < w + 5 && conn.size() >= 2) || ow <= w;
    if (remove) {
      conn.erase(it);
    } else {
      it->second = ow - w;
      oconn.insert({it->second, f});
    }
  }
  // GetKeypointPosition (frame.cc:214-219); the reference accepts idx == cols (an out-of-range
  // read), here idx must be in range
  bool keypoint(int idx, double* k) const {
    if (idx < 0 || idx >= (int)kp.size()) return false;
    for (int i = 0; i < 3; i++) k[i] = kp[idx][i];
    return true;
  }
  bool right_line_status(int idx) const { return idx >= 0 && idx < (int)lr_valid.size() && lr_valid[idx]; }
};

struct MPoint {  // Mappoint
  int id = 0;
  double p[3] = {};
  int type = kUnTriangulated;
  FlatMap<int> obs;        // _obversers: frame id -> keypoint index
  int lmo = -1;
  int observers() const {  // ObverserNum
    int n = 0;
    for (auto& kv : obs) n += kv.second >= 0;
    return n;
  }
  int keypoint_idx(int f) const {
    auto it = obs.find(f);
    return it == obs.end() ? -1 : it->second;
  }
};

struct MLine {  // Mapline
  int id = 0;
  double L[6] = {};  // g2o::Line3D (w, d)
  int type = kUnTriangulated;
  FlatMap<int> obs;         // frame id -> line index
  FlatMap<int> incl;        // _included_endpoints
  int lmo = -1;
  double ep[6] = {};
  bool ep_valid = false, to_update = false;
  int observers() const {
    int n = 0;
    for (auto& kv : obs) n += kv.second >= 0;
    return n;
  }
  int line_idx(int f) const {
    auto it = obs.find(f);
    return it == obs.end() ? -1 : it->second;
  }
};

// Eigen: Quaterniond from a rotation matrix (quaternionbase_assign_impl) -> (x, y, z, w)
void R_to_q(const double* M, int ld, double* q) {
  auto m = [&](int r, int c) { return M[r * ld + c]; };
  double t = m(0, 0) + m(1, 1) + m(2, 2);
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m(2, 1) - m(1, 2)) * t;
    q[1] = (m(0, 2) - m(2, 0)) * t;
    q[2] = (m(1, 0) - m(0, 1)) * t;
  } else {
    int i = 0;
    if (m(1, 1) > m(0, 0)) i = 1;
    if (m(2, 2) > m(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m(k, j) - m(j, k)) * t;
    q[j] = (m(j, i) + m(i, j)) * t;
    q[k] = (m(k, i) + m(i, k)) * t;
  }
}

// Eigen: Quaternion::toRotationMatrix, q = (x, y, z, w), into the upper-left 3 x 3 of a row-major
// matrix with leading dimension ld
void q_to_R(const double* q, double* M, int ld) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  M[0] = 1 - (tyy + tzz); M[1] = txy - twz;       M[2] = txz + twy;
  M[ld] = txy + twz;      M[ld + 1] = 1 - (txx + tzz); M[ld + 2] = tyz - twx;
  M[2 * ld] = txz - twy;  M[2 * ld + 1] = tyz + twx;   M[2 * ld + 2] = 1 - (txx + tyy);
}

// g2o::Line3D::toCartesian: unit direction and the point solving (W^T W + 1e-9 I) p = W^T w,
// W = -[d]x (the point of the line closest to the origin, damped)
void line_to_cartesian(const double* L, double* c) {
  const double* w = L;
  const double* d = L + 3;
  const double dn = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  for (int i = 0; i < 3; i++) c[3 + i] = d[i] / dn;
  const double W[9] = {0, d[2], -d[1], -d[2], 0, d[0], d[1], -d[0], 0};  // -skew(d), row-major
  double A[9], b[3];
  for (int r = 0; r < 3; r++) {
    b[r] = 0;
    for (int k = 0; k < 3; k++) b[r] += W[k * 3 + r] * w[k];
    for (int cc = 0; cc < 3; cc++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += W[k * 3 + r] * W[k * 3 + cc];
      A[r * 3 + cc] = s + (r == cc ? 1e-9 : 0.0);
    }
  }
  // symmetric positive definite 3 x 3: Cholesky solve
  const double l00 = std::sqrt(A[0]), l10 = A[3] / l00, l20 = A[6] / l00;
  const double l11 = std::sqrt(A[4] - l10 * l10), l21 = (A[7] - l20 * l10) / l11;
  const double l22 = std::sqrt(A[8] - l20 * l20 - l21 * l21);
  const double y0 = b[0] / l00, y1 = (b[1] - l10 * y0) / l11, y2 = (b[2] - l20 * y0 - l21 * y1) / l22;
  c[2] = y2 / l22;
  c[1] = (y1 - l21 * c[2]) / l11;
  c[0] = (y0 - l10 * c[1] - l20 * c[2]) / l00;
}

}  // namespace

struct rspl_map {
  double cam[5] = {};
  rspl_map_config cfg{};
  std::unordered_map<int, MFrame> kf;  // _keyframes (by id; id order where the reference iterates it)
  std::vector<int> kf_ids;      // _keyframe_ids (insertion order)
  std::vector<int> kf_sorted;   // the same ids, ascending
  // _mappoints / _maplines: looked up by id only, never iterated (node-based: element pointers stay valid)
  std::unordered_map<int, MPoint> mp;
  std::unordered_map<int, MLine> ml;
  IdIndex<MFrame> kf_ix;
  IdIndex<MPoint> mp_ix;
  IdIndex<MLine> ml_ix;
  // the last assembled problem (rspl_map_last_problem)
  std::vector<int> pose_ids, point_ids, line_ids;
  std::vector<uint8_t> pose_fixed;
  std::vector<int32_t> c_pose[4], c_lm[4];
  std::vector<double> c_obs[4];
  std::vector<uint8_t> c_inl[4];
  // assembly scratch (kept across calls for their capacity): the window's landmarks, their
  // observers flattened, the kept landmarks (id, ordinal) and the ordinal -> dense index map
  struct Obs {
    const MFrame* f;
    int kp;
  };
  std::vector<MPoint*> lm_pts, kept_ptr;
  std::vector<int> lm_beg, lm_rank;
  std::vector<Obs> lm_obs;
  std::vector<std::pair<int, int>> kept_pts;
  // per call, by keyframe id: the frame's class for the window walk and its count of observations
  // outside the window (ids past the table: frame() and a std::map)
  enum : uint8_t { kNoFrame = 0, kWin = 1, kOut = 2, kOutFix = 3 };
  std::vector<uint8_t> fcls;
  std::vector<int> fcnt;
  std::vector<uint64_t> bad;  // remove_outliers scratch: pair keys, the pair table and its used cells
  std::vector<int> pair_cnt, pair_hit;

  MFrame* frame(int id) { return kf_ix.get(kf, id); }
  MPoint* point(int id) { return id < 0 ? nullptr : mp_ix.get(mp, id); }
  MLine* line(int id) { return id < 0 ? nullptr : ml_ix.get(ml, id); }

  // Map::UpdateFrameConnection (map.cc:897-937).  Counts per keyframe id in fcnt (ids past the
  // dense keyframe table in a std::map), read back in ascending id order.
  void update_connection(MFrame& f) {
    const std::vector<MFrame*>& kfd = kf_ix.dense;
    if (fcnt.size() < kfd.size()) fcnt.resize(kfd.size(), 0);
    std::map<int, int> big;
    bool any = false;
    const int nslot = (int)f.mpt.size();
    for (int s = 0; s < nslot; s++) {
      if (s + 8 < nslot)
        if (const MPoint* q = point(f.mpt[s + 8])) __builtin_prefetch(q);
      if (s + 4 < nslot)
        if (const MPoint* q = point(f.mpt[s + 4])) __builtin_prefetch(q->obs.v.data());
      const MPoint* m = point(f.mpt[s]);
      if (!m || m->type == kBad) continue;
      for (auto& kv : m->obs) {
        const int id = kv.first;
        if (id == f.id) continue;
        if ((unsigned)id < kfd.size()) {
          if (!kfd[id]) continue;
          fcnt[id]++;
        } else {
          if (!frame(id)) continue;
          big[id]++;
        }
        any = true;
      }
    }
    if (!any) return;
    std::set<std::pair<int, int>> good;
    int best = -1, best_w = -1;
    auto visit = [&](int id, int w) {  // ascending frame id (the reference's std::map)
      MFrame* cf = frame(id);
      if (w > best_w) {
        best = id;
        best_w = w;
      }
      if (w > 15) {
        good.insert({w, id});
        cf->add_connection(f.id, w);
      }
    };
    auto bi = big.begin();
    for (; bi != big.end() && bi->first < 0; ++bi) visit(bi->first, bi->second);
    for (int id : kf_sorted) {
      if (id < 0 || id >= (int)kfd.size() || !fcnt[id]) continue;
      const int w = fcnt[id];
      fcnt[id] = 0;
      visit(id, w);
    }
    for (; bi != big.end(); ++bi) visit(bi->first, bi->second);
    if (good.empty()) {
      good.insert({best_w, best});
      frame(best)->add_connection(f.id, best_w);
    }
    f.set_connections(good);
  }

  // Map::SearchNeighborFrames (map.cc:471-525); GetOrderedConnections is ascending by weight
  void search_neighbors(MFrame& f, std::vector<MFrame*>& nb) {
    constexpr size_t target = 9;
    const int fid = f.id;
    nb.clear();
    if (kf.size() <= target) {  // every keyframe, in id order (the reference's std::map)
      for (auto& kv : kf) nb.push_back(&kv.second);
      std::sort(nb.begin(), nb.end(), [](const MFrame* a, const MFrame* b) { return a->id < b->id; });
      for (MFrame* k : nb) k->lmo = fid;
      return;
    }
    nb.push_back(&f);
    f.lmo = fid;
    const std::vector<std::pair<int, int>> cs(f.oconn.begin(), f.oconn.end());
    const size_t first = std::min(cs.size(), target - 1);
    for (size_t i = 0; i < first; i++) {
      MFrame* c = frame(cs[i].second);
      c->lmo = fid;
      nb.push_back(c);
    }
    MFrame* par = frame(f.parent);
    if (par && par->lmo != fid) {
      par->lmo = fid;
      nb.push_back(par);
    }
    while (nb.size() < target) {
      std::map<int, int> deeper;
      for (MFrame* k : nb)
        for (auto& wc : k->oconn)
          if (frame(wc.second)->lmo != fid) deeper[wc.second] += wc.first;
      if (deeper.empty()) break;
      std::set<std::pair<int, int>> ord;
      for (auto& kv : deeper) ord.insert({kv.second, kv.first});
      size_t add = std::min(target - nb.size(), ord.size());
      for (auto it = ord.rbegin(); add > 0; add--, ++it) {
        MFrame* c = frame(it->second);
        c->lmo = fid;
        nb.push_back(c);
      }
    }
  }

  // Map::RemoveOutliers (map.cc:818-863).  frame->RemoveMappoint(mpt) runs after the observer was
  // removed, so it looks up index -1 and leaves the frame's slot as it is -- kept as in the reference.
  void remove_outliers(const std::vector<std::pair<int, int>>& outl) {
    // MakeFramePair per (outlier, other observer) as one key, ascending (max, min) order when sorted
    // as unsigned.  Frame ids are offset by 2^31 so that negative ids order too.
    auto key = [](int a, int b) {
      return (uint64_t)((uint32_t)a ^ 0x80000000u) << 32 | (uint32_t)((uint32_t)b ^ 0x80000000u);
    };
    // the pairs are counted first in a (outlier frame, observer id) table -- the outlier frames are
    // the window's few poses -- and only the distinct pairs are sorted; observers past the dense
    // keyframe table go to the key list directly
    const std::vector<MFrame*>& kfd = kf_ix.dense;
    const size_t ncol = kfd.size();
    std::vector<int> rows;  // outlier frame ids, one table row each
    bad.clear();
    pair_hit.clear();
    for (auto& fm : outl) {
      MFrame* f = frame(fm.first);
      MPoint* m = point(fm.second);
      if (!f || !m || m->type == kBad) continue;
      m->obs.erase(f->id);
      const FlatMap<int>& obs = m->obs;  // read before the clear below (the reference copies it under its lock)
      const size_t r = std::find(rows.begin(), rows.end(), f->id) - rows.begin();
      if (r == rows.size()) {
        rows.push_back(f->id);
        if (pair_cnt.size() < rows.size() * ncol) pair_cnt.resize(rows.size() * ncol, 0);
      }
      int* row = pair_cnt.data() + r * ncol;
      for (auto& ob : obs) {
        const int id = ob.first;
        if ((unsigned)id < ncol) {
          if (!kfd[id]) continue;
          if (row[id]++ == 0) pair_hit.push_back((int)(r * ncol) + id);
        } else if (frame(id)) {
          bad.push_back(key(std::max(f->id, id), std::min(f->id, id)));  // MakeFramePair
        }
      }
      if (m->observers() < 2 && m->type != kBad) {
        bool del = true;
        if (m->observers() > 0) {
          MFrame* o = frame(obs.begin()->first);
          if (o) {
            const int k = m->keypoint_idx(o->id);
            if (k >= 0 && k < (int)o->kp.size() && o->kp[k][2] < 0) {  // GetRightPosition(k) < 0: mono
              const int slot = obs.begin()->second;
              if (slot >= 0 && slot < (int)o->mpt.size()) o->mpt[slot] = -1;
            } else {
              del = false;
            }
          }
        }
        if (del) {
          m->type = kBad;
          m->obs.clear();
        }
      }
      // frame->RemoveMappoint(mpt): GetKeypointIdx(frame id) is -1 by now -> no-op
    }
    // the reference's std::map<pair, int> of counts: pairs in ascending order, each with its count
    std::vector<std::pair<uint64_t, int>> cnt;
    cnt.reserve(pair_hit.size() + bad.size());
    for (int h : pair_hit) {
      const int f = rows[h / ncol], o = h % ncol;
      cnt.push_back({key(std::max(f, o), std::min(f, o)), pair_cnt[h]});
      pair_cnt[h] = 0;
    }
    for (uint64_t k : bad) cnt.push_back({k, 1});
    std::sort(cnt.begin(), cnt.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    for (size_t i = 0; i < cnt.size();) {
      size_t j = i;
      int n = 0;
      for (; j < cnt.size() && cnt[j].first == cnt[i].first; j++) n += cnt[j].second;
      const int a = (int)((uint32_t)(cnt[i].first >> 32) ^ 0x80000000u), b = (int)((uint32_t)cnt[i].first ^ 0x80000000u);
      frame(a)->decrease_weight(b, n);
      frame(b)->decrease_weight(a, n);
      i = j;
    }
  }

  // Map::RemoveLineOutliers (map.cc:865-895); the final frame->RemoveMapline is a no-op likewise
  void remove_line_outliers(const std::vector<std::pair<int, int>>& outl) {
    for (auto& fl : outl) {
      MFrame* f = frame(fl.first);
      MLine* l = line(fl.second);
      if (!f || !l || l->type == kBad) continue;
      l->obs.erase(f->id);
      l->incl.erase(f->id);
      const FlatMap<int>& obs = l->obs;
      if (l->observers() < 2 && l->type != kBad) {
        bool del = true;
        if (l->observers() > 0) {
          MFrame* o = frame(obs.begin()->first);
          if (o) {
            if (!o->right_line_status(l->line_idx(o->id))) {
              const int slot = obs.begin()->second;
              if (slot >= 0 && slot < (int)o->mpl.size()) o->mpl[slot] = -1;
            } else {
              del = false;
            }
          }
        }
        if (del) {
          l->type = kBad;
          l->obs.clear();
        }
      }
    }
  }

  // Map::UppdateMapline (map.cc:121-177)
  bool update_mapline(MLine& l) {
    if (l.type != kGood || l.obs.empty()) return false;
    std::vector<std::array<double, 3>> pts;
    for (auto& kv : l.obs) {
      MFrame* f = frame(kv.first);
      if (!f) continue;
      if (kv.second < 0 || kv.second >= (int)f->pol.size()) continue;  // GetPointsOnLine: empty map
      for (auto& pd : f->pol[kv.second]) {
        if (pd.first < 0 || pd.first >= (int)f->mpt.size()) continue;
        const MPoint* m = point(f->mpt[pd.first]);
        if (m && m->type == kGood) pts.push_back({m->p[0], m->p[1], m->p[2]});
      }
    }
    double c[6];
    line_to_cartesian(l.L, c);
    const double* lp = c;
    const double* v = c + 3;
    int md = 0;  // main direction: first index of the largest |component| (Eigen maxCoeff)
    for (int i = 1; i < 3; i++)
      if (std::fabs(v[i]) > std::fabs(v[md])) md = i;
    double mx = DBL_MIN, mn = DBL_MAX;  // DBL_MIN (> 0) as in the reference
    bool fmax = false, fmin = false;
    for (auto& p : pts) {
      const double dp[3] = {p[0] - lp[0], p[1] - lp[1], p[2] - lp[2]};
      const double cr[3] = {v[1] * dp[2] - v[2] * dp[1], v[2] * dp[0] - v[0] * dp[2], v[0] * dp[1] - v[1] * dp[0]};
      const double dist = std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);  // EigenPointLineDistance3D
      if (dist > 0.2) continue;
      const double di = p[md];
      if (di > mx) {
        mx = di;
        fmax = true;
      }
      if (di < mn) {
        mn = di;
        fmin = true;
      }
    }
    if (!fmax || !fmin) return false;
    const double r1 = (mx - lp[md]) / v[md], r2 = (mn - lp[md]) / v[md];
    for (int i = 0; i < 3; i++) {
      l.ep[i] = lp[i] + r1 * v[i];
      l.ep[3 + i] = lp[i] + r2 * v[i];
    }
    l.ep_valid = true;  // SetEndpoints(endpoints, false)
    l.to_update = false;
    return true;
  }

  struct PoseV {
    double q[4], p[3];
    bool fixed;
  };
  // Map::AddFrameVertex (map.cc:527-535): std::map::insert keeps an existing entry
  static void add_vertex(std::map<int, PoseV>& poses, const MFrame& f, bool fixed) {
    if (poses.count(f.id)) return;
    PoseV v;
    R_to_q(f.Twc, 4, v.q);
    for (int i = 0; i < 3; i++) v.p[i] = f.Twc[4 * i + 3];
    v.fixed = fixed;
    poses.emplace(f.id, v);
  }

  // Map::LocalMapOptimization (map.cc:537-808): assembly (into the last-problem vectors), the
  // GPU LocalmapOptimization when ba != null, then outlier removal and write-back
  int local_map_optimization(int fid, rspl_ba* ba, rspl_map_report* rep) {
    MFrame* nf = frame(fid);
    if (!nf) {
      set_error("rspl_map_local_optimization: frame %d is not a keyframe", fid);
      return RSPL_E_ARG;
    }
    static const bool timing = getenv("RSPL_MAP_TIMING") != nullptr;
    using clk = std::chrono::steady_clock;
    clk::time_point tm[6];
    int ntm = 0;
    auto mark = [&]() {
      if (timing) tm[ntm++] = clk::now();
    };
    const auto t_start = clk::now();
    mark();
    update_connection(*nf);
    mark();
    std::map<int, PoseV> poses;
    std::vector<MFrame*> nb;
    search_neighbors(*nf, nb);
    size_t fixed_num = 0;
    for (MFrame* k : nb) {
      const bool fix = k->id == 0;
      fixed_num += fix;
      add_vertex(poses, *k, fix);
    }
    // frame classes: in the window (lmo), outside it, or outside it but marked lmo_fix by an earlier
    // call for this frame id (counted as outside, yet in the window for the constraints, as the
    // reference's two checks read it)
    auto classify = [&](const MFrame* o) -> uint8_t {
      return o->lmo == fid ? kWin : o->lmo_fix == fid ? kOutFix : kOut;
    };
    {
      int top = -1;
      for (int id : kf_ids)
        if (id < kDenseIds) top = std::max(top, id);
      fcls.assign((size_t)(top + 1), kNoFrame);
      if (fcnt.size() < fcls.size()) fcnt.resize(fcls.size(), 0);
      for (int id : kf_ids)
        if (id >= 0 && id <= top) fcls[id] = classify(frame(id));
    }
    std::map<int, int> big_cnt;
    bool any_fixed = false;
    // the window's landmarks in the reference's order (frame by frame, slot by slot), each with its
    // window observers (frame, keypoint index) copied into one flat array, so the constraint pass below
    // reads them sequentially instead of chasing every landmark's observer list a second time; the
    // other observers are only counted per frame (the fixed-frame choice, map.cc:588-602)
    lm_pts.clear();
    lm_beg.clear();
    lm_obs.clear();
    std::vector<int> mpls;
    for (MFrame* k : nb) {
      const int nslot = (int)k->mpt.size();
      for (int s = 0; s < nslot; s++) {
        // the landmarks are scattered heap nodes: fetch the node 8 slots ahead and its observer list 4 ahead
        if (s + 8 < nslot)
          if (const MPoint* q = point(k->mpt[s + 8])) __builtin_prefetch(q);
        if (s + 4 < nslot)
          if (const MPoint* q = point(k->mpt[s + 4])) __builtin_prefetch(q->obs.v.data());
        MPoint* m = point(k->mpt[s]);
        if (!m || m->type != kGood || m->lmo == fid) continue;
        m->lmo = fid;
        lm_pts.push_back(m);
        lm_beg.push_back((int)lm_obs.size());
        for (auto& kv : m->obs) {
          const int id = kv.first;
          uint8_t c;
          if ((unsigned)id < fcls.size()) {
            c = fcls[id];
            if (c >= kOut) fcnt[id]++;
          } else {
            const MFrame* o = frame(id);
            c = o ? classify(o) : kNoFrame;
            if (c >= kOut) big_cnt[id]++;
          }
          if (c == kNoFrame) continue;
          any_fixed |= c >= kOut;
          if (c != kOut) lm_obs.push_back({frame(id), kv.second});
        }
      }
      for (int lid : k->mpl) {
        MLine* l = line(lid);
        if (!l || l->type != kGood || l->lmo == fid) continue;
        l->lmo = fid;
        mpls.push_back(lid);
      }
    }
    lm_beg.push_back((int)lm_obs.size());
    const size_t max_fixed = 1;
    // the frame with the most observations, ties to the larger id (the reference's
    // std::set<pair<int, FramePtr>> read from rbegin; max_fixed - fixed_num is at most 1)
    int fx_id = -1, fx_w = 0;
    auto consider = [&](int id, int w) {
      if (w > fx_w || (w == fx_w && w > 0 && id > fx_id)) {
        fx_id = id;
        fx_w = w;
      }
    };
    for (int id : kf_ids)
      if (id >= 0 && id < (int)fcls.size()) {
        consider(id, fcnt[id]);
        fcnt[id] = 0;
      }
    for (auto& kv : big_cnt) consider(kv.first, kv.second);
    const MFrame* fx = nullptr;  // the fixed frame, when its observations are not in lm_obs yet
    if (any_fixed && max_fixed > fixed_num) {
      MFrame* o = frame(fx_id);
      if (o->lmo_fix != fid) fx = o;
      o->lmo_fix = fid;
      add_vertex(poses, *o, true);
    }
    // dense poses: std::map ids in ascending order (LocalmapOptimization's vertex order); every
    // frame of the window (lmo or lmo_fix == fid) is a vertex and learns its index here
    pose_ids.clear(); point_ids.clear(); line_ids.clear(); pose_fixed.clear();
    std::vector<double> pq, pp, X, Ls;
    for (auto& kv : poses) {
      frame(kv.first)->pidx = (int)pose_ids.size();
      pose_ids.push_back(kv.first);
      pose_fixed.push_back(kv.second.fixed);
      pq.insert(pq.end(), kv.second.q, kv.second.q + 4);
      pp.insert(pp.end(), kv.second.p, kv.second.p + 3);
    }
    mark();
    auto in_window = [&](const MFrame* o) { return o->lmo == fid || o->lmo_fix == fid; };
    // constraints in the reference's order: landmark by landmark, observers by frame id (the fixed
    // frame's observation, looked up in the landmark's observer map, merged into that order), written
    // straight into the dense arrays; a landmark that is dropped (no stereo and at most one mono
    // observation) has its rows taken back.  c_lm holds the kept landmark's ordinal until the
    // landmarks are numbered by id below.
    for (int t = 0; t < 4; t++) {
      c_pose[t].clear(); c_lm[t].clear(); c_obs[t].clear();
    }
    kept_pts.clear();
    kept_ptr.clear();
    for (size_t li = 0; li < lm_pts.size(); li++) {
      const size_t b0 = c_pose[0].size(), b1 = c_pose[1].size();
      const int ord_lm = (int)kept_pts.size();
      auto emit = [&](const MFrame* o, int kpi) {
        if (kpi < 0 || kpi >= (int)o->kp.size()) return;  // GetKeypointPosition
        const double* k = o->kp[kpi].data();
        const int t = k[2] > 0 ? 1 : 0;
        c_pose[t].push_back(o->pidx);
        c_lm[t].push_back(ord_lm);
        c_obs[t].insert(c_obs[t].end(), k, k + 2 + t);
      };
      int fx_kp = fx ? lm_pts[li]->keypoint_idx(fx->id) : -1;
      for (int j = lm_beg[li]; j < lm_beg[li + 1]; j++) {
        const MFrame* o = lm_obs[j].f;
        if (fx_kp >= 0 && o->id > fx->id) {
          emit(fx, fx_kp);
          fx_kp = -1;
        }
        emit(o, lm_obs[j].kp);
      }
      if (fx_kp >= 0) emit(fx, fx_kp);
      if (c_pose[1].size() > b1 || c_pose[0].size() > b0 + 1) {
        kept_pts.push_back({lm_pts[li]->id, ord_lm});
        kept_ptr.push_back(lm_pts[li]);
      } else {
        c_pose[0].resize(b0); c_lm[0].resize(b0); c_obs[0].resize(2 * b0);
        c_pose[1].resize(b1); c_lm[1].resize(b1); c_obs[1].resize(3 * b1);
      }
    }
    std::vector<std::pair<int, MLine*>> kept_lines;
    for (int lid : mpls) {
      MLine* l = line(lid);
      if (!l || l->type != kGood) continue;
      const size_t b0 = c_pose[2].size(), b1 = c_pose[3].size();
      const int ord_lm = (int)kept_lines.size();
      for (auto& kv : l->obs) {
        MFrame* o = frame(kv.first);
        if (!o || !in_window(o)) continue;
        if (kv.second < 0 || kv.second >= (int)o->ll.size()) continue;  // GetLine
        const int t = o->right_line_status(kv.second) ? 3 : 2;          // GetLineRight
        c_pose[t].push_back(o->pidx);
        c_lm[t].push_back(ord_lm);
        c_obs[t].insert(c_obs[t].end(), o->ll[kv.second].begin(), o->ll[kv.second].end());
        if (t == 3) c_obs[t].insert(c_obs[t].end(), o->lr[kv.second].begin(), o->lr[kv.second].end());
      }
      if (c_pose[3].size() > b1 || c_pose[2].size() > b0 + 1) {
        kept_lines.push_back({lid, l});
      } else {
        c_pose[2].resize(b0); c_lm[2].resize(b0); c_obs[2].resize(4 * b0);
        c_pose[3].resize(b1); c_lm[3].resize(b1); c_obs[3].resize(8 * b1);
      }
    }
    mark();
    // dense landmarks: ascending id; constraint rows renumbered from the ordinal
    std::sort(kept_pts.begin(), kept_pts.end());
    lm_rank.resize(kept_pts.size());
    X.resize(3 * kept_pts.size());
    point_ids.resize(kept_pts.size());
    for (size_t i = 0; i < kept_pts.size(); i++) {
      const MPoint* m = kept_ptr[kept_pts[i].second];
      lm_rank[kept_pts[i].second] = (int)i;
      point_ids[i] = kept_pts[i].first;
      for (int c = 0; c < 3; c++) X[3 * i + c] = m->p[c];
    }
    for (int t = 0; t < 2; t++)
      for (auto& v : c_lm[t]) v = lm_rank[v];
    std::vector<int> line_rank(kept_lines.size());
    {
      std::vector<int> o(kept_lines.size());
      for (size_t i = 0; i < o.size(); i++) o[i] = (int)i;
      std::sort(o.begin(), o.end(), [&](int a, int b) { return kept_lines[a].first < kept_lines[b].first; });
      Ls.resize(6 * o.size());
      line_ids.resize(o.size());
      for (size_t i = 0; i < o.size(); i++) {
        line_rank[o[i]] = (int)i;
        line_ids[i] = kept_lines[o[i]].first;
        std::copy(kept_lines[o[i]].second->L, kept_lines[o[i]].second->L + 6, Ls.begin() + 6 * i);
      }
    }
    for (int t = 2; t < 4; t++)
      for (auto& v : c_lm[t]) v = line_rank[v];
    for (int t = 0; t < 4; t++) c_inl[t].assign(c_pose[t].size(), 1);
    if (rep) {
      memset(rep, 0, sizeof(*rep));
      rep->n_poses = (int)pose_ids.size();
      for (uint8_t f : pose_fixed) rep->n_fixed += f;
      rep->n_points = (int)point_ids.size();
      rep->n_lines = (int)line_ids.size();
      rep->n_mono = (int)c_pose[0].size();
      rep->n_stereo = (int)c_pose[1].size();
      rep->n_mono_line = (int)c_pose[2].size();
      rep->n_stereo_line = (int)c_pose[3].size();
    }
    mark();
    if (timing && ntm == 5) {
      auto us = [&](int i) { return std::chrono::duration<double, std::micro>(tm[i + 1] - tm[i]).count(); };
      fprintf(stderr, "rspl_map assembly us: connections %.0f window %.0f constraints %.0f dense %.0f\n", us(0), us(1),
              us(2), us(3));
    }
    last_fid = fid;
    last_cons_ok = true;
    if (!ba) return RSPL_OK;  // assembly only (rspl_map_assemble)
    const int np = (int)pose_ids.size();
    std::vector<double> rq(4 * (size_t)np), rp(3 * (size_t)np), rX(X.size()), rL(Ls.size());
    rspl_ba_problem P{};
    P.n_cameras = 1;
    P.cameras = cam;
    P.n_poses = np;
    P.pose_q = pq.data();
    P.pose_p = pp.data();
    P.pose_fixed = pose_fixed.data();
    P.n_points = (int)point_ids.size();
    P.points = X.data();
    P.n_lines = (int)line_ids.size();
    P.lines = Ls.data();
    P.n_mono = (int)c_pose[0].size(); P.mono_pose = c_pose[0].data(); P.mono_point = c_lm[0].data(); P.mono_obs = c_obs[0].data();
    P.n_stereo = (int)c_pose[1].size(); P.stereo_pose = c_pose[1].data(); P.stereo_point = c_lm[1].data(); P.stereo_obs = c_obs[1].data();
    P.n_mono_line = (int)c_pose[2].size(); P.mono_line_pose = c_pose[2].data(); P.mono_line_line = c_lm[2].data();
    P.mono_line_obs = c_obs[2].data();
    P.n_stereo_line = (int)c_pose[3].size(); P.stereo_line_pose = c_pose[3].data(); P.stereo_line_line = c_lm[3].data();
    P.stereo_line_obs = c_obs[3].data();
    P.th_mono_point = cfg.th_mono_point; P.th_stereo_point = cfg.th_stereo_point;
    P.th_mono_line = cfg.th_mono_line; P.th_stereo_line = cfg.th_stereo_line;
    P.iterations_first = cfg.iterations_first;
    P.iterations_second = cfg.iterations_second;
    rspl_ba_result R{};
    R.pose_q = rq.data(); R.pose_p = rp.data(); R.points = rX.data(); R.lines = rL.data();
    R.mono_inlier = c_inl[0].data(); R.stereo_inlier = c_inl[1].data();
    R.mono_line_inlier = c_inl[2].data(); R.stereo_line_inlier = c_inl[3].data();
    const auto t_ba = clk::now();
    const int rc = rspl_ba_local(ba, &P, &R);
    if (rc) return rc;
    const auto t_fin = clk::now();
    const int rf = finish(R, rep);
    if (rep) {
      auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
      rep->assembly_us = us(t_start, t_ba);
      rep->ba_us = us(t_ba, t_fin);
      rep->finish_us = us(t_fin, clk::now());
    }
    return rf;
  }

  // the part of Map::LocalMapOptimization after LocalmapOptimization returns (map.cc:712-802), on
  // the last assembled problem: outliers, covisibility, write-back
  int last_fid = -1;
  bool last_cons_ok = false;
  int finish(const rspl_ba_result& R, rspl_map_report* rep) {
    if (!last_cons_ok || !frame(last_fid)) {
      set_error("rspl_map_finish: no assembled problem");
      return RSPL_E_ARG;
    }
    last_cons_ok = false;
    MFrame* nf = frame(last_fid);
    static const bool timing = getenv("RSPL_MAP_TIMING") != nullptr;
    using clk = std::chrono::steady_clock;
    clk::time_point tm[8];
    int ntm = 0;
    auto mark = [&]() {
      if (timing) tm[ntm++] = clk::now();
    };
    mark();
    const int np = (int)pose_ids.size();
    const double* rq = R.pose_q;
    const double* rp = R.pose_p;
    const double* rX = R.points;
    const double* rL = R.lines;
    const uint8_t* inl[4] = {R.mono_inlier, R.stereo_inlier, R.mono_line_inlier, R.stereo_line_inlier};
    for (int t = 0; t < 4; t++)
      if (inl[t]) std::copy(inl[t], inl[t] + c_pose[t].size(), c_inl[t].begin());
    if (rep) {
      rep->chi2_first = R.chi2_first;
      rep->chi2_second = R.chi2_second;
      rep->iterations_first = R.iterations_done_first;
      rep->iterations_second = R.iterations_done_second;
    }
    // outliers (map.cc:712-757), in constraint order: mono then stereo points, then lines
    std::vector<std::pair<int, int>> outl, loutl;
    for (int t = 0; t < 4; t++) {
      const std::vector<int>& ids = t < 2 ? point_ids : line_ids;
      for (size_t i = 0; i < c_pose[t].size(); i++) {
        if (c_inl[t][i]) continue;
        const int f = pose_ids[c_pose[t][i]], l = ids[c_lm[t][i]];
        if (!frame(f)) continue;
        if (t < 2 && point(l)) outl.push_back({f, l});
        if (t >= 2 && line(l)) loutl.push_back({f, l});
      }
    }
    if (rep) {
      rep->n_point_outliers = (int)outl.size();
      rep->n_line_outliers = (int)loutl.size();
    }
    mark();
    remove_outliers(outl);
    remove_line_outliers(loutl);
    mark();
    update_connection(*nf);
    mark();
    // write-back (map.cc:767-802)
    for (int i = 0; i < np; i++) {
      MFrame* f = frame(pose_ids[i]);
      if (!f) continue;
      double T[16] = {};
      q_to_R(rq + 4 * (size_t)i, T, 4);
      for (int r = 0; r < 3; r++) T[4 * r + 3] = rp[3 * (size_t)i + r];
      T[15] = 1.0;
      memcpy(f->Twc, T, sizeof(T));
    }
    for (size_t i = 0; i < point_ids.size(); i++) {
      if (i + 8 < point_ids.size()) __builtin_prefetch(point(point_ids[i + 8]), 1);
      MPoint* m = point(point_ids[i]);
      if (!m) continue;
      for (int k = 0; k < 3; k++) m->p[k] = rX[3 * i + k];
      if (m->type == kUnTriangulated) m->type = kGood;
    }
    for (size_t i = 0; i < line_ids.size(); i++) {
      MLine* l = line(line_ids[i]);
      if (!l) continue;
      for (int k = 0; k < 6; k++) l->L[k] = rL[6 * i + k];
      l->to_update = true;  // SetLine3D
      if (l->type == kUnTriangulated) l->type = kGood;
      l->ep_valid = update_mapline(*l);
    }
    mark();
    if (timing && ntm == 5) {
      auto us = [&](int i) { return std::chrono::duration<double, std::micro>(tm[i + 1] - tm[i]).count(); };
      fprintf(stderr, "rspl_map finish us: outliers %.0f remove %.0f connections %.0f write-back %.0f\n", us(0), us(1),
              us(2), us(3));
    }
    return RSPL_OK;
  }
};

// ---------------------------------------------------------------------------------------------
// Map::InsertKeyframe's landmark half (map.cc:31-102): line fit and line triangulation on the host
// ---------------------------------------------------------------------------------------------
namespace {

struct P3f {
  float x, y, z;
};

// cv::fitLine(points, DIST_L2) for 3-D points, restated from the published algorithm (OpenCV is not a
// dependency, so the parity of this function is unpinned): raw moments and the mean in float, the central
// second moments, the matrix whose smallest eigenvector is the principal axis of the scatter, and that
// eigenvector by a cyclic Jacobi (8 sweeps over (0,1), (0,2), (1,2), rational rotations: + - * / sqrt
// only, all in float).  line = direction (unit) | mean.
void fit_line_l2(const std::vector<P3f>& pts, float* line) {
#pragma clang fp contract(off)
  float x0 = 0, y0 = 0, z0 = 0, x2 = 0, y2 = 0, z2 = 0, xy = 0, yz = 0, xz = 0;
  for (const P3f& p : pts) {
    x2 += p.x * p.x; y2 += p.y * p.y; z2 += p.z * p.z;
    xy += p.x * p.y; yz += p.y * p.z; xz += p.x * p.z;
    x0 += p.x; y0 += p.y; z0 += p.z;
  }
  const float w0 = (float)pts.size();
  x2 /= w0; y2 /= w0; z2 /= w0; xy /= w0; yz /= w0; xz /= w0; x0 /= w0; y0 /= w0; z0 /= w0;
  const float dx2 = x2 - x0 * x0, dy2 = y2 - y0 * y0, dz2 = z2 - z0 * z0;
  const float dxy = xy - x0 * y0, dxz = xz - x0 * z0, dyz = yz - y0 * z0;
  float a[3][3] = {{dz2 + dy2, -dxy, -dxz}, {-dxy, dx2 + dz2, -dyz}, {-dxz, -dyz, dy2 + dx2}};
  float v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  static const int PQ[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};  // p, q and the third index
  for (int sweep = 0; sweep < 8; sweep++) {
    for (int k = 0; k < 3; k++) {
      const int p = PQ[k][0], q = PQ[k][1], r = PQ[k][2];
      const float apq = a[p][q];
      if (apq == 0.0f) continue;
      const float theta = (a[q][q] - a[p][p]) / (2.0f * apq);
      const float t = (theta >= 0.0f ? 1.0f : -1.0f) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0f));
      const float c = 1.0f / std::sqrt(t * t + 1.0f), s = t * c;
      a[p][p] = a[p][p] - t * apq;
      a[q][q] = a[q][q] + t * apq;
      a[p][q] = a[q][p] = 0.0f;
      const float arp = a[r][p], arq = a[r][q];
      a[r][p] = a[p][r] = c * arp - s * arq;
      a[r][q] = a[q][r] = s * arp + c * arq;
      for (int i = 0; i < 3; i++) {
        const float vip = v[i][p], viq = v[i][q];
        v[i][p] = c * vip - s * viq;
        v[i][q] = s * vip + c * viq;
      }
    }
  }
  const float e0 = a[0][0], e1 = a[1][1], e2 = a[2][2];
  const int i = e0 < e1 ? (e0 < e2 ? 0 : 2) : (e1 < e2 ? 1 : 2);
  const float n = (float)std::sqrt((double)v[0][i] * v[0][i] + (double)v[1][i] * v[1][i] + (double)v[2][i] * v[2][i]);
  line[0] = v[0][i] / n; line[1] = v[1][i] / n; line[2] = v[2][i] / n;
  line[3] = x0; line[4] = y0; line[5] = z0;
}

// CVPointLineDistance3D (line_processor.cc:52-75), float
float point_line_distance(const P3f& p, const float* line) {
#pragma clang fp contract(off)
  const float x = p.x - line[3], y = p.y - line[4], z = p.z - line[5];
  const float c0 = line[1] * z - line[2] * y, c1 = line[2] * x - line[0] * z, c2 = line[0] * y - line[1] * x;
  return std::sqrt(c0 * c0 + c1 * c1 + c2 * c2);
}

// g2o::Line3D::fromCartesian (point | direction) -> (w, d)
void line_from_cartesian(const double* c, double* L) {
#pragma clang fp contract(off)
  const double n = std::sqrt(c[3] * c[3] + c[4] * c[4] + c[5] * c[5]);
  const double d[3] = {c[3] / n, c[4] / n, c[5] / n};
  const double dp = d[0] * c[0] + d[1] * c[1] + d[2] * c[2];
  const double p[3] = {c[0] - d[0] * dp, c[1] - d[1] * dp, c[2] - d[2] * dp};
  const double q[3] = {p[0] + d[0], p[1] + d[1], p[2] + d[2]};
  L[0] = p[1] * q[2] - p[2] * q[1];
  L[1] = p[2] * q[0] - p[0] * q[2];
  L[2] = p[0] * q[1] - p[1] * q[0];
  L[3] = d[0]; L[4] = d[1]; L[5] = d[2];
}

// Map::TriangulateMaplineByMappoints (map.cc:341-419)
bool triangulate_mapline(rspl_map& M, MLine& l) {
  if (l.type == kGood) return true;
  if (l.obs.size() < 2) return false;
  std::vector<P3f> pts;
  for (auto& kv : l.obs) {
    MFrame* f = M.frame(kv.first);
    if (!f) continue;
    if (kv.second < 0 || kv.second >= (int)f->pol.size()) continue;  // GetPointsOnLine: an empty map
    for (auto& pd : f->pol[kv.second]) {
      if (pd.first < 0 || pd.first >= (int)f->mpt.size()) continue;
      const MPoint* q = M.point(f->mpt[pd.first]);
      if (!q || q->type != kGood) continue;
      pts.push_back({(float)q->p[0], (float)q->p[1], (float)q->p[2]});  // cv::Point3f
    }
  }
  if (pts.size() < 2) return false;
  float line[6];
  for (int round = 0; round < 4; round++) {
    fit_line_l2(pts, line);
    const size_t before = pts.size();
    size_t inl = 0;
    for (size_t j = 0; j < before; j++)
      if ((double)point_line_distance(pts[j], line) < 0.2) pts[inl++] = pts[j];
    pts.resize(inl);
    if (inl == before || inl < 3) break;
  }
  if (pts.size() < 2) return false;
  const double cart[6] = {line[3], line[4], line[5], line[0], line[1], line[2]};
  line_from_cartesian(cart, l.L);
  l.type = kGood;  // SetLine3D
  int md = 0;
  float max_v = std::fabs(line[0]);
  for (int i = 1; i < 3; i++)
    if (std::fabs(line[i]) > max_v) {
      md = i;
      max_v = std::fabs(line[i]);
    }
  // the extreme points along the dominant axis (the reference sorts; on equal coordinates the first wins here)
  auto co = [&](const P3f& p) { return md == 0 ? p.x : (md == 1 ? p.y : p.z); };
  size_t lo = 0, hi = 0;
  for (size_t j = 1; j < pts.size(); j++) {
    if (co(pts[j]) < co(pts[lo])) lo = j;
    if (co(pts[j]) > co(pts[hi])) hi = j;
  }
  const double ep[6] = {pts[lo].x, pts[lo].y, pts[lo].z, pts[hi].x, pts[hi].y, pts[hi].z};
  memcpy(l.ep, ep, sizeof(ep));
  l.ep_valid = true;   // SetEndpoints(endpoints, false)
  l.to_update = false; // SetEndpointsUpdateStatus(false)
  for (auto& kv : l.obs)
    if (M.frame(kv.first)) l.incl[kv.first] = 1;
  return true;
}

double us_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int rspl_map_insert_keyframe(rspl_map* m, const rspl_map_keyframe* k, const rspl_map_tracks* tr,
                                        rspl_kf* kfh, rspl_ba* ba, rspl_map_insert_report* rep) {
  RSPL_CHECK_ARG(m && k && tr, "rspl_map_insert_keyframe: NULL argument");
  RSPL_CHECK_ARG(k->n_keypoints >= 0 && k->n_lines >= 0, "rspl_map_insert_keyframe: negative counts");
  const int n = k->n_keypoints, nl = k->n_lines, fid = k->frame_id;
  RSPL_CHECK_ARG(n == 0 || (tr->track_id && tr->point_slot && tr->new_point && tr->new_position),
                 "rspl_map_insert_keyframe: NULL per-keypoint array");
  const auto t0 = std::chrono::steady_clock::now();
  // everything that can be refused is checked before the map changes
  RSPL_CHECK_ARG(!m->kf.count(fid), "rspl_map_insert_keyframe: frame %d exists", fid);
  {
    std::set<int> fresh;
    for (int i = 0; i < n; i++) {
      if (tr->point_slot[i] >= 0) {
        RSPL_CHECK_ARG(m->point(tr->point_slot[i]), "keypoint %d holds map point %d, which is not in the map", i,
                       tr->point_slot[i]);
      } else if (tr->new_point[i]) {
        const int id = tr->track_id[i];
        RSPL_CHECK_ARG(tr->new_point[i] <= 2 && id >= 0, "keypoint %d: new_point %d with track id %d", i,
                       tr->new_point[i], id);
        RSPL_CHECK_ARG(!m->mp.count(id) && fresh.insert(id).second, "new map point %d is already in the map", id);
      }
    }
  }
  std::vector<int> line_id(nl, -1);
  {
    int next = tr->next_line_track_id ? *tr->next_line_track_id : 0;
    std::set<int> fresh;
    for (int i = 0; i < nl; i++) {
      int id = tr->line_track_id ? tr->line_track_id[i] : -1;
      if (id < 0) {  // map_builder.cc:668-673
        RSPL_CHECK_ARG(tr->next_line_track_id, "line %d needs a track id and next_line_track_id is NULL", i);
        id = next++;
      }
      line_id[i] = id;
      const int slot = tr->line_slot ? tr->line_slot[i] : -1;
      if (slot >= 0) {
        RSPL_CHECK_ARG(m->line(slot), "line %d holds map line %d, which is not in the map", i, slot);
      } else {
        RSPL_CHECK_ARG(!m->ml.count(id) && fresh.insert(id).second, "new map line %d is already in the map", id);
      }
    }
  }
  int rc = rspl_map_add_keyframe(m, k);  // map.cc:26-28
  if (rc) return rc;
  MFrame& f = *m->frame(fid);
  const bool first = m->kf.size() < 2;  // :29 -- the first keyframe's landmarks are MapBuilder::Init's (below)
  rspl_map_insert_report R{};

  // map points (:40-60): a new one per keypoint that holds none, the observer, the candidates
  std::vector<MPoint*> cand;
  for (int i = 0; i < n; i++) {
    MPoint* q = nullptr;
    if (tr->point_slot[i] >= 0) {
      q = m->point(tr->point_slot[i]);
    } else if (tr->new_point[i]) {
      MPoint np;
      np.id = tr->track_id[i];
      if (tr->new_point[i] == 1) {  // SetPosition
        for (int c = 0; c < 3; c++) np.p[c] = tr->new_position[3 * (size_t)i + c];
        np.type = kGood;
      }
      q = &m->mp.emplace(np.id, np).first->second;
      m->mp_ix.put(np.id, q);
      R.n_new_points++;
    } else {
      continue;
    }
    f.mpt[i] = q->id;
    q->obs[fid] = i;
    if (!first && q->type == kUnTriangulated && q->observers() > 2) cand.push_back(q);
  }
  R.bookkeeping_us = us_since(t0);

  // Map::TriangulateMappoint for every candidate, one batch: a candidate reads its own observers and the
  // keyframe poses only, so the batch equals the reference's one-by-one calls inside the loop above
  const auto t1 = std::chrono::steady_clock::now();
  R.n_tri_candidates = (int)cand.size();
  if (!cand.empty()) {
    std::map<int, int> pose_ix;
    std::vector<double> poses, xy, pos(3 * cand.size());
    std::vector<int32_t> off(1, 0), op;
    std::vector<uint8_t> st(cand.size());
    for (MPoint* q : cand) {
      for (auto& kv : q->obs) {  // ascending frame id
        const MFrame* of = m->frame(kv.first);
        int px = -1;
        double kp[3] = {0, 0, 0};
        // (an index >= the frame's keypoint count is an invalid observer: see kf_triangulate.hpp)
        if (of && kv.second >= 0 && of->keypoint(kv.second, kp)) {
          auto it = pose_ix.find(kv.first);
          if (it == pose_ix.end()) {
            it = pose_ix.emplace(kv.first, (int)pose_ix.size()).first;
            poses.insert(poses.end(), of->Twc, of->Twc + 16);
          }
          px = it->second;
        }
        op.push_back(px);
        xy.push_back(kp[0]);
        xy.push_back(kp[1]);
      }
      off.push_back((int32_t)op.size());
    }
    rc = rspl_kf_triangulate(kfh, (int)pose_ix.size(), poses.data(), m->cam, (int)cand.size(), off.data(), op.data(),
                             xy.data(), pos.data(), st.data());
    if (rc) return rc;
    for (size_t c = 0; c < cand.size(); c++) {
      if (st[c] == 1) {  // SetPosition: UnTriangulated -> Good
        for (int j = 0; j < 3; j++) cand[c]->p[j] = pos[3 * c + j];
        cand[c]->type = kGood;
        R.n_tri_ok++;
      } else if (st[c] == 2) {
        R.n_tri_rank_failures++;
      }
    }
  }
  R.triangulation_us = us_since(t1);

  // map lines (:68-102).  Frame::TriangulateStereoLine returns false unconditionally (frame.cc:443), so a
  // new line never gets endpoints from stereo.
  const auto t2 = std::chrono::steady_clock::now();
  for (int i = 0; i < nl; i++) {
    MLine* l = nullptr;
    const int slot = tr->line_slot ? tr->line_slot[i] : -1;
    if (slot >= 0) {
      l = m->line(slot);
    } else {
      MLine nw;
      nw.id = line_id[i];
      l = &m->ml.emplace(nw.id, nw).first->second;
      m->ml_ix.put(nw.id, l);
      R.n_new_lines++;
    }
    f.mpl[i] = l->id;
    l->obs[fid] = i;
    if (l->incl.find(fid) == l->incl.end() || l->incl[fid] < 0) l->incl[fid] = 0;
    if (!first && l->type == kUnTriangulated && l->observers() >= 2) R.n_lines_triangulated += triangulate_mapline(*m, *l);
  }
  if (tr->next_line_track_id) {
    int next = *tr->next_line_track_id;
    for (int i = 0; i < nl; i++)
      if (!tr->line_track_id || tr->line_track_id[i] < 0) next++;
    *tr->next_line_track_id = next;
  }
  R.bookkeeping_us += us_since(t2);
  if (ba && !first) {  // :105-107
    rc = m->local_map_optimization(fid, ba, &R.optimization);
    R.optimized = rc == RSPL_OK;
  }
  if (rep) *rep = R;
  return rc;
}

extern "C" int rspl_map_get_mapline_observers(const rspl_map* m, int id, int32_t* frames, int32_t* lines,
                                              int32_t* endpoint_status, int cap, int* n_observers) {
  RSPL_CHECK_ARG(m, "rspl_map_get_mapline_observers: NULL map");
  auto it = m->ml.find(id);
  RSPL_CHECK_ARG(it != m->ml.end(), "rspl_map_get_mapline_observers: unknown map line %d", id);
  const MLine& l = it->second;
  if (n_observers) *n_observers = (int)l.obs.size();
  int i = 0;
  for (auto& kv : l.obs) {
    if (i >= cap) break;
    if (frames) frames[i] = kv.first;
    if (lines) lines[i] = kv.second;
    if (endpoint_status) {  // Mapline::GetObverserEndpointStatus
      auto s = l.incl.find(kv.first);
      endpoint_status[i] = s == l.incl.end() ? -1 : s->second;
    }
    i++;
  }
  return RSPL_OK;
}

extern "C" int rspl_map_create(const rspl_map_config* cfg, rspl_map** out) {
  RSPL_CHECK_ARG(cfg && out && cfg->camera, "rspl_map_create: NULL argument");
  auto* m = new rspl_map();
  m->cfg = *cfg;
  memcpy(m->cam, cfg->camera, sizeof(m->cam));
  m->cfg.camera = m->cam;
  *out = m;
  return RSPL_OK;
}

extern "C" void rspl_map_destroy(rspl_map* m) { delete m; }

extern "C" int rspl_map_add_keyframe(rspl_map* m, const rspl_map_keyframe* k) {
  RSPL_CHECK_ARG(m && k && k->Twc, "rspl_map_add_keyframe: NULL argument");
  RSPL_CHECK_ARG(k->n_keypoints >= 0 && k->n_lines >= 0, "rspl_map_add_keyframe: negative counts");
  RSPL_CHECK_ARG(!m->kf.count(k->frame_id), "rspl_map_add_keyframe: frame %d exists", k->frame_id);
  MFrame f;
  f.id = k->frame_id;
  f.ts = k->timestamp;
  memcpy(f.Twc, k->Twc, sizeof(f.Twc));
  f.kp.resize(k->n_keypoints);
  for (int i = 0; i < k->n_keypoints; i++)
    for (int c = 0; c < 3; c++) f.kp[i][c] = k->keypoints[3 * i + c];
  f.mpt.assign(k->n_keypoints, -1);
  f.ll.resize(k->n_lines);
  f.lr.resize(k->n_lines);
  f.lr_valid.assign(k->n_lines, 0);
  f.mpl.assign(k->n_lines, -1);
  f.pol.resize(k->n_lines);
  for (int i = 0; i < k->n_lines; i++) {
    for (int c = 0; c < 4; c++) {
      f.ll[i][c] = k->lines_left[4 * i + c];
      f.lr[i][c] = k->lines_right ? k->lines_right[4 * i + c] : 0.0;
    }
    f.lr_valid[i] = k->lines_right_valid ? k->lines_right_valid[i] : 0;
    if (k->pol_offsets)
      for (int j = k->pol_offsets[i]; j < k->pol_offsets[i + 1]; j++) f.pol[i][k->pol_points[j]] = k->pol_dist[j];
  }
  f.parent = k->parent_id;
  const int fid = f.id;
  MFrame* fp = &m->kf.emplace(fid, std::move(f)).first->second;
  m->kf_ix.put(fid, fp);
  m->kf_ids.push_back(k->frame_id);
  m->kf_sorted.insert(std::upper_bound(m->kf_sorted.begin(), m->kf_sorted.end(), fid), fid);
  return RSPL_OK;
}

extern "C" int rspl_map_add_mappoint(rspl_map* m, int id, const double* p, int type) {
  RSPL_CHECK_ARG(m && p && type >= 0 && type <= 2, "rspl_map_add_mappoint: bad argument");
  RSPL_CHECK_ARG(!m->mp.count(id), "rspl_map_add_mappoint: map point %d exists", id);
  MPoint q;
  q.id = id;
  q.type = type;
  for (int i = 0; i < 3; i++) q.p[i] = p[i];
  m->mp_ix.put(id, &m->mp.emplace(id, q).first->second);
  return RSPL_OK;
}

extern "C" int rspl_map_add_mapline(rspl_map* m, int id, const double* line3d, int type) {
  RSPL_CHECK_ARG(m && line3d && type >= 0 && type <= 2, "rspl_map_add_mapline: bad argument");
  RSPL_CHECK_ARG(!m->ml.count(id), "rspl_map_add_mapline: map line %d exists", id);
  MLine l;
  l.id = id;
  l.type = type;
  for (int i = 0; i < 6; i++) l.L[i] = line3d[i];
  m->ml_ix.put(id, &m->ml.emplace(id, l).first->second);
  return RSPL_OK;
}

extern "C" int rspl_map_add_point_observation(rspl_map* m, int point_id, int frame_id, int kp) {
  RSPL_CHECK_ARG(m, "rspl_map_add_point_observation: NULL map");
  MPoint* q = m->point(point_id);
  MFrame* f = m->frame(frame_id);
  RSPL_CHECK_ARG(q && f && kp >= 0 && kp < (int)f->kp.size(), "rspl_map_add_point_observation: bad ids");
  q->obs[frame_id] = kp;  // Mappoint::AddObverser
  f->mpt[kp] = point_id;  // Frame::InsertMappoint
  return RSPL_OK;
}

extern "C" int rspl_map_add_line_observation(rspl_map* m, int line_id, int frame_id, int idx) {
  RSPL_CHECK_ARG(m, "rspl_map_add_line_observation: NULL map");
  MLine* l = m->line(line_id);
  MFrame* f = m->frame(frame_id);
  RSPL_CHECK_ARG(l && f && idx >= 0 && idx < (int)f->ll.size(), "rspl_map_add_line_observation: bad ids");
  l->obs[frame_id] = idx;
  f->mpl[idx] = line_id;
  return RSPL_OK;
}

extern "C" int rspl_map_add_mappoints(rspl_map* m, int n, const int32_t* ids, const double* p, const int32_t* types) {
  RSPL_CHECK_ARG(m && (n == 0 || (ids && p)), "rspl_map_add_mappoints: NULL argument");
  for (int i = 0; i < n; i++) {
    const int rc = rspl_map_add_mappoint(m, ids[i], p + 3 * (size_t)i, types ? types[i] : kGood);
    if (rc) return rc;
  }
  return RSPL_OK;
}

extern "C" int rspl_map_add_point_observations(rspl_map* m, int frame_id, int n, const int32_t* point_ids,
                                               const int32_t* keypoints) {
  RSPL_CHECK_ARG(m && (n == 0 || (point_ids && keypoints)), "rspl_map_add_point_observations: NULL argument");
  for (int i = 0; i < n; i++) {
    const int rc = rspl_map_add_point_observation(m, point_ids[i], frame_id, keypoints[i]);
    if (rc) return rc;
  }
  return RSPL_OK;
}

extern "C" int rspl_map_update_connections(rspl_map* m, int frame_id) {
  RSPL_CHECK_ARG(m && m->frame(frame_id), "rspl_map_update_connections: unknown frame");
  m->update_connection(*m->frame(frame_id));
  return RSPL_OK;
}

extern "C" int rspl_map_local_optimization(rspl_map* m, int frame_id, rspl_ba* ba, rspl_map_report* rep) {
  RSPL_CHECK_ARG(m && ba, "rspl_map_local_optimization: NULL argument");
  return m->local_map_optimization(frame_id, ba, rep);
}

extern "C" int rspl_map_finish(rspl_map* m, const rspl_ba_result* result, rspl_map_report* rep) {
  RSPL_CHECK_ARG(m && result && result->pose_q && result->pose_p, "rspl_map_finish: NULL argument");
  RSPL_CHECK_ARG((m->point_ids.empty() || result->points) && (m->line_ids.empty() || result->lines),
                 "rspl_map_finish: NULL landmark result");
  return m->finish(*result, rep);
}

extern "C" int rspl_map_assemble(rspl_map* m, int frame_id, rspl_map_report* rep) {
  RSPL_CHECK_ARG(m, "rspl_map_assemble: NULL map");
  return m->local_map_optimization(frame_id, nullptr, rep);
}

extern "C" int rspl_map_last_problem(const rspl_map* m, int32_t* pose_ids, uint8_t* pose_fixed, int32_t* point_ids,
                                     int32_t* line_ids, int32_t* const* c_pose, int32_t* const* c_lm,
                                     double* const* c_obs) {
  RSPL_CHECK_ARG(m, "rspl_map_last_problem: NULL map");
  if (pose_ids) std::copy(m->pose_ids.begin(), m->pose_ids.end(), pose_ids);
  if (pose_fixed) std::copy(m->pose_fixed.begin(), m->pose_fixed.end(), pose_fixed);
  if (point_ids) std::copy(m->point_ids.begin(), m->point_ids.end(), point_ids);
  if (line_ids) std::copy(m->line_ids.begin(), m->line_ids.end(), line_ids);
  for (int t = 0; t < 4; t++) {
    if (c_pose && c_pose[t]) std::copy(m->c_pose[t].begin(), m->c_pose[t].end(), c_pose[t]);
    if (c_lm && c_lm[t]) std::copy(m->c_lm[t].begin(), m->c_lm[t].end(), c_lm[t]);
    if (c_obs && c_obs[t]) std::copy(m->c_obs[t].begin(), m->c_obs[t].end(), c_obs[t]);
  }
  return RSPL_OK;
}

extern "C" int rspl_map_get_keyframe(const rspl_map* m, int frame_id, double* Twc, int* n_connections) {
  RSPL_CHECK_ARG(m, "rspl_map_get_keyframe: NULL map");
  auto it = m->kf.find(frame_id);
  RSPL_CHECK_ARG(it != m->kf.end(), "rspl_map_get_keyframe: unknown frame %d", frame_id);
  if (Twc) memcpy(Twc, it->second.Twc, sizeof(double) * 16);
  if (n_connections) *n_connections = (int)it->second.oconn.size();
  return RSPL_OK;
}

extern "C" int rspl_map_get_connections(const rspl_map* m, int frame_id, int32_t* ids, int32_t* weights, int cap,
                                        int* n) {
  RSPL_CHECK_ARG(m && n, "rspl_map_get_connections: NULL argument");
  auto it = m->kf.find(frame_id);
  RSPL_CHECK_ARG(it != m->kf.end(), "rspl_map_get_connections: unknown frame %d", frame_id);
  const auto& oc = it->second.oconn;
  *n = (int)oc.size();
  RSPL_CHECK_ARG(cap >= *n || (!ids && !weights), "rspl_map_get_connections: capacity %d < %d", cap, *n);
  int i = 0;
  for (auto& wc : oc) {  // GetOrderedConnections(-1): ascending weight
    if (ids) ids[i] = wc.second;
    if (weights) weights[i] = wc.first;
    i++;
  }
  return RSPL_OK;
}

extern "C" int rspl_map_get_mappoint(const rspl_map* m, int id, double* p, int* type, int* n_observers,
                                     int32_t* frames, int32_t* kps, int cap) {
  RSPL_CHECK_ARG(m, "rspl_map_get_mappoint: NULL map");
  auto it = m->mp.find(id);
  RSPL_CHECK_ARG(it != m->mp.end(), "rspl_map_get_mappoint: unknown map point %d", id);
  const MPoint& q = it->second;
  if (p) memcpy(p, q.p, sizeof(q.p));
  if (type) *type = q.type;
  if (n_observers) *n_observers = (int)q.obs.size();
  int i = 0;
  for (auto& kv : q.obs) {
    if (i >= cap) break;
    if (frames) frames[i] = kv.first;
    if (kps) kps[i] = kv.second;
    i++;
  }
  return RSPL_OK;
}

extern "C" int rspl_map_get_mapline(const rspl_map* m, int id, double* line3d, int* type, int* n_observers,
                                    double* endpoints, int* endpoints_valid) {
  RSPL_CHECK_ARG(m, "rspl_map_get_mapline: NULL map");
  auto it = m->ml.find(id);
  RSPL_CHECK_ARG(it != m->ml.end(), "rspl_map_get_mapline: unknown map line %d", id);
  const MLine& l = it->second;
  if (line3d) memcpy(line3d, l.L, sizeof(l.L));
  if (type) *type = l.type;
  if (n_observers) *n_observers = (int)l.obs.size();
  if (endpoints) memcpy(endpoints, l.ep, sizeof(l.ep));
  if (endpoints_valid) *endpoints_valid = l.ep_valid;
  return RSPL_OK;
}

extern "C" int rspl_map_get_frame_slots(const rspl_map* m, int frame_id, int32_t* mappoints, int32_t* maplines) {
  RSPL_CHECK_ARG(m, "rspl_map_get_frame_slots: NULL map");
  auto it = m->kf.find(frame_id);
  RSPL_CHECK_ARG(it != m->kf.end(), "rspl_map_get_frame_slots: unknown frame %d", frame_id);
  if (mappoints) std::copy(it->second.mpt.begin(), it->second.mpt.end(), mappoints);
  if (maplines) std::copy(it->second.mpl.begin(), it->second.mpl.end(), maplines);
  return RSPL_OK;
}

// Map::SaveKeyframeTrajectory (map.cc:1007-1024): "timestamp tx ty tz qx qy qz qw" per keyframe in
// insertion order, std::fixed with setprecision(9)
extern "C" int rspl_map_save_trajectory(const rspl_map* m, const char* path) {
  RSPL_CHECK_ARG(m && path, "rspl_map_save_trajectory: NULL argument");
  FILE* f = fopen(path, "w");
  if (!f) {
    set_error("rspl_map_save_trajectory: cannot open %s", path);
    return RSPL_E_ARG;
  }
  for (int id : m->kf_ids) {
    const MFrame& k = m->kf.at(id);
    double q[4];
    R_to_q(k.Twc, 4, q);
    fprintf(f, "%.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n", k.ts, k.Twc[3], k.Twc[7], k.Twc[11], q[0], q[1], q[2], q[3]);
  }
  fclose(f);
  return RSPL_OK;
}

// MapBuilder::UpdateReferenceFrame (map_builder.cc:684-712).  The reference counts in a std::map keyed by
// FramePtr and keeps the first strictly larger count of its pointer-ordered walk; here, as for the covisibility
// ties above, the walk is in ascending frame id.
extern "C" int rspl_map_reference_keyframe(const rspl_map* m, int current_frame_id, int n, const int32_t* point_ids,
                                           int current_ref, int* ref, int* changed) {
  RSPL_CHECK_ARG(m && ref && changed && (n == 0 || point_ids) && n >= 0, "rspl_map_reference_keyframe: bad argument");
  std::map<int, int> votes;
  for (int i = 0; i < n; i++) {
    auto it = point_ids[i] < 0 ? m->mp.end() : m->mp.find(point_ids[i]);
    if (it == m->mp.end() || it->second.type == kBad) continue;  // !mpt || mpt->IsBad()
    for (auto& kv : it->second.obs) {
      if (kv.first == current_frame_id || !m->kf.count(kv.first)) continue;
      votes[kv.first]++;
    }
  }
  int best = current_ref, best_n = -1;
  for (auto& kv : votes)
    if (kv.second > best_n) {
      best = kv.first;
      best_n = kv.second;
    }
  *ref = best;
  *changed = best != current_ref;
  return RSPL_OK;
}

// MapBuilder::UpdateLocalKeyframes + UpdateLocalMappoints (map_builder.cc:714-734): tracking_frame_id's
// "seen in this walk" mark is a set here
extern "C" int rspl_map_local_mappoints(const rspl_map* m, int ref_frame_id, int32_t* ids, double* positions, int cap,
                                        int* n) {
  RSPL_CHECK_ARG(m && n && cap >= 0, "rspl_map_local_mappoints: bad argument");
  auto fit = m->kf.find(ref_frame_id);
  RSPL_CHECK_ARG(fit != m->kf.end(), "rspl_map_local_mappoints: unknown frame %d", ref_frame_id);
  std::vector<const MPoint*> out;
  std::set<int> seen;
  for (auto& wc : fit->second.oconn) {  // GetOrderedConnections(-1): ascending (weight, frame id)
    auto kit = m->kf.find(wc.second);
    if (kit == m->kf.end()) continue;
    for (int id : kit->second.mpt) {
      auto pit = id < 0 ? m->mp.end() : m->mp.find(id);
      if (pit == m->mp.end() || pit->second.type != kGood) continue;  // mpt && mpt->IsValid()
      if (seen.insert(id).second) out.push_back(&pit->second);
    }
  }
  *n = (int)out.size();
  if (cap < *n) {
    set_error("rspl_map_local_mappoints: capacity %d < %d local map points", cap, *n);
    return RSPL_E_CAPACITY;
  }
  for (size_t i = 0; i < out.size(); i++) {
    if (ids) ids[i] = out[i]->id;
    if (positions) memcpy(positions + 3 * i, out[i]->p, sizeof(double) * 3);
  }
  return RSPL_OK;
}

// every Good map point, ascending id (a read-only walk)
extern "C" int rspl_map_good_mappoints(const rspl_map* m, int32_t* ids, double* positions, int cap, int* n) {
  RSPL_CHECK_ARG(m && n && cap >= 0, "rspl_map_good_mappoints: bad argument");
  std::vector<const MPoint*> out;
  for (auto& kv : m->mp)
    if (kv.second.type == kGood) out.push_back(&kv.second);
  std::sort(out.begin(), out.end(), [](const MPoint* a, const MPoint* b) { return a->id < b->id; });
  *n = (int)out.size();
  if (cap < *n) {
    set_error("rspl_map_good_mappoints: capacity %d < %d good map points", cap, *n);
    return RSPL_E_CAPACITY;
  }
  for (size_t i = 0; i < out.size(); i++) {
    if (ids) ids[i] = out[i]->id;
    if (positions) memcpy(positions + 3 * i, out[i]->p, sizeof(double) * 3);
  }
  return RSPL_OK;
}

// ---- loop closure: the pose graph out, the corrected poses back in, the candidate vote ------
// The reference has no such stage.  All three are host walks of the native map.
extern "C" int rspl_map_pose_graph(const rspl_map* m, int min_weight, int32_t* frame_ids, double* pose_q, double* pose_p,
                                   int node_cap, int* n_nodes, int32_t* edge_i, int32_t* edge_j, double* edge_q,
                                   double* edge_p, int32_t* edge_weight, int edge_cap, int* n_edges) {
  RSPL_CHECK_ARG(m && n_nodes && n_edges && node_cap >= 0 && edge_cap >= 0, "rspl_map_pose_graph: bad argument");
  const std::vector<int>& ids = m->kf_sorted;
  std::map<std::pair<int, int>, int> pairs;  // (lower id, higher id) -> connection weight, 0: parent only
  for (int id : ids) {
    const MFrame& f = m->kf.at(id);
    if (f.parent >= 0 && f.parent != id && m->kf.count(f.parent))
      pairs.insert({{std::min(id, f.parent), std::max(id, f.parent)}, 0});
  }
  for (int id : ids)
    for (auto& kv : m->kf.at(id).conn) {
      if (kv.second < min_weight || kv.first == id || !m->kf.count(kv.first)) continue;
      int& w = pairs[{std::min(id, kv.first), std::max(id, kv.first)}];
      w = std::max(w, kv.second);
    }
  *n_nodes = (int)ids.size();
  *n_edges = (int)pairs.size();
  if (node_cap < *n_nodes || edge_cap < *n_edges) {
    set_error("rspl_map_pose_graph: capacities %d, %d < %d keyframes, %d edges", node_cap, edge_cap, *n_nodes, *n_edges);
    return RSPL_E_CAPACITY;
  }
  for (size_t i = 0; i < ids.size(); i++) {
    const MFrame& f = m->kf.at(ids[i]);
    if (frame_ids) frame_ids[i] = ids[i];
    if (pose_q) {
      R_to_q(f.Twc, 4, pose_q + 4 * i);
      const double* q = pose_q + 4 * i;
      const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int c = 0; c < 4; c++) pose_q[4 * i + c] /= nq;
    }
    if (pose_p)
      for (int c = 0; c < 3; c++) pose_p[3 * i + c] = f.Twc[4 * c + 3];
  }
  size_t e = 0;
  for (auto& kv : pairs) {
    const MFrame& a = m->kf.at(kv.first.first);
    const MFrame& b = m->kf.at(kv.first.second);
    if (edge_i) edge_i[e] = (int32_t)(std::lower_bound(ids.begin(), ids.end(), a.id) - ids.begin());
    if (edge_j) edge_j[e] = (int32_t)(std::lower_bound(ids.begin(), ids.end(), b.id) - ids.begin());
    double Rz[9], tz[3];  // Z = T_wa^-1 T_wb
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++)
        Rz[3 * r + c] = a.Twc[r] * b.Twc[c] + a.Twc[4 + r] * b.Twc[4 + c] + a.Twc[8 + r] * b.Twc[8 + c];
      tz[r] = a.Twc[r] * (b.Twc[3] - a.Twc[3]) + a.Twc[4 + r] * (b.Twc[7] - a.Twc[7]) + a.Twc[8 + r] * (b.Twc[11] - a.Twc[11]);
    }
    if (edge_q) {
      double q[4];
      R_to_q(Rz, 3, q);
      const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int c = 0; c < 4; c++) edge_q[4 * e + c] = q[c] / nq;
    }
    if (edge_p) memcpy(edge_p + 3 * e, tz, sizeof(tz));
    if (edge_weight) edge_weight[e] = kv.second;
    e++;
  }
  return RSPL_OK;
}

extern "C" int rspl_map_apply_pose_graph(rspl_map* m, int n, const int32_t* frame_ids, const double* pose_q,
                                         const double* pose_p) {
  RSPL_CHECK_ARG(m && n >= 0 && (n == 0 || (frame_ids && pose_q && pose_p)), "rspl_map_apply_pose_graph: bad argument");
  struct Motion {
    double R[9], t[3];  // T' T^-1
  };
  std::map<int, Motion> motion;
  for (int i = 0; i < n; i++) {
    auto it = m->kf.find(frame_ids[i]);
    RSPL_CHECK_ARG(it != m->kf.end(), "rspl_map_apply_pose_graph: unknown frame %d", frame_ids[i]);
    RSPL_CHECK_ARG(!motion.count(frame_ids[i]), "rspl_map_apply_pose_graph: frame %d listed twice", frame_ids[i]);
    const double* q = pose_q + 4 * (size_t)i;
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    bool finite = std::isfinite(nq) && nq > 0;
    for (int c = 0; c < 3; c++) finite = finite && std::isfinite(pose_p[3 * (size_t)i + c]);
    RSPL_CHECK_ARG(finite, "rspl_map_apply_pose_graph: frame %d: bad pose", frame_ids[i]);
    motion[frame_ids[i]] = Motion{};
  }
  for (int i = 0; i < n; i++) {
    MFrame& f = m->kf.at(frame_ids[i]);
    const double* q = pose_q + 4 * (size_t)i;
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double qn[4] = {q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq};
    double Rn[9];
    q_to_R(qn, Rn, 3);
    Motion& M = motion[frame_ids[i]];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++)
        M.R[3 * r + c] = Rn[3 * r] * f.Twc[4 * c] + Rn[3 * r + 1] * f.Twc[4 * c + 1] + Rn[3 * r + 2] * f.Twc[4 * c + 2];
    for (int r = 0; r < 3; r++)
      M.t[r] = pose_p[3 * (size_t)i + r] - (M.R[3 * r] * f.Twc[3] + M.R[3 * r + 1] * f.Twc[7] + M.R[3 * r + 2] * f.Twc[11]);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) f.Twc[4 * r + c] = Rn[3 * r + c];
      f.Twc[4 * r + 3] = pose_p[3 * (size_t)i + r];
    }
  }
  auto anchor = [&](const FlatMap<int>& obs) -> const Motion* {
    for (auto& kv : obs) {  // ascending frame id
      if (kv.second < 0) continue;
      auto it = motion.find(kv.first);
      if (it != motion.end()) return &it->second;
    }
    return nullptr;
  };
  auto move = [](const Motion& M, const double* x, double* o) {
    const double v[3] = {x[0], x[1], x[2]};
    for (int r = 0; r < 3; r++) o[r] = M.R[3 * r] * v[0] + M.R[3 * r + 1] * v[1] + M.R[3 * r + 2] * v[2] + M.t[r];
  };
  for (auto& kv : m->mp) {
    MPoint& p = kv.second;
    if (p.type != kGood) continue;  // bad, or no position yet
    if (const Motion* M = anchor(p.obs)) move(*M, p.p, p.p);
  }
  for (auto& kv : m->ml) {
    MLine& l = kv.second;
    if (l.type == kBad) continue;
    const Motion* M = anchor(l.obs);
    if (!M) continue;
    // Pluecker (w, d): d' = R d, w' = R w + t x d'
    double w[3], d[3];
    for (int r = 0; r < 3; r++) {
      w[r] = M->R[3 * r] * l.L[0] + M->R[3 * r + 1] * l.L[1] + M->R[3 * r + 2] * l.L[2];
      d[r] = M->R[3 * r] * l.L[3] + M->R[3 * r + 1] * l.L[4] + M->R[3 * r + 2] * l.L[5];
    }
    l.L[0] = w[0] + M->t[1] * d[2] - M->t[2] * d[1];
    l.L[1] = w[1] + M->t[2] * d[0] - M->t[0] * d[2];
    l.L[2] = w[2] + M->t[0] * d[1] - M->t[1] * d[0];
    for (int r = 0; r < 3; r++) l.L[3 + r] = d[r];
    if (l.ep_valid) {
      move(*M, l.ep, l.ep);
      move(*M, l.ep + 3, l.ep + 3);
    }
  }
  return RSPL_OK;
}

extern "C" int rspl_map_loop_candidates(const rspl_map* m, int frame_id, int n, const int32_t* point_ids, int min_gap,
                                        int32_t* ids, int32_t* votes, int cap, int* n_out) {
  RSPL_CHECK_ARG(m && n_out && (n == 0 || point_ids) && n >= 0 && cap >= 0, "rspl_map_loop_candidates: bad argument");
  auto fit = m->kf.find(frame_id);
  RSPL_CHECK_ARG(fit != m->kf.end(), "rspl_map_loop_candidates: unknown frame %d", frame_id);
  std::map<int, int> count;
  for (int i = 0; i < n; i++) {
    auto it = point_ids[i] < 0 ? m->mp.end() : m->mp.find(point_ids[i]);
    if (it == m->mp.end() || it->second.type == kBad) continue;
    for (auto& kv : it->second.obs) {
      const int f = kv.first;
      if (kv.second < 0 || f == frame_id || !m->kf.count(f) || fit->second.conn.count(f)) continue;  // < 0: removed
      if (std::abs((long)f - (long)frame_id) <= (long)min_gap) continue;
      count[f]++;
    }
  }
  std::vector<std::pair<int, int>> order(count.begin(), count.end());  // ascending id
  std::stable_sort(order.begin(), order.end(),
                   [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.second > b.second; });
  *n_out = (int)order.size();
  if (cap < *n_out) {
    set_error("rspl_map_loop_candidates: capacity %d < %d candidates", cap, *n_out);
    return RSPL_E_CAPACITY;
  }
  for (size_t i = 0; i < order.size(); i++) {
    if (ids) ids[i] = order[i].first;
    if (votes) votes[i] = order[i].second;
  }
  return RSPL_OK;
}
