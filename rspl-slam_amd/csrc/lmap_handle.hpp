// The local map tracking handle (rspl_lmap), shared by lmap.cpp (bank, local table, search by projection, chain) and
// lmap_reloc.cpp (the global descriptor search of the same table).
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "lmap_global.hpp"
#include "lmap_kernels.hpp"

struct rspl_lmap {
  rspl_lmap_config cfg{};
  bool host_only = false;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr, store_ev = nullptr, local_ev = nullptr;
  rspl::Arena arena;
  rspl::PinnedArena pinned;
  rspl::lmap::Args a{};
  // the bank: id -> row; rows are handed out in order and never freed
  std::unordered_map<int, int> row_of;
  double* bank = nullptr;             // device [max_bank_points][256]
  std::vector<double> host_bank;      // a host-only handle's descriptors
  // the local map: the device arrays (pieces of `arena`) and their host-mapped staging
  int n_local = 0;
  std::vector<int32_t> local_ids;
  int32_t *d_local_row = nullptr, *d_local_id = nullptr;
  double* d_local_pos = nullptr;
  int32_t *s_local_row = nullptr, *s_local_row_dev = nullptr, *s_local_id = nullptr, *s_local_id_dev = nullptr;
  double *s_local_pos = nullptr, *s_local_pos_dev = nullptr;
  int32_t *s_pairs = nullptr, *s_pairs_dev = nullptr;  // rspl_lmap_store's (row, keypoint) pairs
  // host-mapped: the per-frame parameters in, the results out
  rspl::lmap::Param* params = nullptr;
  rspl::lmap::Out* out = nullptr;
  int32_t *o_good_kp = nullptr, *o_good_point = nullptr, *o_assoc = nullptr;
  bool pending = false;
  int batch = 0;        // frames of the last enqueue
  int batch_local = 0;  // the local map's length at that enqueue
  // the global search (rspl_lmap_global_*): its arrays are allocated by the first global enqueue
  bool pending_global = false;  // the enqueue in flight is a global one
  bool g_ready = false;
  rspl::Arena g_arena;
  rspl::PinnedArena g_pinned;
  rspl::lmap::GArgs g{};
  rspl::lmap::GParam* g_params = nullptr;
  rspl::lmap::GOut* g_out = nullptr;
  int32_t *go_arg = nullptr, *go_match = nullptr, *go_kbest = nullptr, *go_m_kp = nullptr, *go_m_local = nullptr,
          *go_m_id = nullptr;
  double *go_best = nullptr, *go_second = nullptr, *go_m_pos = nullptr, *go_m_xy = nullptr;
  int g_batch = 0;
};

namespace rspl {
namespace lmap {

// the last bank store and local-map upload may have gone to other streams than this enqueue's: it waits for both
// (an event never recorded is complete)
inline hipError_t wait_uploads(rspl_lmap* h, hipStream_t st) {
  const hipError_t e = hipStreamWaitEvent(st, h->store_ev, 0);
  return e != hipSuccess ? e : hipStreamWaitEvent(st, h->local_ev, 0);
}

}  // namespace lmap
}  // namespace rspl
