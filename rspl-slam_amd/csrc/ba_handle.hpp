#pragma once
// The rspl_ba handle and what the local BA's host files share (host only: no kernel file includes it):
//   ba.cpp        the handle's life: arena, staging slots, create / destroy, setters, rspl_ba_local
//   ba_lm.cpp     one optimize(iters): the device and the host Levenberg-Marquardt drivers
//   ba_call.cpp   one call: host staging, upload, both optimize() phases, final kernel, write-back
//   ba_queue.cpp  the native tracking thread: staging / tracking loops, submit / join, the trace ring
//   ba_plan.cpp   the Schur chunk plan and the window geometry (no device call)
//   ba_debug.cpp  measurement and test hooks (RSPL_BA_PROF, kernel timing, LM trace, rspl_ba_debug_*)
#include <immintrin.h>
#include <time.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ba_kernels.hpp"
#include "ba_stage.hpp"
#include "common.hpp"

namespace rspl {
namespace ba {

struct StagedCall;  // one call's host staging (below)

constexpr int kMaxCams = 16;
constexpr int kMaxRanks = 64;
constexpr int kParEdges = 8192;    // staging on the host workers from this many edges
constexpr int kChunkWaves = 1024;  // Schur chunk waves of one dispatch round (one wave per SIMD)
constexpr int kEventTrials = 64;   // timing-event triples created by rspl_ba_kernel_timing

// The per-call host timeline record (rspl_ba_trace; include/rspl.h documents the slots and the flag bits)
enum TraceField {
  kTrSubmitted = 0,  // rspl_ba_submit; rspl_ba_local: entry
  kTrStageBegin = 1,
  kTrStageEnd = 2,
  kTrRunBegin = 3,  // device part started (tracking thread)
  kTrUpload = 4,    // upload queued
  kTrOpt1 = 5,      // optimize(10) stopped (mailbox read)
  kTrOpt2 = 6,      // optimize(5) stopped
  kTrDone = 7,      // results written back
  kTrSlot = 8,
  kTrFlags = 9,
  kTrIters = 10,
  kTrLocal = 11,  // 1 for rspl_ba_local, 0 for a submitted call
  kTrWidth = 12
};
static_assert(kTrWidth == RSPL_BA_TRACE_W, "trace record width");
enum TraceFlag : unsigned {
  kGrewStage = 1u,   // a buffer grown inside the call: staging slot,
  kGrewPairs = 2u,   //   edge-pair list,
  kGrewPdg = 4u,     //   pose-diagonal partials,
  kGrewEvents = 8u,  //   timing events
  kSpecSetupRan = 16u,  // optimize(5)'s setup ran from the speculative queue behind optimize(10)'s trials
  kToppedUp = 32u       // optimize(10) needed trials beyond its first batch
};
inline void trace_flag(double* tr, unsigned bits) { tr[kTrFlags] = (double)((unsigned)tr[kTrFlags] | bits); }

}  // namespace ba
}  // namespace rspl

// One bank of linearisation records.  Two alternate: bank[0] is the current set, bank[1] the spare one each
// trial's candidate is linearised into speculatively, which becomes current by a swap when accepted.
struct LinBank {
  double *Hpp, *bp, *Hll, *bl, *Hpl;  // per edge (ba::Lin)
  double *lm_Hll, *lm_bl;             // per landmark (ba::Sys::Hll / bl)
};

struct rspl_ba {
  rspl_ba_config cfg{};
  hipStream_t stream = nullptr;
  rspl::Arena arena;
  int maxE = 0, maxL = 0, maxK = 0, maxV = 0;
  // candidate state (ping-pong partners of the call buffer's T / X / L)
  double *Tb, *Xb, *Lb;
  double* err;      // [E][4] per-edge errors (not banked)
  LinBank bank[2];  // linearisation records: current, spare
  uint8_t* lm_act2;
  // system
  double *bp, *S, *x, *partial, *partial2;
  unsigned* lm_ctr;  // [max_lines] line-landmark tickets (zeroed at create, re-armed by the kernel)
  unsigned long long* prof = nullptr;  // RSPL_BA_PROF: timing trace of one trial per call
  int prof_nb[5] = {0, 0, 0, 0, 0};    // its pair_chunk / update_errors grid sizes, group blocks, nchk, K
  rspl::ba::Active prof_A{};           // the traced trial's chunk geometry (chunk_geo)
  // landmark CSR (filled on the device) and the Schur chunk / pose-pair sums
  double *chunk, *pairfin;
  unsigned* pair_ctr;  // [npairs] chunk tickets (zeroed at create, re-armed by the kernel)
  int *pp_cnt, *pp_off;  // [npairs * nchk (+1)] edge pairs per Schur chunk, segment offsets
  size_t chunk_slots = 0;  // Schur chunks the buffers hold (capacity pose pairs x landmark ranges)
  int4* pp_buf = nullptr;  // edge-pair list {e1, e2, landmark, 0}, growable
  size_t pp_cap = 0;      // capacity in pairs
  // per-call inputs (cameras, T / X / L, edges, reduced pose ids, landmark offsets, pose pairs,
  // zeroed level / fill / flags / out), laid out exactly like the staging buffer's call
  // region: one upload per call (capacity fixed at create).  One per staging slot: the tracking
  // thread uploads the next staged call into its slot's buffer behind the current call's last kernels
  // (preupload_next), so a call's upload is off its own critical path
  char* cbuf[2] = {nullptr, nullptr};
  // pinned, host-mapped staging for uploads; the final kernel writes results straight into it.
  // Two slots: the tracking thread's next queued call is staged into one while the running call
  // reads its results from the other
  char* stage[2] = {nullptr, nullptr};
  char* stage_dev[2] = {nullptr, nullptr};
  size_t stage_cap[2] = {0, 0};
  // host-mapped mailbox
  rspl::ba::Mail* mail = nullptr;
  rspl::ba::Mail* mail_dev = nullptr;
  unsigned long long seq = 0;
  rspl::ba::Stager stg;  // host staging into landmark-CSR order (scratch and host workers reused across calls)
  // landmark sharding (rspl_ba_set_shard): this rank keeps the edges of landmarks g % nranks == rank
  int rank = 0, nranks = 1;
  rspl_allreduce_fn allreduce = nullptr;
  void* ar_ctx = nullptr;
  double* red = nullptr;       // [6 maxK + kMaxRanks + 3] lambda-init / cost all-reduce buffer
  rspl::ba::LmCtrl* lmctl = nullptr;  // device-side LM control (fast path, unsharded)
  double* lm_trace = nullptr;   // RSPL_BA_LMTRACE: per-trial decisions (debug)
  double* gbuf = nullptr;      // final gather buffer (grown on demand)
  size_t gcap = 0;
  double* pdg = nullptr;       // per-block pose-diagonal partials of the first pass (grown on demand)
  size_t pdg_cap = 0;
  // kernel timing (rspl_ba_kernel_timing): HIP events around each device-LM trial's two launches on
  // the BA stream, every ktime_every-th call; totals per launch kind (0: Schur chunks + fused solve,
  // 1: update + speculative linearisation) over the trials that did work
  int ktime_every = 0;
  unsigned long long ncalls = 0;
  bool ktime_on = false;
  std::vector<hipEvent_t> kev;  // 3 per trial
  std::vector<int> kev_eval;    // event-triple indices of the trials that did work (this call)
  int kev_used = 0;
  double kt_ms[2] = {0, 0};
  long long kt_n[2] = {0, 0};
  // native tracking thread (rspl_ba_submit / rspl_ba_join): a FIFO of calls run in order by one host
  // thread of the handle, as the reference's TrackingThread drains _tracking_data_buffer
  struct Job {
    const rspl_ba_problem* pr;
    rspl_ba_result* res;
    std::shared_ptr<rspl::ba::StagedCall> sc;  // its host staging (made by the staging thread)
    int state;                                  // 0 waiting, 1 being staged, 2 staged
  };
  std::thread worker;
  std::thread stager;  // stages the next queued call into the free slot while the worker runs one
  bool slot_busy[2] = {false, false};
  std::mutex qmu;
  std::condition_variable qcv;  // the worker waits for jobs; submitters for room; joiners for idle
  std::deque<Job> jobs;
  bool busy = false, quit = false;
  bool tracking_call = false;  // run_call is running on the tracking thread (preupload_next may look ahead)
  int q_err = 0;                // first failed call since the last join
  std::string q_msg;
  long long q_done = 0, q_iters = 0;
  double q_ms = 0.0;
  // per-call host timeline (rspl_ba_trace): a ring of the last kTraceCap calls, under qmu
  static constexpr int kTraceCap = 4096;
  std::vector<double> trace;  // kTraceCap x RSPL_BA_TRACE_W
  long long trace_n = 0;      // records written since the last read
  unsigned grew = 0;          // device-side buffers grown during the running call (tracking thread)
  int line_jac = 0;           // rspl_ba_set_line_jacobian: 0 g2o's central difference, 1 its analytic limit
  // what the last completed call left on the device, for the test hooks (rspl_ba_debug_pairs / _final): its
  // final state and records, its first optimize's structure (the edge-pair lists were built for it), its
  // CSR -> caller edge map and the T the final kernel wrote into the staging slot
  struct Last {
    bool valid = false, fused = false;
    rspl::ba::Problem P{};
    rspl::ba::Lin L{};
    rspl::ba::Active A{};
    int E = 0;
    const int* gmap = nullptr;
    const double* T_out = nullptr;
  } last;
};

namespace rspl {
namespace ba {

// per-call upload layout (staging call region == device call buffer)
struct CallLayout {
  size_t cams, T, X, L, obs, type, pose, lm, cam, gmap, ginv, lm_pose, pidx, lm_off, lm_act, pairs, ltab, pp_off, level,
      flags, out, bytes;
  CallLayout() = default;
  // nobs: observation doubles (4 / 8 per edge); nchunks: Schur chunks of the window (pp_off)
  CallLayout(int ncam, int np, int nq, int nl, int E, size_t nobs, size_t nchunks) {
    const size_t nL = (size_t)nq + nl;
    size_t so = 0;
    auto place = [&](size_t n) {
      const size_t o = so;
      so = al256(so + n);
      return o;
    };
    cams = place(sizeof(double) * 5 * ncam); T = place(sizeof(double) * 8 * np); X = place(sizeof(double) * 3 * nq);
    L = place(sizeof(double) * 6 * nl); obs = place(sizeof(double) * nobs); type = place(E);
    pose = place(4 * (size_t)E); lm = place(4 * (size_t)E); cam = place(4 * (size_t)E); gmap = place(4 * (size_t)E);
    ginv = place(4 * (size_t)E);  // caller edge id -> CSR position (unsharded calls: the final kernel's flag order)
    lm_pose = place(4 * (size_t)E);
    pidx = place(4 * (size_t)np); lm_off = place(4 * (nL + 1)); lm_act = place(nL);
    pairs = place(8 * (size_t)np * (np + 1) / 2);
    // line-workgroup table (pack_line_blocks) -- sized tight, as the call uploads [0, bytes) in one copy
    const size_t line_edges = nobs >= 4 * (size_t)E ? (nobs - 4 * (size_t)E) / 4 : 0;
    ltab = place(sizeof(int4) * line_blocks_bound((size_t)nl, line_edges));
    // segment offsets of the Schur chunks' edge-pair lists, counted by the staging (ba::pair_offsets)
    pp_off = place(4 * (nchunks + 1));
    level = place(E); flags = place(4 * sizeof(int)); out = place(8 * sizeof(double));  // zeros
    bytes = so;
  }
};

// result layout written by the final kernel into the mapped staging buffer
struct DownLayout {
  size_t inl, T, X, L, bytes;
  DownLayout() = default;
  DownLayout(int np, int nq, int nl, int E) {
    inl = 0; T = al256(E); X = T + al256(sizeof(double) * 8 * np); L = X + al256(sizeof(double) * 3 * nq);
    bytes = L + al256(sizeof(double) * 6 * nl);
  }
};

// RSPL_BA_TIMING=1: host stage times of a call, microseconds since the previous mark, one stderr line
struct HostMarks {
  static bool on() {
    static const bool t = getenv("RSPL_BA_TIMING") != nullptr;
    return t;
  }
  std::chrono::steady_clock::time_point t[16];
  const char* name[16];
  int n = 0;
  void mark(const char* s) {
    if (on() && n < 16) {
      name[n] = s;
      t[n++] = std::chrono::steady_clock::now();
    }
  }
  void print(const char* label) const {
    if (!on()) return;
    fprintf(stderr, "%s", label);
    for (int i = 1; i < n; i++)
      fprintf(stderr, " %s %.1f", name[i], std::chrono::duration<double, std::micro>(t[i] - t[i - 1]).count());
    fprintf(stderr, "\n");
  }
};

// CLOCK_MONOTONIC seconds (Python's time.perf_counter clock): the per-call timeline's time base
inline double mono_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// one call's host staging: its slot and what the device part needs of it
struct StagedCall {
  int slot = 0;
  int rc = RSPL_OK;  // staging failed (argument errors): reported when the call's turn comes
  std::string msg;
  int E = 0, Ep = 0, n_lblk = 0;
  Active G{};              // the window's geometry (plan_window): run_call's Active starts from it
  size_t pair_bound = 0;   // edge pairs the call's lists must hold (pp_staged: the exact total)
  bool pp_staged = false;  // cl.pp_off holds the chunks' segment offsets (ba::pair_offsets)
  CallLayout cl;
  DownLayout dl;
  HostMarks tm;
  double tr[RSPL_BA_TRACE_W] = {};  // its host timeline record (rspl_ba_trace)
  bool uploaded = false;  // its inputs already queued for upload into cbuf[slot] (tracking thread only)
};

// ---- ba.cpp ----
// Staging slot `slot` of at least `bytes` (allocated at create for the handle's capacities: grows only for a
// handle created without them); *grew: it did
int ensure_stage(rspl_ba* b, int slot, size_t bytes, bool* grew = nullptr);
void begin_call(rspl_ba* b);
// after a call: a device-side failure drains the stream and re-arms the cross-call tickets; returns rc
int end_call(rspl_ba* b, int rc);

// A grow-on-demand device buffer of the handle: at least `need` elements, `min_cap` when it grows.  The
// stream may still read the old buffer, so it drains first; grew_bit goes into the call's trace flags.
template <typename T>
int grow_device(rspl_ba* b, T*& buf, size_t& cap, size_t need, size_t min_cap, unsigned grew_bit) {
  if (need <= cap) return RSPL_OK;
  RSPL_HIP(hipStreamSynchronize(b->stream));
  if (buf) (void)hipFree(buf);
  buf = nullptr;
  cap = 0;
  const size_t n = std::max(need, min_cap);
  RSPL_HIP(hipMalloc((void**)&buf, sizeof(T) * n));
  cap = n;
  b->grew |= grew_bit;
  return RSPL_OK;
}

// Spin on the mailbox until accept() takes what it reads there.  Every 4096 spins: surface stream
// errors, give up when the stream has gone idle without posting what accept() waits for (`what`, for
// the message), and bound the wait to 60 s.
template <typename Accept>
int spin_mail(rspl_ba* b, const char* what, Accept&& accept) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  for (unsigned it = 1;; it++) {
    if (accept()) return RSPL_OK;
    if ((it & 4095) == 0) {
      const hipError_t q = hipStreamQuery(b->stream);
      if (q != hipSuccess && q != hipErrorNotReady) {
        set_error("BA stream failed: %s", hipGetErrorString(q));
        return RSPL_E_DEVICE;
      }
      if (q == hipSuccess) {
        if (accept()) return RSPL_OK;
        set_error("BA mailbox: stream idle but %s never posted", what);
        return RSPL_E_DEVICE;
      }
      if (clk::now() - t0 > std::chrono::seconds(60)) {
        set_error("BA mailbox: timed out waiting for %s", what);
        return RSPL_E_DEVICE;
      }
    }
    _mm_pause();
  }
}

// wait until the kernel chain tagged `seq` has posted; v: the four values it posted
inline int wait_mail(rspl_ba* b, unsigned long long seq, double* v) {
  char what[40];
  snprintf(what, sizeof(what), "sequence %llu", seq);
  const int rc = spin_mail(b, what, [&] { return __atomic_load_n(&b->mail->seq, __ATOMIC_ACQUIRE) == seq; });
  if (rc) return rc;
  if (v) {
    volatile const double* mv = b->mail->v;
    for (int k = 0; k < 4; k++) v[k] = mv[k];
  }
  return RSPL_OK;
}

// ---- ba_lm.cpp ----
// the second optimize()'s setup launch queued right behind the first optimize()'s first batch of trials,
// before the host has seen them: a no-op unless that optimize() stopped within the batch (setup_dev's gate);
// then the second optimize() starts from it instead of queueing its own after the host's round trip
struct SpecSetup {
  Active A2{};               // the second optimize()'s active structure (levels, landmark activity)
  uint8_t* level = nullptr;  // where its setup classifies the edges
  int iters2 = 0;
  bool queued = false;  // queued behind a batch of the first optimize()'s trials
  bool extra = false;   // a later batch was queued after it: that setup did nothing (and none followed yet)
  bool topped_up = false;  // the first optimize() needed trials beyond its first batch
};

// the call's final kernel (inlier flags, final T / X / L into the staging slot) queued right behind the
// last optimize()'s trials instead of after the host has seen that optimize() stop: it reads the control
// after the last queued trial and does nothing unless the optimize() stopped there (then the host queues
// top-up trials and another one).  q: the sequence the finish that will post carries.
struct SpecFinish {
  bool on = false;
  Lin L{};
  int E = 0;
  const int* ginv = nullptr;
  uint8_t* inl = nullptr;
  double *Th = nullptr, *Xh = nullptr, *Lh = nullptr;
  unsigned long long q = 0;
};

// what only the device driver reads of an optimize() call
struct DevLmArgs {
  uint8_t* cls_level = nullptr;  // classify the edges into it first (the second optimize's levels)
  bool build_pp = false;         // build the Schur chunks' edge-pair lists (see setup_dev)
  bool pp_staged = false;        // ... against the offsets the staging counted (else counted on the device)
  SpecFinish* fin = nullptr;
  SpecSetup* nxt = nullptr;
  bool setup_done = false;       // its setup already ran from the speculative queue (SpecSetup)
};

// (Lin, Sys) view of one of the handle's banks
inline void view_bank(const LinBank& k, Lin& L, Sys& S) {
  L.Hpp = k.Hpp; L.bp = k.bp; L.Hll = k.Hll; L.bl = k.bl; L.Hpl = k.Hpl;
  S.Hll = k.lm_Hll; S.bl = k.lm_bl;
}
// the device driver takes this optimize() (else the host driver)
bool dev_lm(const rspl_ba* b, const Active& A, int iters);
// one g2o SparseOptimizer::optimize(iters)
int optimize(rspl_ba* b, Problem& P, Lin& Lr, Sys& S, const Active& A, int iters, double* chi2_out, int* done_out,
             const DevLmArgs& d = {});
// the rank's sum all-reduce, stream-ordered on the BA stream
int shard_allreduce(rspl_ba* b, double* d, size_t n);

// ---- ba_call.cpp ----
// Host staging of one call into stage slot `slot`; off_chain: on the staging thread, not on the call's own chain
int stage_call(rspl_ba* b, int slot, const rspl_ba_problem* pr, rspl_ba_result* res, StagedCall& c, bool off_chain);
// the device part of one staged call; tr: its trace record
int run_call(rspl_ba* b, const StagedCall& c, const rspl_ba_problem* pr, rspl_ba_result* res, double* tr);
// the next staged call's upload queued behind the running call's last kernels (tracking thread only)
void preupload_next(rspl_ba* b);
// rspl_ba_local without its begin_call / end_call frame
int local_call(rspl_ba* b, const rspl_ba_problem* pr, rspl_ba_result* res);

// ---- ba_queue.cpp ----
// calls queued on / running in the native tracking thread (rspl_ba_submit) and not yet joined
bool queue_active(rspl_ba* b);
// append one record to the handle's timeline ring (qmu held)
void push_trace(rspl_ba* b, const double* tr);
// an entry point that runs on the BA stream or changes the handle refuses to run beside queued calls
#define RSPL_BA_REFUSE_QUEUED(b, name) \
  RSPL_CHECK_ARG(!::rspl::ba::queue_active(b), name ": calls are queued on the tracking thread (rspl_ba_join first)")

// ---- ba_plan.cpp ----
// The window geometry of an Active from (nL, K) in a handle of chunk_slots chunks: K, npairs, nL and the chunk
// plan (nchk / lmchunk / dsub / lmsub); with update_geometry also ue_bpr (set_update_geometry)
void plan_window(Active& A, int nL, int K, size_t chunk_slots, bool update_geometry);

// ---- ba_debug.cpp ----
// RSPL_BA_PROF: trace the trial about to be queued with S (one per call) and note its grids and chunk
// geometry for report_prof; the caller clears S.prof after the trial's launches
void arm_prof(rspl_ba* b, const Active& A, Sys& S);
void report_prof(rspl_ba* b);          // ... and its stderr lines after the call
void add_kernel_times(rspl_ba* b);     // kernel timing: the call's event triples into the handle's totals
void dump_lm_trace(rspl_ba* b);        // RSPL_BA_LMTRACE: the device LM decisions of both optimize() calls

}  // namespace ba
}  // namespace rspl
