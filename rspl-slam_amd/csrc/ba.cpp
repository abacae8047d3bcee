// Local BA handle: C ABI (include/rspl.h) over the BA kernels (ba_first.hip, ba_schur.hip, ba_trial.hip).
// This file is the handle's life: its arena, staging slots and grow-on-demand buffers, create / destroy, the
// setters and the synchronous call's frame.  The call itself is ba_call.cpp, one optimize() ba_lm.cpp, the
// native tracking thread ba_queue.cpp (ba_handle.hpp lists the host files).
#include <cstring>
#include <type_traits>

#include "ba_handle.hpp"

using namespace rspl;

namespace {

template <typename F>
void carve(F& ar, rspl_ba* b) {
  const size_t E = b->maxE, NL = b->maxL, K = b->maxK, nq = b->cfg.max_points, nl = b->cfg.max_lines;
  auto take = [&](auto*& p, size_t n) {
    using Tp = std::remove_pointer_t<std::remove_reference_t<decltype(p)>>;
    if constexpr (std::is_same_v<F, Arena>) p = ar.template take<Tp>(n ? n : 1);
    else ar.template take<Tp>(n ? n : 1);
  };
  take(b->Tb, K * 8); take(b->Xb, nq * 3); take(b->Lb, nl * 6);
  take(b->err, E * 4);
  for (LinBank& k : b->bank) {
    take(k.Hpp, E * 21); take(k.bp, E * 6); take(k.Hll, E * 16); take(k.bl, E * 4); take(k.Hpl, E * 24);
  }
  take(b->bank[1].lm_Hll, NL * 16); take(b->bank[1].lm_bl, NL * 4);
  take(b->lm_act2, NL);
  take(b->bank[0].lm_Hll, NL * 16); take(b->bank[0].lm_bl, NL * 4); take(b->bp, K * 6);
  // block partials: edge-per-thread kernels (E / 256) and landmark-group kernels (NL * 8 / 256)
  const size_t nblk = std::max(E / 256, NL * 8 / 256) + 2;
  // partial also holds the setup kernel's per-block costs: the landmark groups plus the line
  // workgroups (at most one per line landmark plus one per kLineBlk line edges)
  // (+ 1024: update_errors' XCD-aligned grid rounds the landmark blocks up to whole ranges per XCD)
  take(b->S, 36 * K * K); take(b->x, 6 * K); take(b->partial, nblk + NL + E / ba::kLineBlk + 1032);
  // partial2: scale partials, and the pose-diagonal partials (K x E/256 x 6) of the lambda init
  take(b->partial2, std::max(std::max((size_t)b->maxV / 256, nblk) + 1026, K * (E / 256 + 1) * 6));
  take(b->lm_ctr, nl);
  const size_t npairs = K * (K + 1) / 2, slots = ba::chunk_slots_for((int)NL, (int)K);
  // pair_ctr: + the solve ticket
  take(b->chunk, slots * 48); take(b->pairfin, npairs * 48 + 8); take(b->pair_ctr, npairs + 1);
  take(b->red, 6 * K + ba::kMaxRanks + 8);
  take(b->lmctl, 2);
  take(b->pp_cnt, slots); take(b->pp_off, slots + 1);
  b->chunk_slots = slots;
}

}  // namespace

namespace rspl {
namespace ba {

// Staging slots are allocated at create for the handle's capacities (stage_bytes), so in use this never
// grows; it stays for a handle created without them.  The slot being grown is not in use (a slot is
// handed out only when its previous call has finished), so the new buffer is taken before the old one
// is released and nothing waits for the stream.
int ensure_stage(rspl_ba* b, int slot, size_t bytes, bool* grew) {
  if (bytes <= b->stage_cap[slot]) return RSPL_OK;
  const size_t cap = std::max(bytes, b->stage_cap[slot] * 2);
  char *nh = nullptr, *nd = nullptr;
  RSPL_HIP(hipHostMalloc((void**)&nh, cap, hipHostMallocMapped | hipHostMallocCoherent));
  if (hipHostGetDevicePointer((void**)&nd, nh, 0) != hipSuccess) {
    (void)hipHostFree(nh);
    set_error("BA staging slot: no device mapping");
    return RSPL_E_DEVICE;
  }
  if (b->stage[slot]) (void)hipHostFree(b->stage[slot]);
  b->stage[slot] = nh;
  b->stage_dev[slot] = nd;
  b->stage_cap[slot] = cap;
  if (grew) *grew = true;
  return RSPL_OK;
}

void begin_call(rspl_ba* b) {
  b->ktime_on = b->ktime_every > 0 && b->ncalls++ % (unsigned long long)b->ktime_every == 0;
  b->kev_used = 0;
  b->kev_eval.clear();
}

// A device-side failure can return while the call's kernel chain is still queued or running (a
// mailbox timeout, a failed all-reduce): drain the stream before anything of the handle is reused
// (the next call restages the mapped buffers the old chain reads) and re-arm the cross-call
// tickets and release flags the chain may have left half-counted.  If the drain itself fails the
// device is gone and the handle must be recreated (the error says so).
int end_call(rspl_ba* b, int rc) {
  if (rc != RSPL_E_DEVICE) return rc;
  const std::string msg = rspl_last_error();
  if (hipStreamSynchronize(b->stream) != hipSuccess ||
      hipMemset(b->lm_ctr, 0, sizeof(unsigned) * std::max(b->cfg.max_lines, 1)) != hipSuccess ||
      hipMemset(b->pair_ctr, 0, sizeof(unsigned) * (b->maxK * (b->maxK + 1) / 2 + 1)) != hipSuccess) {
    set_error("%s; the BA stream could not be drained: recreate the handle", msg.c_str());
    return rc;
  }
  set_error("%s", msg.c_str());
  return rc;
}

}  // namespace ba
}  // namespace rspl

extern "C" int rspl_ba_create(const rspl_ba_config* cfg, rspl_ba** out) {
  RSPL_CHECK_ARG(cfg && out, "rspl_ba_create: NULL argument");
  RSPL_CHECK_ARG(cfg->max_poses > 0 && cfg->max_poses <= 64 && cfg->max_points >= 0 && cfg->max_lines >= 0 &&
                     cfg->max_edges >= 0,
                 "capacities: 1 <= max_poses <= 64, others >= 0");
  *out = nullptr;
  RSPL_HIP(hipSetDevice(cfg->device));
  auto* b = new rspl_ba();
  b->cfg = *cfg;
  b->maxE = 4 * cfg->max_edges;
  b->maxL = cfg->max_points + cfg->max_lines;
  b->maxK = cfg->max_poses;
  b->maxV = cfg->max_poses + cfg->max_points + cfg->max_lines;
  Sizer sz;
  carve(sz, b);
  int rc = b->arena.reserve(sz.used);
  if (rc) { delete b; return rc; }
  carve(b->arena, b);
  // the BA is a host-driven chain of short kernels on the tracking thread's critical path:
  // give its stream the highest priority so each trial's kernels dispatch ahead of queued
  // SuperPoint/SuperGlue work instead of waiting behind it
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  // the largest call's upload: the call buffers' and (with the results') the staging slots' size
  const size_t cbytes = ba::CallLayout(ba::kMaxCams, b->maxK, cfg->max_points, cfg->max_lines, b->maxE,
                                       8 * (size_t)b->maxE, b->chunk_slots).bytes;
  {
    const char* what = nullptr;
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r, const char* w) {
      if (e == hipSuccess && r != hipSuccess) {
        e = r;
        what = w;
      }
    };
    step(hipStreamCreateWithPriority(&b->stream, hipStreamNonBlocking, prio_hi), "hipStreamCreateWithPriority");
    if (e == hipSuccess)
      step(hipHostMalloc((void**)&b->mail, sizeof(ba::Mail), hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc(mailbox)");
    if (e == hipSuccess) step(hipHostGetDevicePointer((void**)&b->mail_dev, b->mail, 0), "hipHostGetDevicePointer(mailbox)");
    for (int i = 0; i < 2 && e == hipSuccess; i++) step(hipMalloc((void**)&b->cbuf[i], cbytes), "hipMalloc(call buffer)");
    if (e == hipSuccess) step(hipMemset(b->lm_ctr, 0, sizeof(unsigned) * std::max(b->cfg.max_lines, 1)), "hipMemset(lm_ctr)");
    if (e == hipSuccess)
      step(hipMemset(b->pair_ctr, 0, sizeof(unsigned) * (b->maxK * (b->maxK + 1) / 2 + 1)), "hipMemset(pair_ctr)");
    if (e != hipSuccess) {
      set_error("BA stream / mailbox allocation failed: %s: %s (call buffer %zu bytes, arena %zu bytes)", what,
                hipGetErrorString(e), cbytes, b->arena.size);
      rspl_ba_destroy(b);
      return RSPL_E_DEVICE;
    }
  }
  memset(b->mail, 0, sizeof(ba::Mail));
  // everything a call can need, allocated once here for the handle's capacities (never inside a call:
  // a pinned allocation or a hipFree there stalls the device and the pipeline beside it): both staging
  // slots, the pose-diagonal partials of the first pass and the edge-pair lists (sum over landmarks of
  // k^2 edge pairs, k = edges of the landmark; sized for 8 edges per landmark on average -- beyond that
  // the list still grows on demand, flagged in the call's trace record)
  {
    const size_t sb = std::max(cbytes, ba::DownLayout(b->maxK, cfg->max_points, cfg->max_lines, b->maxE).bytes);
    ba::Active Amax{};  // the largest call: every landmark, the most line workgroups
    Amax.nL = b->maxL;
    Amax.K = b->maxK;
    Amax.n_lblk = (int)ba::line_blocks_bound((size_t)cfg->max_lines, (size_t)b->maxE);
    const size_t pdg = (size_t)ba::setup_pdg_len(Amax);
    const size_t pp = std::max<size_t>((size_t)1 << 16, 8 * (size_t)b->maxE);
    if (ba::ensure_stage(b, 0, sb) || ba::ensure_stage(b, 1, sb) ||
        hipMalloc((void**)&b->pdg, sizeof(double) * pdg) != hipSuccess ||
        hipMalloc((void**)&b->pp_buf, sizeof(int4) * pp) != hipSuccess) {
      set_error("BA staging / scratch allocation failed");
      rspl_ba_destroy(b);
      return RSPL_E_DEVICE;
    }
    b->pdg_cap = pdg;
    b->pp_cap = pp;
  }
  b->trace.assign((size_t)rspl_ba::kTraceCap * RSPL_BA_TRACE_W, 0.0);
  if (getenv("RSPL_BA_PROF") &&
      (hipMalloc((void**)&b->prof, sizeof(unsigned long long) * ba::kProfLen) != hipSuccess ||
       hipMemset(b->prof, 0, sizeof(unsigned long long) * ba::kProfLen) != hipSuccess)) {
    set_error("BA trace allocation failed");
    rspl_ba_destroy(b);
    return RSPL_E_DEVICE;
  }
  *out = b;
  return RSPL_OK;
}

extern "C" int rspl_ba_use_reserved_cus(rspl_ba* b, int reserve_cus) {
  RSPL_CHECK_ARG(b, "rspl_ba_use_reserved_cus: NULL handle");
  hipStream_t ns = nullptr;
  if (reserve_cus > 0) {
    std::vector<uint32_t> mask;
    int rc = cu_mask(reserve_cus, true, mask);
    if (rc) return rc;
    RSPL_HIP(hipExtStreamCreateWithCUMask(&ns, (uint32_t)mask.size(), mask.data()));
  } else {
    int lo = 0, hi = 0;
    RSPL_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    RSPL_HIP(hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, hi));
  }
  RSPL_HIP(hipStreamSynchronize(b->stream));
  RSPL_HIP(hipStreamDestroy(b->stream));
  b->stream = ns;
  return RSPL_OK;
}

extern "C" int rspl_ba_set_shard(rspl_ba* b, int rank, int nranks, rspl_allreduce_fn fn, void* ctx) {
  RSPL_CHECK_ARG(b, "rspl_ba_set_shard: NULL handle");
  RSPL_BA_REFUSE_QUEUED(b, "rspl_ba_set_shard");
  RSPL_CHECK_ARG(nranks >= 1 && nranks <= ba::kMaxRanks && rank >= 0 && rank < nranks, "rank %d of %d (1..%d ranks)",
                 rank, nranks, ba::kMaxRanks);
  RSPL_CHECK_ARG(nranks == 1 || fn, "an all-reduce function is required for nranks > 1");
  // with fn the sharded schedule runs even for one rank (every all-reduce an identity): the
  // collective path can be exercised on a single GPU; fn == NULL with one rank = unsharded
  b->rank = rank;
  b->nranks = nranks;
  b->allreduce = fn;
  b->ar_ctx = ctx;
  return RSPL_OK;
}

extern "C" int rspl_ba_set_line_jacobian(rspl_ba* b, int analytic) {
  RSPL_CHECK_ARG(b && (analytic == 0 || analytic == 1), "rspl_ba_set_line_jacobian: NULL handle or mode not 0 / 1");
  RSPL_BA_REFUSE_QUEUED(b, "rspl_ba_set_line_jacobian");
  b->line_jac = analytic;
  return RSPL_OK;
}

extern "C" void rspl_ba_destroy(rspl_ba* b) {
  if (!b) return;
  if (b->worker.joinable()) {  // finish the queued calls, then stop the tracking thread
    {
      std::lock_guard<std::mutex> lk(b->qmu);
      b->quit = true;
    }
    b->qcv.notify_all();
    b->worker.join();
    b->stager.join();
  }
  for (hipEvent_t e : b->kev) (void)hipEventDestroy(e);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->gbuf) (void)hipFree(b->gbuf);
  if (b->pdg) (void)hipFree(b->pdg);
  b->arena.release();
  for (char* cb : b->cbuf)
    if (cb) (void)hipFree(cb);
  if (b->pp_buf) (void)hipFree(b->pp_buf);
  if (b->prof) (void)hipFree(b->prof);
  for (char* sg : b->stage)
    if (sg) (void)hipHostFree(sg);
  if (b->mail) (void)hipHostFree(b->mail);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

extern "C" int rspl_ba_local(rspl_ba* b, const rspl_ba_problem* pr, rspl_ba_result* res) {
  if (!b) return ba::local_call(b, pr, res);
  // the synchronous call stages into slot 0 and runs on the BA stream: never beside queued calls
  RSPL_BA_REFUSE_QUEUED(b, "rspl_ba_local");
  ba::begin_call(b);
  return ba::end_call(b, ba::local_call(b, pr, res));
}
