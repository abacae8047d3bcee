// Local BA: the native tracking thread (rspl_ba_submit / rspl_ba_join) and the per-call trace ring.
// Two host threads per handle: the staging thread stages each queued call (validation, landmark-CSR
// scatter, tables: host work only) into a free staging slot as soon as it is queued; the tracking
// thread runs the staged calls on the device in order.  The next call's staging therefore overlaps
// the current call's LM trials instead of preceding them on the tracking thread's critical path; the
// calls still run one at a time and in submission order, each on the inputs given at submission.
#include "ba_handle.hpp"

using namespace rspl;

namespace {
constexpr size_t kTrackingBuffer = 2;  // map_builder.cc:176: the feature thread waits while 2 are queued

void staging_loop(rspl_ba* b) {
  (void)hipSetDevice(b->cfg.device);
  std::unique_lock<std::mutex> lk(b->qmu);
  for (;;) {
    rspl_ba::Job* j = nullptr;
    int slot = -1;
    b->qcv.wait(lk, [&] {
      j = nullptr;
      for (rspl_ba::Job& q : b->jobs)
        if (q.state == 0) {
          j = &q;
          break;
        }
      slot = !b->slot_busy[0] ? 0 : !b->slot_busy[1] ? 1 : -1;
      return (j && slot >= 0) || (b->quit && !j);
    });
    if (!j) return;  // quit with every queued call staged
    j->state = 1;    // (deque elements stay in place while others are pushed; j is popped only when staged)
    b->slot_busy[slot] = true;
    const std::shared_ptr<ba::StagedCall> sc = j->sc;
    const rspl_ba_problem* pr = j->pr;
    rspl_ba_result* res = j->res;
    lk.unlock();
    sc->slot = slot;
    sc->tr[ba::kTrStageBegin] = ba::mono_s();
    sc->rc = ba::stage_call(b, slot, pr, res, *sc, true);
    sc->tr[ba::kTrStageEnd] = ba::mono_s();
    sc->tr[ba::kTrSlot] = slot;
    if (sc->rc) sc->msg = rspl_last_error();
    lk.lock();
    j->state = 2;
    b->qcv.notify_all();  // the tracking thread may be waiting for it
  }
}

void tracking_loop(rspl_ba* b) {
  (void)hipSetDevice(b->cfg.device);
  std::unique_lock<std::mutex> lk(b->qmu);
  for (;;) {
    b->qcv.wait(lk, [&] { return (!b->jobs.empty() && b->jobs.front().state == 2) || (b->quit && b->jobs.empty()); });
    if (b->jobs.empty()) return;  // quit with nothing left
    const rspl_ba::Job j = b->jobs.front();
    b->jobs.pop_front();
    b->busy = true;
    lk.unlock();
    b->qcv.notify_all();  // room for a submitter
    const auto t0 = std::chrono::steady_clock::now();
    j.sc->tr[ba::kTrRunBegin] = ba::mono_s();
    int rc;
    if (j.sc->rc) {
      set_error("%s", j.sc->msg.c_str());
      rc = j.sc->rc;
    } else {
      ba::begin_call(b);
      b->tracking_call = true;
      rc = ba::end_call(b, ba::run_call(b, *j.sc, j.pr, j.res, j.sc->tr));
      b->tracking_call = false;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const std::string msg = rc ? std::string(rspl_last_error()) : std::string();
    lk.lock();
    b->slot_busy[j.sc->slot] = false;
    b->busy = false;
    b->q_done++;
    b->q_ms += ms;
    if (!rc) ba::push_trace(b, j.sc->tr);
    if (!rc) b->q_iters += j.res->iterations_done_first + j.res->iterations_done_second;
    if (rc && !b->q_err) {
      b->q_err = rc;
      b->q_msg = msg;
    }
    b->qcv.notify_all();  // a joiner may be waiting for idle; the staging thread for a free slot
  }
}
}  // namespace

namespace rspl {
namespace ba {

bool queue_active(rspl_ba* b) {
  std::lock_guard<std::mutex> lk(b->qmu);
  return !b->jobs.empty() || b->busy;
}

void push_trace(rspl_ba* b, const double* tr) {
  if (b->trace.empty()) return;
  const size_t i = (size_t)(b->trace_n++ % rspl_ba::kTraceCap);
  std::copy(tr, tr + RSPL_BA_TRACE_W, b->trace.begin() + i * RSPL_BA_TRACE_W);
}

}  // namespace ba
}  // namespace rspl

extern "C" int rspl_ba_submit(rspl_ba* b, const rspl_ba_problem* pr, rspl_ba_result* res) {
  RSPL_CHECK_ARG(b && pr && res, "rspl_ba_submit: NULL argument");
  std::unique_lock<std::mutex> lk(b->qmu);
  if (!b->worker.joinable()) {
    b->worker = std::thread(tracking_loop, b);
    b->stager = std::thread(staging_loop, b);
  }
  const double t_sub = ba::mono_s();
  b->qcv.wait(lk, [&] { return b->jobs.size() < kTrackingBuffer; });
  b->jobs.push_back({pr, res, std::make_shared<ba::StagedCall>(), 0});
  b->jobs.back().sc->tr[ba::kTrSubmitted] = t_sub;
  lk.unlock();
  b->qcv.notify_all();
  return RSPL_OK;
}

extern "C" int rspl_ba_join(rspl_ba* b, long long* calls, long long* iterations, double* ms) {
  RSPL_CHECK_ARG(b, "rspl_ba_join: NULL handle");
  std::unique_lock<std::mutex> lk(b->qmu);
  b->qcv.wait(lk, [&] { return b->jobs.empty() && !b->busy; });
  if (calls) *calls = b->q_done;
  if (iterations) *iterations = b->q_iters;
  if (ms) *ms = b->q_ms;
  b->q_done = b->q_iters = 0;
  b->q_ms = 0.0;
  const int rc = b->q_err;
  if (rc) set_error("%s", b->q_msg.c_str());
  b->q_err = 0;
  b->q_msg.clear();
  return rc;
}

extern "C" int rspl_ba_trace(rspl_ba* b, double* out, int cap, int* n) {
  RSPL_CHECK_ARG(b && n && cap >= 0 && (out || cap == 0), "rspl_ba_trace: NULL argument or cap < 0");
  std::lock_guard<std::mutex> lk(b->qmu);
  const long long have = std::min<long long>(b->trace_n, rspl_ba::kTraceCap);
  const long long first = b->trace_n - have;  // oldest record still in the ring
  const int m = (int)std::min<long long>(have, cap);
  for (int i = 0; i < m; i++) {
    const size_t r = (size_t)((first + i) % rspl_ba::kTraceCap);
    std::copy(b->trace.begin() + r * RSPL_BA_TRACE_W, b->trace.begin() + (r + 1) * RSPL_BA_TRACE_W,
              out + (size_t)i * RSPL_BA_TRACE_W);
  }
  *n = m;
  b->trace_n = 0;
  return RSPL_OK;
}
