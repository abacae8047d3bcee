// The line detectors of the rspl_lines handle, the asynchronous LineExtractor worker and
// the detector's debug hooks.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "common.hpp"
#include "fld_host.hpp"
#include "fld_kernels.hpp"
#include "line_kernels.hpp"
#include "lines_handle.hpp"

#pragma clang fp contract(off)

using namespace rspl;

// ---------------------------------------------------------------------------------------------
// LineDetector's detector: cv::resize(0.5, INTER_LINEAR) + fld->detect (line_processor.cc:455-466,
// FastLineDetector with do_merge false), restated as oracle/fld_ref.py.  The pixel-parallel front
// (resize, Sobel, Canny's non-maximum suppression and thresholds) runs on the GPU
// (line_kernels.hip canny_kernel).  The order-dependent rest runs either on the host
// (fld_host.hpp: hysteresis, the corner zeroing, then chains, runs, filters and orientation) or on
// the device (fld_kernels.hip); both compile the arithmetic of fld_device.hpp and equal the
// restatement bit for bit (FP contraction is off in this file too).
// ---------------------------------------------------------------------------------------------
namespace {

// what both detectors ask of an image, its half image and a config; the device path's own bounds follow below
int fld_check_image(int H, int W, size_t stride) {
  RSPL_CHECK_ARG(H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0, "image %dx%d: even sizes >= 4 required", W, H);
  RSPL_CHECK_ARG(stride >= (size_t)W && stride <= (size_t)INT32_MAX, "stride %zu below the width %d (or beyond int)",
                 stride, W);
  return RSPL_OK;
}

int fld_check_half(int hh, int hw) {  // a chain's points are packed as 16 + 16 bits
  RSPL_CHECK_ARG(hh >= 2 && hw >= 2 && hh < 65536 && hw < 65536, "half image %dx%d outside [2, 65535]", hw, hh);
  return RSPL_OK;
}

int fld_check_cfg(const rspl_fld_config* cfg) {
  RSPL_CHECK_ARG(cfg, "NULL rspl_fld_config");
  RSPL_CHECK_ARG(cfg->canny_aperture_size == 3, "canny_aperture_size %d: only 3 (the configs' value)",
                 cfg->canny_aperture_size);
  RSPL_CHECK_ARG(cfg->length_threshold >= 1 && cfg->distance_threshold >= 0, "bad FLD thresholds");
  return RSPL_OK;
}

// the device path's own bounds: the component sort's 15-bit indices and the LDS budget of the two bitmasks
int fld_check_cfg_device(const rspl_fld_config* cfg) {
  if (int rc = fld_check_cfg(cfg)) return rc;
  RSPL_CHECK_ARG(cfg->length_threshold < fld::kMaxEdge, "bad FLD thresholds");
  return RSPL_OK;
}

int fld_check_mask(int hh, int hw) {
  if (int rc = fld_check_half(hh, hw)) return rc;
  RSPL_CHECK_ARG(fld::mask_fits(hh, hw),
                 "half image %dx%d: its two bitmasks (rows * ceil(width / 32) * 8 = %lld bytes) exceed the %d-byte LDS "
                 "budget", hw, hh, (long long)hh * fld::words_per_row(hw) * 8, fld::kMaskLdsBytes);
  return RSPL_OK;
}

// cv::Canny's argument handling (the thresholds swapped into order and floored) for one image
lines::CannyArgs canny_args(const rspl_fld_config* cfg, const uint8_t* image, int H, int W, int stride, uint8_t* half,
                            uint8_t* cls) {
  double lo = cfg->canny_th1, hi = cfg->canny_th2;
  if (lo > hi) std::swap(lo, hi);
  lines::CannyArgs a{};
  a.img = image; a.H = H; a.W = W; a.stride = stride;
  a.half = half; a.cls = cls;
  a.low = (int)std::floor(lo); a.high = (int)std::floor(hi);
  return a;
}

// the host detector's second piece and its count past capacity, for the three entries that run it
int segments_out(const uint8_t* half, uint8_t* edges, int hh, int hw, const rspl_fld_config* cfg,
                 std::vector<uint32_t>& pts, float* segments, int capacity, int* n_out) {
  const int n = fld::segments_from_edges(half, edges, hh, hw, cfg->length_threshold, cfg->distance_threshold, pts,
                                         segments, capacity);
  *n_out = n;
  if (n > capacity) {
    set_error("%d segments exceed capacity %d", n, capacity);
    return RSPL_E_CAPACITY;
  }
  return RSPL_OK;
}

}  // namespace

extern "C" int rspl_lines_detect(rspl_lines* h, const uint8_t* image, int H, int W, int stride,
                                 const rspl_fld_config* cfg, float* segments, int capacity, int* n_out) {
  RSPL_CHECK_ARG(h && image && cfg && n_out && (segments || capacity == 0), "rspl_lines_detect: NULL argument");
  if (int rc = fld_check_image(H, W, (size_t)stride)) return rc;
  if (int rc = fld_check_half(H / 2, W / 2)) return rc;
  if (int rc = fld_check_cfg(cfg)) return rc;
  *n_out = 0;
  const size_t px = (size_t)H * W, hp = px / 4;
  const int hh = H / 2, hw = W / 2;
  if (px > h->det_cap) {  // grow the detector buffers (the stream is idle between calls)
    RSPL_HIP(hipStreamSynchronize(h->stream));
    if (h->d_img) (void)hipFree(h->d_img);
    if (h->d_det) (void)hipFree(h->d_det);
    if (h->h_img) (void)hipHostFree(h->h_img);
    if (h->h_det) (void)hipHostFree(h->h_det);
    h->d_img = h->d_det = h->h_img = h->h_det = nullptr;
    h->det_cap = 0;
    RSPL_HIP(hipMalloc((void**)&h->d_img, px));
    RSPL_HIP(hipMalloc((void**)&h->d_det, 2 * (px / 4)));
    RSPL_HIP(hipHostMalloc((void**)&h->h_img, px));
    RSPL_HIP(hipHostMalloc((void**)&h->h_det, 2 * (px / 4)));
    h->det_cap = px;
  }
  const auto tp0 = std::chrono::steady_clock::now();
  for (int r = 0; r < H; r++) memcpy(h->h_img + (size_t)r * W, image + (size_t)r * stride, W);
  const auto tp1 = std::chrono::steady_clock::now();
  hipStream_t st = h->stream;
  RSPL_HIP(hipMemcpyAsync(h->d_img, h->h_img, px, hipMemcpyHostToDevice, st));
  RSPL_HIP(lines::canny_classes(canny_args(cfg, h->d_img, H, W, W, h->d_det, h->d_det + hp), st));
  RSPL_HIP(hipMemcpyAsync(h->h_det, h->d_det, 2 * hp, hipMemcpyDeviceToHost, st));
  RSPL_HIP(hipStreamSynchronize(st));
  const auto tp2 = std::chrono::steady_clock::now();
  h->det_H = H;
  h->det_W = W;
  fld::HostScratch& s = h->fld_host;
  fld::edges_from_classes(h->h_det + hp, hh, hw, s);
  const int rc = segments_out(h->h_det, s.edge.data(), hh, hw, cfg, s.pts, segments, capacity, n_out);
  const auto tp3 = std::chrono::steady_clock::now();
  auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
  h->ph_us[0] = us(tp0, tp1);
  h->ph_us[1] = us(tp1, tp2);
  h->ph_us[2] = us(tp2, tp3);
  return rc;
}

// the host detector without a handle or a device: from an edge map (after hysteresis and the corner zeroing),
// and from a class map as rspl_lines_detect gets it back from the Canny kernel
extern "C" int rspl_lines_debug_fld_host(const uint8_t* half, const uint8_t* edges, int hh, int hw,
                                         const rspl_fld_config* cfg, float* segments, int capacity, int* n_out) {
  if (int rc = fld_check_half(hh, hw)) return rc;
  if (int rc = fld_check_cfg_device(cfg)) return rc;  // as the device path it was written to mirror
  RSPL_CHECK_ARG(half && edges && n_out && capacity >= 0 && (capacity == 0 || segments),
                 "rspl_lines_debug_fld_host: bad argument");
  std::vector<uint8_t> e(edges, edges + (size_t)hh * hw);  // the walk consumes its edge map
  std::vector<uint32_t> pts;
  return segments_out(half, e.data(), hh, hw, cfg, pts, segments, capacity, n_out);
}

extern "C" int rspl_lines_debug_fld_classes(const uint8_t* half, const uint8_t* cls, int hh, int hw,
                                            const rspl_fld_config* cfg, float* segments, int capacity, int* n_out) {
  if (int rc = fld_check_half(hh, hw)) return rc;
  if (int rc = fld_check_cfg(cfg)) return rc;
  RSPL_CHECK_ARG(half && cls && n_out && capacity >= 0 && (capacity == 0 || segments),
                 "rspl_lines_debug_fld_classes: bad argument");
  fld::HostScratch s;
  fld::edges_from_classes(cls, hh, hw, s);
  return segments_out(half, s.edge.data(), hh, hw, cfg, s.pts, segments, capacity, n_out);
}

extern "C" int rspl_lines_debug_canny(rspl_lines* h, int H, int W, uint8_t* half, uint8_t* cls) {
  RSPL_CHECK_ARG(h && half && cls, "rspl_lines_debug_canny: NULL argument");
  RSPL_CHECK_ARG(H == h->det_H && W == h->det_W && H > 0,
                 "rspl_lines_debug_canny: %dx%d is not the last detection's size (%dx%d)", W, H, h->det_W, h->det_H);
  const size_t hp = (size_t)H * W / 4;
  memcpy(half, h->h_det, hp);
  memcpy(cls, h->h_det + hp, hp);
  return RSPL_OK;
}


namespace {

void extract_job_device(rspl_lines* h);

// the worker's job: rspl_lines_detect into a growing segment buffer, then rspl_line_extract
void extract_job(rspl_lines* h) {
  if (h->a_dev) return extract_job_device(h);
  const auto t0 = std::chrono::steady_clock::now();
  int n = 0, rc;
  for (;;) {
    if (h->a_seg.size() < 4096) h->a_seg.resize(4096 * 4);
    const int cap = (int)(h->a_seg.size() / 4);
    rc = rspl_lines_detect(h, h->a_img, h->a_H, h->a_W, h->a_stride, &h->a_cfg, h->a_seg.data(), cap, &n);
    if (rc != RSPL_E_CAPACITY || n <= cap) break;
    h->a_seg.resize((size_t)n * 4);
  }
  h->a_n = 0;
  if (rc == RSPL_OK) {
    h->a_lines.resize((size_t)std::max(n, 1) * 4);  // the merges never add lines
    rc = rspl_line_extract(h->a_seg.data(), n, h->a_merge, h->a_lines.data(), std::max(n, 1), &h->a_n);
  }
  h->a_rc = rc;
  h->a_err = rc == RSPL_OK ? std::string() : std::string(rspl_last_error());
  h->a_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  static const bool timing = getenv("RSPL_LINES_TIMING") != nullptr;  // diagnostics
  if (timing)
    fprintf(stderr, "lines_job us: stage %.1f gpu %.1f fld %.1f merge+rest %.1f total %.1f segs %d lines %d\n", h->ph_us[0],
            h->ph_us[1], h->ph_us[2], h->a_us - h->ph_us[0] - h->ph_us[1] - h->ph_us[2], h->a_us, n, h->a_n);
}

void ensure_worker(rspl_lines* h) {
  if (h->worker.joinable()) return;
  const int dev = h->cfg.device;
  h->worker = std::thread([h, dev]() {
    (void)hipSetDevice(dev);  // the HIP device is per thread
    std::unique_lock<std::mutex> lk(h->mu);
    for (;;) {
      h->cv.wait(lk, [h] { return h->quit || (h->job && !h->done); });
      if (h->quit) return;
      lk.unlock();
      extract_job(h);
      lk.lock();
      h->done = true;
      h->cv.notify_all();
    }
  });
}

}  // namespace

extern "C" int rspl_lines_extract_async(rspl_lines* h, const uint8_t* image, int H, int W, int stride,
                                        const rspl_fld_config* cfg, int do_merge) {
  RSPL_CHECK_ARG(h && image && cfg, "rspl_lines_extract_async: NULL argument");
  {
    std::lock_guard<std::mutex> lk(h->mu);
    RSPL_CHECK_ARG(!h->job, "rspl_lines_extract_async: the previous job has not been waited for");
    h->a_img = image;
    h->a_H = H;
    h->a_W = W;
    h->a_stride = stride;
    h->a_cfg = *cfg;
    h->a_merge = do_merge;
    h->a_dev = false;
    h->job = true;
    h->done = false;
  }
  ensure_worker(h);
  h->cv.notify_all();
  return RSPL_OK;
}

extern "C" int rspl_lines_extract_wait(rspl_lines* h, double* lines, int capacity, int* n_out, double* job_us) {
  RSPL_CHECK_ARG(h && n_out && (capacity == 0 || lines) && capacity >= 0, "rspl_lines_extract_wait: bad argument");
  std::unique_lock<std::mutex> lk(h->mu);
  RSPL_CHECK_ARG(h->job, "rspl_lines_extract_wait: no job submitted");
  h->cv.wait(lk, [h] { return h->done; });
  h->job = false;
  *n_out = h->a_n;
  if (job_us) *job_us = h->a_us;
  if (h->a_rc != RSPL_OK) {
    set_error("%s", h->a_err.c_str());
    return h->a_rc;
  }
  if (h->a_n > capacity) {
    set_error("%d lines exceed capacity %d", h->a_n, capacity);
    return RSPL_E_CAPACITY;
  }
  if (h->a_n) memcpy(lines, h->a_lines.data(), sizeof(double) * 4 * h->a_n);
  return RSPL_OK;
}

extern "C" int rspl_lines_extract_wait_device(rspl_lines* h, double* d_lines, int capacity, int* n_out,
                                              double* job_us, void* stream) {
  RSPL_CHECK_ARG(h && n_out && (capacity == 0 || d_lines) && capacity >= 0,
                 "rspl_lines_extract_wait_device: bad argument");
  constexpr int S = rspl_lines::kPinSlots;
  if (h->pin_cap < capacity) {  // grow every slot (their pending copies drained first)
    for (int k = 0; k < S; k++) {
      if (h->copy_pending[k]) RSPL_HIP(hipEventSynchronize(h->copy_ev[k]));
      h->copy_pending[k] = false;
      if (h->pin_lines[k]) (void)hipHostFree(h->pin_lines[k]);
      h->pin_lines[k] = nullptr;
    }
    h->pin_cap = 0;
    for (int k = 0; k < S; k++)
      RSPL_HIP(hipHostMalloc((void**)&h->pin_lines[k], sizeof(double) * 4 * capacity, hipHostMallocDefault));
    h->pin_cap = capacity;
  }
  const int k = h->pin_next;
  if (!h->copy_ev[k]) RSPL_HIP(hipEventCreateWithFlags(&h->copy_ev[k], kOrderEventFlags));
  if (h->copy_pending[k]) {  // this slot's copy S joins ago
    RSPL_HIP(hipEventSynchronize(h->copy_ev[k]));
    h->copy_pending[k] = false;
  }
  int rc = rspl_lines_extract_wait(h, h->pin_lines[k], capacity, n_out, job_us);
  if (rc != RSPL_OK) return rc;
  if (*n_out) {
    RSPL_HIP(hipMemcpyAsync(d_lines, h->pin_lines[k], sizeof(double) * 4 * *n_out, hipMemcpyHostToDevice,
                            (hipStream_t)stream));
    RSPL_HIP(hipEventRecord(h->copy_ev[k], (hipStream_t)stream));
    h->copy_pending[k] = true;
    h->pin_next = (k + 1) % S;
  }
  return RSPL_OK;
}

// ---------------------------------------------------------------------------------------------
// The detector on the device (fld_kernels.hip): the Canny classes as above, then hysteresis,
// component labels, the chain walk, the segment fit and the (seed, k) order as stream-ordered
// launches -- device image in, device segments and count out, no host wait.
// ---------------------------------------------------------------------------------------------
namespace {

// what rspl_lines_detect_device refuses before any device call
int fld_check_images(int batch, int H, int W, size_t stride, size_t pitch, const rspl_fld_config* cfg) {
  RSPL_CHECK_ARG(batch >= 1 && batch <= fld::kMaxBatch, "batch %d outside [1, %d]", batch, fld::kMaxBatch);
  if (int rc = fld_check_image(H, W, stride)) return rc;
  RSPL_CHECK_ARG(pitch >= stride * (size_t)(H - 1) + (size_t)W, "pitch %zu below one %dx%d image of stride %zu", pitch, W,
                 H, stride);
  if (int rc = fld_check_mask(H / 2, W / 2)) return rc;
  return fld_check_cfg_device(cfg);
}

// the scratch of fld::kMaxBatch images; the first call (and a larger image) allocates, which is the one time the
// call is not purely stream-ordered
int fld_reserve(rspl_lines* h, size_t hp) {
  constexpr size_t B = fld::kMaxBatch, E = fld::kMaxEdge, S = fld::kMaxSeg;
  if (!h->fld_arena.base) {
    const size_t words = fld::kMaskLdsBytes / 8;
    const size_t bytes = B * (words * 4 + E * 4 * 5 + 4 + E * 12 + S * 8 + S * 16 + fld::kMetaInts * 4) +
                         rspl_lines::kDevSegCap * 16 + B * 4 + 16 * 256;
    if (int rc = h->fld_arena.reserve(bytes)) return rc;
    Arena& ar = h->fld_arena;
    fld::Args& a = h->fld;
    a.ebits = ar.take<uint32_t>(B * words);
    a.pix = ar.take<int>(B * E);
    a.lab = ar.take<int>(B * E);
    a.spix = ar.take<int>(B * E);
    a.cstart = ar.take<int>(B * (E + 1));
    a.pts = ar.take<uint32_t>(B * E);
    a.chains = ar.take<int>(B * E * 3);
    a.skey = ar.take<unsigned long long>(B * S);
    a.sseg = ar.take<float>(B * S * 4);
    a.meta = ar.take<int>(B * fld::kMetaInts);
    h->dev_seg = ar.take<float>((size_t)rspl_lines::kDevSegCap * 4);
    h->dev_cnt = ar.take<int32_t>(B);
    if (!h->dev_cnt) {
      h->fld_arena.release();
      set_error("detector scratch carving failed");
      return RSPL_E_DEVICE;
    }
    for (hipEvent_t& e : h->fld_ev) RSPL_HIP(hipEventCreateWithFlags(&e, kTimingEventFlags));
  }
  if (hp > h->fld_hp) {
    if (h->fld_img) {
      RSPL_HIP(hipDeviceSynchronize());  // earlier calls may still read the old buffer
      (void)hipFree(h->fld_img);
      h->fld_img = nullptr;
      h->fld_hp = 0;
    }
    RSPL_HIP(hipMalloc((void**)&h->fld_img, B * 2 * hp));
    h->fld_hp = hp;
  }
  return RSPL_OK;
}

void fld_shape(rspl_lines* h, int hh, int hw, const rspl_fld_config* cfg) {
  fld::Args& a = h->fld;
  a.hh = hh;
  a.hw = hw;
  a.half = h->fld_img;
  a.cls = h->fld_img + (size_t)fld::kMaxBatch * hh * hw;
  a.len_thr = cfg ? cfg->length_threshold : 1;
  a.dist_thr = cfg ? cfg->distance_threshold : 0.0;
  a.out = nullptr;
  a.capacity = 0;
  a.counts = h->dev_cnt;
}

int fld_clear_meta(rspl_lines* h, int B, hipStream_t st) {
  h->fld_batch = B;
  RSPL_HIP(hipMemsetAsync(h->fld.meta, 0, sizeof(int) * fld::kMetaInts * B, st));
  return RSPL_OK;
}

}  // namespace

extern "C" int rspl_lines_detect_device(rspl_lines* h, const uint8_t* d_images, int batch, int H, int W, size_t stride,
                                        size_t pitch, const rspl_fld_config* cfg, float* d_segments, int capacity,
                                        int32_t* d_counts, void* stream) {
  if (int rc = fld_check_images(batch, H, W, stride, pitch, cfg)) return rc;
  RSPL_CHECK_ARG(capacity >= 0 && (capacity == 0 || d_segments), "capacity %d without a segment buffer", capacity);
  RSPL_CHECK_ARG(h && d_images && d_counts, "rspl_lines_detect_device: NULL argument");
  const int hh = H / 2, hw = W / 2;
  const size_t hp = (size_t)hh * hw;
  if (int rc = fld_reserve(h, hp)) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  fld_shape(h, hh, hw, cfg);
  fld::Args a = h->fld;
  a.out = d_segments;
  a.capacity = capacity;
  a.counts = d_counts;
  const bool prof = h->fld_profile;
  if (int rc = fld_clear_meta(h, batch, st)) return rc;
  if (prof) RSPL_HIP(hipEventRecord(h->fld_ev[0], st));
  for (int b = 0; b < batch; b++)
    RSPL_HIP(lines::canny_classes(canny_args(cfg, d_images + (size_t)b * pitch, H, W, (int)stride,
                                             h->fld_img + (size_t)b * hp,
                                             h->fld_img + ((size_t)fld::kMaxBatch + b) * hp), st));
  if (prof) RSPL_HIP(hipEventRecord(h->fld_ev[1], st));
  RSPL_HIP(fld::hysteresis(a, batch, st));
  if (prof) RSPL_HIP(hipEventRecord(h->fld_ev[2], st));
  RSPL_HIP(fld::labels(a, batch, st));
  if (prof) RSPL_HIP(hipEventRecord(h->fld_ev[3], st));
  RSPL_HIP(fld::walk(a, batch, st));
  if (prof) RSPL_HIP(hipEventRecord(h->fld_ev[4], st));
  RSPL_HIP(fld::fit(a, batch, st));
  if (prof) RSPL_HIP(hipEventRecord(h->fld_ev[5], st));
  RSPL_HIP(fld::order(a, batch, st));
  if (prof) RSPL_HIP(hipEventRecord(h->fld_ev[6], st));
  return RSPL_OK;
}

extern "C" int rspl_lines_detect_status(rspl_lines* h, int* status) {
  RSPL_CHECK_ARG(h && status, "rspl_lines_detect_status: NULL argument");
  *status = 0;
  if (!h->fld_arena.base || h->fld_batch == 0) return RSPL_OK;
  int meta[fld::kMaxBatch * fld::kMetaInts];
  RSPL_HIP(hipMemcpy(meta, h->fld.meta, sizeof(int) * fld::kMetaInts * h->fld_batch, hipMemcpyDeviceToHost));
  for (int b = 0; b < h->fld_batch; b++) *status |= meta[b * fld::kMetaInts + fld::kStatus];
  return RSPL_OK;
}

extern "C" int rspl_lines_debug_fld_stats(rspl_lines* h, int b, int32_t* stats) {
  RSPL_CHECK_ARG(h && stats && b >= 0 && b < fld::kMaxBatch && h->fld_arena.base,
                 "rspl_lines_debug_fld_stats: bad argument, or no device detection yet");
  RSPL_HIP(hipMemcpy(stats, h->fld.meta + b * fld::kMetaInts, sizeof(int) * 8, hipMemcpyDeviceToHost));
  return RSPL_OK;
}

extern "C" int rspl_lines_debug_fld_profile(rspl_lines* h, int enable) {
  RSPL_CHECK_ARG(h, "rspl_lines_debug_fld_profile: NULL handle");
  h->fld_profile = enable != 0;
  return RSPL_OK;
}

extern "C" int rspl_lines_debug_fld_stage_ms(rspl_lines* h, float* ms) {
  RSPL_CHECK_ARG(h && ms && h->fld_profile && h->fld_ev[0], "rspl_lines_debug_fld_stage_ms: no profiled call");
  RSPL_HIP(hipEventSynchronize(h->fld_ev[6]));
  for (int k = 0; k < 6; k++) RSPL_HIP(hipEventElapsedTime(&ms[k], h->fld_ev[k], h->fld_ev[k + 1]));
  return RSPL_OK;
}

extern "C" int rspl_lines_debug_hysteresis(rspl_lines* h, const uint8_t* cls, int hh, int hw, uint8_t* edges) {
  if (int rc = fld_check_mask(hh, hw)) return rc;
  RSPL_CHECK_ARG(h && cls && edges, "rspl_lines_debug_hysteresis: NULL argument");
  const size_t hp = (size_t)hh * hw;
  if (int rc = fld_reserve(h, hp)) return rc;
  fld_shape(h, hh, hw, nullptr);
  hipStream_t st = h->stream;
  if (int rc = fld_clear_meta(h, 1, st)) return rc;
  RSPL_HIP(hipMemcpyAsync((void*)h->fld.cls, cls, hp, hipMemcpyHostToDevice, st));
  RSPL_HIP(fld::hysteresis(h->fld, 1, st));
  const int wpr = fld::words_per_row(hw);
  std::vector<uint32_t> bits((size_t)hh * wpr);
  RSPL_HIP(hipMemcpyAsync(bits.data(), h->fld.ebits, bits.size() * 4, hipMemcpyDeviceToHost, st));
  RSPL_HIP(hipStreamSynchronize(st));
  for (int r = 0; r < hh; r++)
    for (int c = 0; c < hw; c++) edges[(size_t)r * hw + c] = (bits[(size_t)r * wpr + (c >> 5)] >> (c & 31)) & 1u ? 255 : 0;
  return RSPL_OK;
}

namespace {
std::vector<uint32_t> pack_edges(const uint8_t* edges, int hh, int hw) {
  const int wpr = fld::words_per_row(hw);
  std::vector<uint32_t> bits((size_t)hh * wpr, 0u);
  for (int r = 0; r < hh; r++)
    for (int c = 0; c < hw; c++)
      if (edges[(size_t)r * hw + c]) bits[(size_t)r * wpr + (c >> 5)] |= 1u << (c & 31);
  return bits;
}
}  // namespace

extern "C" int rspl_lines_debug_chains(rspl_lines* h, const uint8_t* edges, int hh, int hw, int32_t* seeds,
                                       int32_t* offsets, int32_t* points, int cap_chains, int cap_points,
                                       int* n_chains) {
  if (int rc = fld_check_mask(hh, hw)) return rc;
  RSPL_CHECK_ARG(h && edges && seeds && offsets && points && n_chains && cap_chains >= 0 && cap_points >= 0,
                 "rspl_lines_debug_chains: bad argument");
  *n_chains = 0;
  if (int rc = fld_reserve(h, (size_t)hh * hw)) return rc;
  fld_shape(h, hh, hw, nullptr);
  hipStream_t st = h->stream;
  if (int rc = fld_clear_meta(h, 1, st)) return rc;
  const std::vector<uint32_t> bits = pack_edges(edges, hh, hw);
  RSPL_HIP(hipMemcpyAsync(h->fld.ebits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, st));
  RSPL_HIP(fld::labels(h->fld, 1, st));
  RSPL_HIP(fld::walk(h->fld, 1, st));
  int meta[fld::kMetaInts];
  RSPL_HIP(hipMemcpyAsync(meta, h->fld.meta, sizeof(meta), hipMemcpyDeviceToHost, st));
  RSPL_HIP(hipStreamSynchronize(st));
  if (meta[fld::kStatus]) {
    set_error("rspl_lines_debug_chains: detector status %d (1: more than %d edge pixels, 4: internal bound)",
              meta[fld::kStatus], fld::kMaxEdge);
    return RSPL_E_CAPACITY;
  }
  const int nc = meta[fld::kNChain], ne = meta[fld::kNEdge];
  std::vector<int> ch((size_t)nc * 3);
  std::vector<uint32_t> pts((size_t)ne);
  if (nc) RSPL_HIP(hipMemcpy(ch.data(), h->fld.chains, ch.size() * 4, hipMemcpyDeviceToHost));
  if (ne) RSPL_HIP(hipMemcpy(pts.data(), h->fld.pts, pts.size() * 4, hipMemcpyDeviceToHost));
  std::vector<int> ord((size_t)nc);
  std::iota(ord.begin(), ord.end(), 0);
  std::sort(ord.begin(), ord.end(), [&](int x, int y) { return ch[3 * x] < ch[3 * y]; });
  long long total = 0;
  for (int k = 0; k < nc; k++) total += ch[3 * k + 2];
  *n_chains = nc;
  if (nc > cap_chains || total > cap_points) {
    set_error("%d chains / %lld points exceed the capacities %d / %d", nc, total, cap_chains, cap_points);
    return RSPL_E_CAPACITY;
  }
  int at = 0;
  for (int k = 0; k < nc; k++) {
    const int* c = &ch[3 * (size_t)ord[k]];
    seeds[k] = c[0];
    offsets[k] = at;
    for (int q = 0; q < c[2]; q++) {
      points[2 * (at + q)] = fld::pt_x(pts[c[1] + q]);
      points[2 * (at + q) + 1] = fld::pt_y(pts[c[1] + q]);
    }
    at += c[2];
  }
  offsets[nc] = at;
  return RSPL_OK;
}

namespace {

// the device job on the worker: wait for the detector's segments in pinned memory, then rspl_line_extract
void extract_job_device(rspl_lines* h) {
  int rc = RSPL_OK;
  h->a_n = 0;
  if (hipEventSynchronize(h->dev_done) != hipSuccess) {
    set_error("rspl_lines_extract_async_device: the detector's stream failed");
    rc = RSPL_E_DEVICE;
  }
  const int32_t* pin = h->dev_pin;
  const int status = pin[fld::kStatus], n = pin[fld::kMetaInts];
  if (rc == RSPL_OK && (status || n > rspl_lines::kDevSegCap)) {
    set_error("device detector status %d, %d segments (1: more than %d edge pixels, 2: more than %d segments, 4: "
              "internal bound)", status, n, fld::kMaxEdge, rspl_lines::kDevSegCap);
    rc = RSPL_E_CAPACITY;
  }
  if (rc == RSPL_OK) {
    h->a_lines.resize((size_t)std::max(n, 1) * 4);  // the merges never add lines
    rc = rspl_line_extract((const float*)(pin + fld::kMetaInts + 1), n, h->a_merge, h->a_lines.data(), std::max(n, 1),
                           &h->a_n);
  }
  h->a_rc = rc;
  h->a_err = rc == RSPL_OK ? std::string() : std::string(rspl_last_error());
  h->a_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h->a_t0).count();
}

}  // namespace

extern "C" int rspl_lines_extract_async_device(rspl_lines* h, const uint8_t* d_image, int H, int W, size_t stride,
                                               const rspl_fld_config* cfg, int do_merge, void* stream) {
  if (int rc = fld_check_images(1, H, W, stride, stride * (size_t)(H > 0 ? H : 0), cfg)) return rc;
  RSPL_CHECK_ARG(h && d_image, "rspl_lines_extract_async_device: NULL argument");
  {
    std::lock_guard<std::mutex> lk(h->mu);
    RSPL_CHECK_ARG(!h->job, "rspl_lines_extract_async_device: the previous job has not been waited for");
  }
  const auto t0 = std::chrono::steady_clock::now();
  constexpr size_t kPinBytes = sizeof(int32_t) * (fld::kMetaInts + 1) + sizeof(float) * 4 * rspl_lines::kDevSegCap;
  if (!h->dev_pin) {
    RSPL_HIP(hipHostMalloc((void**)&h->dev_pin, kPinBytes, hipHostMallocDefault));
    RSPL_HIP(hipEventCreateWithFlags(&h->dev_in, kOrderEventFlags));
    RSPL_HIP(hipEventCreateWithFlags(&h->dev_done, kHostEventFlags));  // the worker reads dev_pin after it
  }
  if (int rc = fld_reserve(h, (size_t)(H / 2) * (W / 2))) return rc;  // the job's device segments live there
  RSPL_HIP(hipEventRecord(h->dev_in, (hipStream_t)stream));
  RSPL_HIP(hipStreamWaitEvent(h->stream, h->dev_in, 0));
  if (int rc = rspl_lines_detect_device(h, d_image, 1, H, W, stride, stride * (size_t)H, cfg, h->dev_seg,
                                        rspl_lines::kDevSegCap, h->dev_cnt, h->stream))
    return rc;
  RSPL_HIP(hipMemcpyAsync(h->dev_pin, h->fld.meta, sizeof(int32_t) * fld::kMetaInts, hipMemcpyDeviceToHost, h->stream));
  RSPL_HIP(hipMemcpyAsync(h->dev_pin + fld::kMetaInts, h->dev_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  RSPL_HIP(hipMemcpyAsync(h->dev_pin + fld::kMetaInts + 1, h->dev_seg, sizeof(float) * 4 * rspl_lines::kDevSegCap,
                          hipMemcpyDeviceToHost, h->stream));
  RSPL_HIP(hipEventRecord(h->dev_done, h->stream));
  {
    std::lock_guard<std::mutex> lk(h->mu);
    h->a_merge = do_merge;
    h->a_dev = true;
    h->a_t0 = t0;
    h->job = true;
    h->done = false;
  }
  ensure_worker(h);
  h->cv.notify_all();
  return RSPL_OK;
}
