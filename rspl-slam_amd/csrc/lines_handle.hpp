#pragma once
// The rspl_lines handle: shared by lines.cpp (assignment, matching, stereo association) and lines_detect.cpp
// (the two detectors, the asynchronous worker, the debug hooks).
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.hpp"
#include "fld_host.hpp"
#include "fld_kernels.hpp"

struct rspl_lines {
  rspl_lines_config cfg{};
  hipStream_t stream = nullptr;
  rspl::Arena arena;
  int cap = 0;
  double *lines, *pts, *dist;
  int *n_lines, *n_points, *offsets, *idx, *status;
  int *matches, *n_matches, *M, *inv, *out;
  // detector (rspl_lines_detect): device image / half image / classes, pinned host copies; grown on demand
  uint8_t *d_img = nullptr, *d_det = nullptr, *h_img = nullptr, *h_det = nullptr;
  size_t det_cap = 0;  // pixels of the largest full-size image so far
  int det_H = 0, det_W = 0;  // the last detection's image size (rspl_lines_debug_canny must match it)
  rspl::fld::HostScratch fld_host;  // the host detector's edge map, hysteresis stack and chain points
  // asynchronous LineExtractor (rspl_lines_extract_async / _wait): a native worker thread of the handle
  // runs detect + the merge passes, so a caller's feature thread only submits and joins (the reference's
  // line threads, map_builder.cc:285-290, 325-337)
  std::thread worker;
  std::mutex mu;
  std::condition_variable cv;
  bool job = false, done = false, quit = false;
  const uint8_t* a_img = nullptr;
  int a_H = 0, a_W = 0, a_stride = 0, a_merge = 1, a_rc = 0, a_n = 0;
  double a_us = 0;  // the job's own duration on the worker
  double ph_us[4] = {0, 0, 0, 0};  // the last detection's phases (image staged, GPU classes back, FLD), us
  // rspl_lines_extract_wait_device: the worker's lines staged in pinned memory and copied to the device in
  // stream order, through a ring of kPinSlots buffers: a slot is rewritten only once its copy of
  // kPinSlots joins ago has completed (copy_ev), so a join never waits for the stream in practice
  static constexpr int kPinSlots = 4;
  double* pin_lines[kPinSlots] = {};
  int pin_cap = 0;  // lines per slot
  hipEvent_t copy_ev[kPinSlots] = {};
  bool copy_pending[kPinSlots] = {};
  int pin_next = 0;
  rspl_fld_config a_cfg{};
  std::vector<float> a_seg;
  // device detector (rspl_lines_detect_device): scratch for fld::kMaxBatch images, allocated at the first call;
  // the half images and classes grow with the image size
  rspl::Arena fld_arena;
  rspl::fld::Args fld{};
  uint8_t* fld_img = nullptr;  // [kMaxBatch][2][fld_hp]: half image, classes
  size_t fld_hp = 0;
  int fld_batch = 0;           // images of the last call (rspl_lines_detect_status)
  bool fld_profile = false;
  hipEvent_t fld_ev[7] = {};
  // rspl_lines_extract_async_device: the job's input event, its segments and count on the device, their pinned
  // copies ([kMetaInts] ints of the image's meta, then the count, then the segments) and the event behind them
  static constexpr int kDevSegCap = 4096;
  float* dev_seg = nullptr;
  int32_t* dev_cnt = nullptr;
  int32_t* dev_pin = nullptr;
  hipEvent_t dev_in = nullptr, dev_done = nullptr;
  bool a_dev = false;
  std::chrono::steady_clock::time_point a_t0;
  std::vector<double> a_lines;
  std::string a_err;
};
