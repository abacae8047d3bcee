// RCF edge-network handle: C ABI (include/rspl.h, rspl_rcf_*) over rcf_conv.hip and rcf_side.hip.  Replaces the
// reference's TensorRT wrapper: RCF::build (src/rcf.cpp:25-93), RCF::infer (src/rcf.cpp:95-135) with
// process_input_1 (src/rcf.cpp:161-192: the gray image as raw floats in three identical channels) and
// process_output (src/rcf.cpp:137-159: 255 - p * 255 truncated).  MapBuilder::AddInput runs it on both rectified
// images of a frame (src/map_builder.cc:86-121) and hands the edge image to the line detector
// (src/map_builder.cc:286, :327).  The network itself is restated from the public model (yun-liu/RCF-PyTorch):
// the reference ships only the engine's path.  Weights are read once, laid out for the kernels and kept on the
// device; a call is a fixed chain of launches on one stream and never waits for the device.
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "rcf_kernels.hpp"

using namespace rspl;

namespace {

constexpr int kMinDim = 16, kMaxDim = 2048, kMaxBatch = 64;
constexpr int kConvs[rcf::kStages] = {2, 2, 3, 3, 3};
constexpr int kChan[rcf::kStages] = {64, 128, 256, 512, 512};
constexpr int kNumConvs = 13;

struct Conv {
  int cin, cout;
  void* w = nullptr;        // 3x3 weights in the kernels' layout (conv1_1: [9][64] floats)
  float* bias = nullptr;    // [cout]
  void* down_w = nullptr;   // [32][cout]
  float* down_b = nullptr;  // [32]
};

// stage sizes for an H x W image: max-pool 2, stride 2, ceil_mode before stages 2..4, stride 1 before stage 5
void stage_dims(int H, int W, int* Hs, int* Ws) {
  Hs[0] = H;
  Ws[0] = W;
  for (int s = 1; s < 4; s++) {
    Hs[s] = (Hs[s - 1] + 1) / 2;
    Ws[s] = (Ws[s - 1] + 1) / 2;
  }
  Hs[4] = Hs[3] - 1;
  Ws[4] = Ws[3] - 1;
}

}  // namespace

struct rspl_rcf {
  rspl_rcf_config cfg{};
  hipStream_t stream = nullptr;
  Arena arena;
  Conv conv[kNumConvs];
  float* dsn_w[rcf::kStages] = {};  // [32] each
  float dsn_b[rcf::kStages] = {};
  float fuse_w[rcf::kStages] = {}, fuse_b = 0;
  void *act[2] = {};                // ping-pong activations, each the largest stage of max_batch images
  float* side_acc = nullptr;        // [B][H][W][kSidePad]
  float* so[rcf::kStages] = {};     // [B][Hs][Ws]
  float* logits = nullptr;          // [B][6][H][W]
  uint8_t *d_img = nullptr, *d_edge = nullptr;  // rspl_rcf_infer's image and result
  int tile_rows = 0;                // rspl_rcf_debug_tile_rows
  StageTimer timer;                 // RSPL_RCF_STAGES: stages 1..5 (pool, convs, side branches), tail
  int last_H = 0, last_W = 0, last_B = 0;
  hipStream_t last_stream = nullptr;
};

namespace {

const Tensor* tensor(const std::vector<Tensor>& ts, const std::string& name, std::initializer_list<int64_t> dims) {
  for (auto& t : ts)
    if (t.name == name) {
      if (t.dims.size() != dims.size() || !std::equal(dims.begin(), dims.end(), t.dims.begin())) {
        std::string got, want;
        for (int64_t d : t.dims) got += (got.empty() ? "" : ",") + std::to_string(d);
        for (int64_t d : dims) want += (want.empty() ? "" : ",") + std::to_string(d);
        set_error("RCF weight %s has shape (%s), expected (%s)", name.c_str(), got.c_str(), want.c_str());
        return nullptr;
      }
      return &t;
    }
  set_error("RCF weight %s missing from blob", name.c_str());
  return nullptr;
}

template <typename T>
bool up(T* dst, const std::vector<T>& src) {
  return hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

int check_size(const rspl_rcf* h, int H, int W, const char* who) {
  RSPL_CHECK_ARG(H >= kMinDim && H <= h->cfg.max_height && W >= kMinDim && W <= h->cfg.max_width,
                 "%s: image %dx%d, sizes are %d..%dx%d", who, W, H, kMinDim, h->cfg.max_width, h->cfg.max_height);
  return RSPL_OK;
}

// every tensor of the state_dict present and of its shape: checked before a device is touched
int check_weights(const std::vector<Tensor>& ts) {
  int cin = 3;
  for (int s = 0; s < rcf::kStages; s++) {
    const std::string n = std::to_string(s + 1);
    for (int k = 0; k < kConvs[s]; k++) {
      const std::string name = "conv" + n + "_" + std::to_string(k + 1);
      if (!tensor(ts, name + ".weight", {kChan[s], cin, 3, 3}) || !tensor(ts, name + ".bias", {kChan[s]}) ||
          !tensor(ts, name + "_down.weight", {rcf::kSide, kChan[s], 1, 1}) ||
          !tensor(ts, name + "_down.bias", {rcf::kSide}))
        return RSPL_E_WEIGHTS;
      cin = kChan[s];
    }
    if (!tensor(ts, "score_dsn" + n + ".weight", {1, rcf::kSide, 1, 1}) || !tensor(ts, "score_dsn" + n + ".bias", {1}))
      return RSPL_E_WEIGHTS;
  }
  if (!tensor(ts, "score_fuse.weight", {1, rcf::kStages, 1, 1}) || !tensor(ts, "score_fuse.bias", {1}))
    return RSPL_E_WEIGHTS;
  return RSPL_OK;
}

// reads the blob into the handle's device weights; the arena is reserved by the caller
int load_weights(rspl_rcf* h, const std::vector<Tensor>& ts) {
  const bool half = h->cfg.precision == RSPL_PREC_FP16;
  int ci = 0;
  for (int s = 0; s < rcf::kStages; s++) {
    for (int k = 0; k < kConvs[s]; k++, ci++) {
      Conv& c = h->conv[ci];
      const std::string name = "conv" + std::to_string(s + 1) + "_" + std::to_string(k + 1);
      const int cin_file = ci == 0 ? 3 : c.cin;
      const Tensor* w = tensor(ts, name + ".weight", {c.cout, cin_file, 3, 3});
      const Tensor* b = w ? tensor(ts, name + ".bias", {c.cout}) : nullptr;
      const Tensor* dw = b ? tensor(ts, name + "_down.weight", {rcf::kSide, c.cout, 1, 1}) : nullptr;
      const Tensor* db = dw ? tensor(ts, name + "_down.bias", {rcf::kSide}) : nullptr;
      if (!db) return RSPL_E_WEIGHTS;
      bool ok = true;
      if (ci == 0) {  // the three identical input channels folded: [9][64]
        std::vector<float> r(9 * 64);
        for (int co = 0; co < 64; co++)
          for (int t = 0; t < 9; t++) {
            const double sum = (double)w->data[(co * 3 + 0) * 9 + t] + (double)w->data[(co * 3 + 1) * 9 + t] +
                               (double)w->data[(co * 3 + 2) * 9 + t];
            r[t * 64 + co] = half ? (float)(_Float16)(float)sum : (float)sum;
          }
        ok = up((float*)c.w, r);
      } else if (half) {  // [9][cout][cin]
        std::vector<_Float16> r((size_t)9 * c.cin * c.cout);
        for (int co = 0; co < c.cout; co++)
          for (int i = 0; i < c.cin; i++)
            for (int t = 0; t < 9; t++)
              r[((size_t)t * c.cout + co) * c.cin + i] = (_Float16)w->data[((size_t)co * c.cin + i) * 9 + t];
        ok = up((_Float16*)c.w, r);
      } else {  // [9][cin][cout]
        std::vector<float> r((size_t)9 * c.cin * c.cout);
        for (int co = 0; co < c.cout; co++)
          for (int i = 0; i < c.cin; i++)
            for (int t = 0; t < 9; t++)
              r[((size_t)t * c.cin + i) * c.cout + co] = w->data[((size_t)co * c.cin + i) * 9 + t];
        ok = up((float*)c.w, r);
      }
      ok = ok && up(c.bias, b->data);
      if (half) {
        std::vector<_Float16> r((size_t)rcf::kSideRows * c.cout, (_Float16)0.f);
        for (size_t i = 0; i < dw->data.size(); i++) r[i] = (_Float16)dw->data[i];
        ok = ok && up((_Float16*)c.down_w, r);
      } else {
        std::vector<float> r((size_t)rcf::kSideRows * c.cout, 0.f);
        std::copy(dw->data.begin(), dw->data.end(), r.begin());
        ok = ok && up((float*)c.down_w, r);
      }
      std::vector<float> rb(rcf::kSideRows, 0.f);
      std::copy(db->data.begin(), db->data.end(), rb.begin());
      ok = ok && up(c.down_b, rb);
      if (!ok) {
        set_error("rspl_rcf_create: upload of %s failed", name.c_str());
        return RSPL_E_DEVICE;
      }
    }
    const std::string name = "score_dsn" + std::to_string(s + 1);
    const Tensor* w = tensor(ts, name + ".weight", {1, rcf::kSide, 1, 1});
    const Tensor* b = w ? tensor(ts, name + ".bias", {1}) : nullptr;
    if (!b) return RSPL_E_WEIGHTS;
    std::vector<float> r(rcf::kSideRows, 0.f);
    std::copy(w->data.begin(), w->data.end(), r.begin());
    if (!up(h->dsn_w[s], r)) {
      set_error("rspl_rcf_create: upload of %s failed", name.c_str());
      return RSPL_E_DEVICE;
    }
    h->dsn_b[s] = b->data[0];
  }
  const Tensor* w = tensor(ts, "score_fuse.weight", {1, rcf::kStages, 1, 1});
  const Tensor* b = w ? tensor(ts, "score_fuse.bias", {1}) : nullptr;
  if (!b) return RSPL_E_WEIGHTS;
  for (int s = 0; s < rcf::kStages; s++) h->fuse_w[s] = w->data[s];
  h->fuse_b = b->data[0];
  return RSPL_OK;
}

// the device layout, once to size the arena (Sizer) and once to carve it (Arena)
// (alloc(bytes) returns the block, or null in the sizing pass)
template <typename Alloc>
void carve(rspl_rcf* h, Alloc&& alloc) {
  const bool half = h->cfg.precision == RSPL_PREC_FP16;
  const size_t es = half ? 2 : 4, B = h->cfg.max_batch;
  int Hs[rcf::kStages], Ws[rcf::kStages];
  stage_dims(h->cfg.max_height, h->cfg.max_width, Hs, Ws);
  size_t act = 0;
  for (int s = 0; s < rcf::kStages; s++) act = std::max(act, (size_t)Hs[s] * Ws[s] * kChan[s]);
  const size_t px = (size_t)Hs[0] * Ws[0];
  auto take = [&](auto*& p, size_t bytes) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(alloc(bytes)); };
  for (int i = 0; i < kNumConvs; i++) {
    Conv& c = h->conv[i];
    take(c.w, i == 0 ? 9 * 64 * sizeof(float) : (size_t)9 * c.cin * c.cout * es);
    take(c.bias, c.cout * sizeof(float));
    take(c.down_w, (size_t)rcf::kSideRows * c.cout * es);
    take(c.down_b, rcf::kSideRows * sizeof(float));
  }
  for (int s = 0; s < rcf::kStages; s++) take(h->dsn_w[s], rcf::kSideRows * sizeof(float));
  take(h->act[0], B * act * es);
  take(h->act[1], B * act * es);
  take(h->side_acc, B * px * rcf::kSidePad * sizeof(float));
  for (int s = 0; s < rcf::kStages; s++) take(h->so[s], B * (size_t)Hs[s] * Ws[s] * sizeof(float));
  take(h->logits, B * 6 * px * sizeof(float));
  take(h->d_img, px);
  take(h->d_edge, px);
}

int run(rspl_rcf* h, const uint8_t* d_images, int B, int H, int W, size_t stride, size_t pitch, uint8_t* d_edges,
        size_t out_stride, size_t out_pitch, hipStream_t st) {
  const bool half = h->cfg.precision == RSPL_PREC_FP16;
  int Hs[rcf::kStages], Ws[rcf::kStages];
  stage_dims(H, W, Hs, Ws);
  int cur = 0, ci = 0;
  for (int s = 0; s < rcf::kStages; s++) {
    h->timer.mark(s, st);
    if (s > 0) {
      rcf::PoolArgs p{h->act[cur], h->act[cur ^ 1], Hs[s - 1], Ws[s - 1], Hs[s], Ws[s], B, kChan[s - 1], s == 4 ? 1 : 2};
      RSPL_HIP(rcf::pool(p, half, st));
      cur ^= 1;
    }
    for (int k = 0; k < kConvs[s]; k++, ci++) {
      const Conv& c = h->conv[ci];
      if (ci == 0) {
        rcf::FirstArgs f{d_images, stride, pitch, (const float*)c.w, c.bias, h->act[cur], H, W, B};
        RSPL_HIP(rcf::first_conv(f, half, st));
      } else {
        rcf::ConvArgs a{h->act[cur], c.w, c.bias, h->act[cur ^ 1], Hs[s], Ws[s], B, c.cin, c.cout, s == 4 ? 2 : 1,
                        h->tile_rows};
        RSPL_HIP(rcf::conv3x3(a, half, st));
        cur ^= 1;
      }
      rcf::SideArgs sd{};
      sd.act = h->act[cur];
      sd.w = c.down_w;
      sd.bias = c.down_b;
      sd.acc = h->side_acc;
      sd.dsn_w = h->dsn_w[s];
      sd.dsn_b = h->dsn_b[s];
      sd.so = h->so[s];
      sd.npix = (size_t)B * Hs[s] * Ws[s];
      sd.C = c.cout;
      sd.first = k == 0;
      sd.last = k == kConvs[s] - 1;
      RSPL_HIP(rcf::side(sd, half, st));
    }
  }
  rcf::TailArgs t{};
  for (int s = 0; s < rcf::kStages; s++) {
    t.so[s] = h->so[s];
    t.Hs[s] = Hs[s];
    t.Ws[s] = Ws[s];
    t.fuse_w[s] = h->fuse_w[s];
  }
  t.fuse_b = h->fuse_b;
  t.logits = h->logits;
  t.edges = d_edges;
  t.out_stride = out_stride;
  t.out_pitch = out_pitch;
  t.H = H;
  t.W = W;
  t.B = B;
  t.output = h->cfg.output;
  h->timer.mark(rcf::kStages, st);
  RSPL_HIP(rcf::tail(t, st));
  h->timer.mark(RSPL_RCF_STAGES, st);
  h->timer.end_call();
  h->last_H = H;
  h->last_W = W;
  h->last_B = B;
  h->last_stream = st;
  return RSPL_OK;
}

}  // namespace

extern "C" int rspl_rcf_debug_sizeof(int which) { return which == 0 ? (int)sizeof(rspl_rcf_config) : -1; }

// RCF::build (src/rcf.cpp:25-93)
extern "C" int rspl_rcf_create(const rspl_rcf_config* cfg, const char* weights_path, rspl_rcf** out) {
  RSPL_CHECK_ARG(cfg && out, "rspl_rcf_create: NULL argument");
  *out = nullptr;
  RSPL_CHECK_ARG(cfg->max_height >= kMinDim && cfg->max_height <= kMaxDim && cfg->max_width >= kMinDim &&
                     cfg->max_width <= kMaxDim,
                 "rspl_rcf_create: max size %dx%d, sizes are %d..%d", cfg->max_width, cfg->max_height, kMinDim, kMaxDim);
  RSPL_CHECK_ARG(cfg->max_batch >= 1 && cfg->max_batch <= kMaxBatch, "rspl_rcf_create: max_batch %d, 1..%d",
                 cfg->max_batch, kMaxBatch);
  RSPL_CHECK_ARG(cfg->precision == RSPL_PREC_FP32 || cfg->precision == RSPL_PREC_FP16,
                 "rspl_rcf_create: precision %d (RSPL_PREC_FP32 or RSPL_PREC_FP16)", cfg->precision);
  RSPL_CHECK_ARG(cfg->output >= 0 && cfg->output <= 5, "rspl_rcf_create: output %d, 0..5", cfg->output);
  std::vector<Tensor> ts;
  if (int rc = load_blob(weights_path, ts)) return rc;
  if (int rc = check_weights(ts)) return rc;
  auto* h = new rspl_rcf();
  h->cfg = *cfg;
  int ci = 0;
  for (int s = 0; s < rcf::kStages; s++)
    for (int k = 0; k < kConvs[s]; k++, ci++) {
      h->conv[ci].cin = k > 0 ? kChan[s] : (s > 0 ? kChan[s - 1] : 1);
      h->conv[ci].cout = kChan[s];
    }
  Sizer sz;
  carve(h, [&](size_t n) {
    sz.take<char>(n);
    return (char*)nullptr;
  });
  bool ok = hipSetDevice(cfg->device) == hipSuccess && h->timer.init(RSPL_RCF_STAGES) == RSPL_OK &&
            hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
            h->arena.reserve(sz.used + 256) == RSPL_OK;
  if (ok) {
    carve(h, [&](size_t n) { return h->arena.take<char>(n); });
    ok = h->d_edge != nullptr;  // the last block carved: the arena held them all
  }
  if (!ok) {
    set_error("rspl_rcf_create: device, stream or allocation of %zu bytes failed", sz.used);
    rspl_rcf_destroy(h);
    return RSPL_E_DEVICE;
  }
  if (int rc = load_weights(h, ts)) {
    rspl_rcf_destroy(h);
    return rc;
  }
  *out = h;
  return RSPL_OK;
}

extern "C" void rspl_rcf_destroy(rspl_rcf* h) {
  if (!h) return;
  if (h->stream) (void)hipStreamSynchronize(h->stream);  // (calls on a caller's stream: the caller has waited)
  h->timer.destroy();
  h->arena.release();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// RCF::infer on device images (src/rcf.cpp:95-135 without the copies of :121 and :126)
extern "C" int rspl_rcf_infer_device(rspl_rcf* h, const uint8_t* d_images, int batch, int H, int W, size_t stride,
                                     size_t pitch, uint8_t* d_edges, size_t out_stride, size_t out_pitch,
                                     void* stream) {
  RSPL_CHECK_ARG(h && batch >= 0, "rspl_rcf_infer_device: bad argument");
  RSPL_CHECK_ARG(batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
  if (int rc = check_size(h, H, W, "rspl_rcf_infer_device")) return rc;
  if (batch == 0) return RSPL_OK;
  RSPL_CHECK_ARG(d_images && d_edges, "rspl_rcf_infer_device: NULL argument");
  RSPL_CHECK_ARG(stride >= (size_t)W && out_stride >= (size_t)W, "strides %zu / %zu below the width %d", stride,
                 out_stride, W);
  const size_t image = (size_t)(H - 1) * stride + W, out_image = (size_t)(H - 1) * out_stride + W;
  RSPL_CHECK_ARG(batch == 1 || (pitch >= image && out_pitch >= out_image),
                 "pitches %zu / %zu below an image (%zu / %zu bytes)", pitch, out_pitch, image, out_image);
  RSPL_CHECK_ARG(stride <= (size_t)1 << 31 && out_stride <= (size_t)1 << 31 && pitch <= (size_t)1 << 40 &&
                     out_pitch <= (size_t)1 << 40,
                 "rspl_rcf_infer_device: stride or pitch too large");
  return run(h, d_images, batch, H, W, stride, pitch, d_edges, out_stride, out_pitch,
             stream ? (hipStream_t)stream : h->stream);
}

// RCF::infer (src/rcf.cpp:95-135) with process_output's u8 conversion (src/rcf.cpp:147-152)
extern "C" int rspl_rcf_infer(rspl_rcf* h, const uint8_t* image, int H, int W, size_t stride, uint8_t* edges) {
  RSPL_CHECK_ARG(h && image && edges, "rspl_rcf_infer: NULL argument");
  if (int rc = check_size(h, H, W, "rspl_rcf_infer")) return rc;
  RSPL_CHECK_ARG(stride >= (size_t)W, "stride %zu below the width %d", stride, W);
  RSPL_HIP(hipMemcpy2DAsync(h->d_img, W, image, stride, W, H, hipMemcpyHostToDevice, h->stream));
  if (int rc = run(h, h->d_img, 1, H, W, W, (size_t)H * W, h->d_edge, W, (size_t)H * W, h->stream)) return rc;
  RSPL_HIP(hipMemcpyAsync(edges, h->d_edge, (size_t)H * W, hipMemcpyDeviceToHost, h->stream));
  RSPL_HIP(hipStreamSynchronize(h->stream));
  return RSPL_OK;
}

// measurement hooks (tools/bench_rcf.py), as rspl_sp_profile / rspl_sp_stage_times
extern "C" int rspl_rcf_profile(rspl_rcf* h, int enable) {
  RSPL_CHECK_ARG(h, "rspl_rcf_profile: NULL handle");
  h->timer.reset(enable != 0);
  return RSPL_OK;
}

extern "C" int rspl_rcf_stage_times(rspl_rcf* h, float* ms, int* calls) {
  RSPL_CHECK_ARG(h && ms, "rspl_rcf_stage_times: NULL argument");
  return h->timer.query(ms, calls);
}

// test hook: no counterpart in the reference
extern "C" int rspl_rcf_debug_tile_rows(rspl_rcf* h, int rows) {
  RSPL_CHECK_ARG(h && (rows == 0 || rows == 8 || rows == 16), "rspl_rcf_debug_tile_rows: rows 0, 8 or 16");
  h->tile_rows = rows;
  return RSPL_OK;
}

// parity hook: no counterpart in the reference (the engine's other five bindings, output/readme.txt, are not read there)
extern "C" int rspl_rcf_debug_logits(rspl_rcf* h, int b, int which, float* out) {
  RSPL_CHECK_ARG(h && out && which >= 0 && which <= 5, "rspl_rcf_debug_logits: bad argument");
  RSPL_CHECK_ARG(h->last_B > 0 && b >= 0 && b < h->last_B, "rspl_rcf_debug_logits: image %d of a call of %d", b,
                 h->last_B);
  const size_t hw = (size_t)h->last_H * h->last_W;
  RSPL_HIP(hipStreamSynchronize(h->last_stream));
  RSPL_HIP(hipMemcpy(out, h->logits + ((size_t)b * 6 + which) * hw, hw * sizeof(float), hipMemcpyDeviceToHost));
  return RSPL_OK;
}
