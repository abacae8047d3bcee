// Stereo rectification handle: C ABI (include/rspl.h, rspl_rect_*) over rect_kernels.hip.  Mirrors what the
// reference does on the host before anything else sees a frame -- Camera::Camera's maps
// (src/camera.cc:9-63: cv::initUndistortRectifyMap or its cv::fisheye twin) and Camera::UndistortImage
// (src/camera.cc:87-91: cv::remap, INTER_LINEAR), run by MapBuilder::AddInput (src/map_builder.cc:53-60).
// The maps are built on the host once, turned into the kernel's fixed-point table once and kept on the
// device; per frame one launch remaps a batch of images of both cameras, device in, device out.
// Operation order of the map builders follows the restatement (tests/rect_ref.py); FP contraction is off in
// this file, so the maps are bit-exact with it.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "common.hpp"
#include "rect_kernels.hpp"

#pragma clang fp contract(off)

using namespace rspl;

struct rspl_rect {
  rspl_rect_config cfg{};
  hipStream_t stream = nullptr;
  std::vector<float> map_x[2], map_y[2];
  std::vector<uint32_t> h_table;  // staging of one camera's table
  Arena arena;
  PinnedArena pinned;
  uint32_t* table = nullptr;  // device [2][H][tpitch]
  uint8_t *raw = nullptr, *out = nullptr;  // device [2][H][W] each: rspl_rect_pair's images
  uint8_t *h_raw = nullptr, *h_raw_dev = nullptr;  // host-mapped pinned slot and its device address
  uint8_t* h_out = nullptr;                        // pinned
};

namespace {

// Gauss-Jordan with partial pivoting, the operations in the order of oracle/ba.c's small_inv
bool inv3(const double* A, double* I) {
  double M[3][6];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      M[i][j] = A[3 * i + j];
      M[i][3 + j] = (i == j);
    }
  for (int c = 0; c < 3; c++) {
    int p = c;
    for (int r = c + 1; r < 3; r++)
      if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
    if (M[p][c] == 0 || !std::isfinite(M[p][c])) return false;
    if (p != c)
      for (int k = 0; k < 6; k++) std::swap(M[c][k], M[p][k]);
    const double iv = 1.0 / M[c][c];
    for (int k = 0; k < 6; k++) M[c][k] *= iv;
    for (int r = 0; r < 3; r++)
      if (r != c) {
        const double f = M[r][c];
        for (int k = 0; k < 6; k++) M[r][k] -= f * M[c][k];
      }
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) I[3 * i + j] = M[i][3 + j];
  return true;
}

int build_maps(const rspl_rect_camera& c, int type, int H, int W, float* map_x, float* map_y) {
  bool finite = true;
  for (double v : c.K) finite = finite && std::isfinite(v);
  for (double v : c.D) finite = finite && std::isfinite(v);
  for (double v : c.R) finite = finite && std::isfinite(v);
  for (double v : c.P) finite = finite && std::isfinite(v);
  RSPL_CHECK_ARG(finite, "rectification: non-finite camera parameter");
  RSPL_CHECK_ARG(type == 0 || (c.D[4] == 0 && c.D[5] == 0 && c.D[6] == 0 && c.D[7] == 0),
                 "rectification: the fisheye model has four coefficients, D[4..7] must be 0");
  double PR[9], iR[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      PR[3 * i + j] = c.P[4 * i] * c.R[j] + c.P[4 * i + 1] * c.R[3 + j] + c.P[4 * i + 2] * c.R[6 + j];
  RSPL_CHECK_ARG(inv3(PR, iR), "rectification: P[:3,:3] * R is singular");
  const double fx = c.K[0], fy = c.K[4], cx = c.K[2], cy = c.K[5];
  const double k1 = c.D[0], k2 = c.D[1];
  constexpr double inf = std::numeric_limits<double>::infinity();
  for (int i = 0; i < H; i++) {
    const double di = i;
    for (int j = 0; j < W; j++) {
      const double dj = j;
      const double _x = di * iR[1] + iR[2] + dj * iR[0];
      const double _y = di * iR[4] + iR[5] + dj * iR[3];
      const double _w = di * iR[7] + iR[8] + dj * iR[6];
      double u, v;
      if (type == 0) {
        const double p1 = c.D[2], p2 = c.D[3], k3 = c.D[4], k4 = c.D[5], k5 = c.D[6], k6 = c.D[7];
        const double x = _x / _w, y = _y / _w;
        const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2 * x * y;
        const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
        const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
        const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
        u = fx * xd + cx;
        v = fy * yd + cy;
      } else {
        const double k3 = c.D[2], k4 = c.D[3];
        double x, y;
        if (_w <= 0) {  // behind the camera: OpenCV's infinities, which end as NaN maps
          x = _x > 0 ? -inf : inf;
          y = _y > 0 ? -inf : inf;
        } else {
          x = _x / _w;
          y = _y / _w;
        }
        const double r = std::sqrt(x * x + y * y), th = std::atan(r);
        const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
        const double thd = th * (1 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8);
        const double scale = (r == 0) ? 1.0 : thd / r;
        u = fx * x * scale + cx;
        v = fy * y * scale + cy;
      }
      map_x[(size_t)i * W + j] = (float)u;
      map_y[(size_t)i * W + j] = (float)v;
    }
  }
  return RSPL_OK;
}

// cv::remap's coordinate rounding on one axis of extent N: cvRound(m * 32) (half to even), then the outside
// classes clamped so the result fits the table
inline void fix_axis(float m, int N, int* i, int* f) {
  const float v = m * 32.0f;
  if (!(v >= -64.0f)) {  // NaN, -inf, or both taps left of the image
    *i = -2;
    *f = 0;
    return;
  }
  if (v >= (float)(N * 32)) {
    *i = N;
    *f = 0;
    return;
  }
  const int s = (int)std::lrintf(v);
  *i = s >> 5;
  *f = (*i == -2) ? 0 : (s & 31);
}

void build_table(const float* mx, const float* my, int H, int W, uint32_t* t) {
  const size_t tp = rect::table_pitch(W);
  for (int y = 0; y < H; y++)
    for (size_t x = 0; x < tp; x++) {
      int ix = -2, iy = -2, fx = 0, fy = 0;
      if (x < (size_t)W) {
        fix_axis(mx[(size_t)y * W + x], W, &ix, &fx);
        fix_axis(my[(size_t)y * W + x], H, &iy, &fy);
      }
      t[(size_t)y * tp + x] = rect::pack(ix, iy, fx, fy);
    }
}

int upload_table(rspl_rect* h, int cam) {
  const int H = h->cfg.height, W = h->cfg.width;
  const size_t n = (size_t)H * rect::table_pitch(W);
  build_table(h->map_x[cam].data(), h->map_y[cam].data(), H, W, h->h_table.data());
  RSPL_HIP(hipMemcpy(h->table + n * cam, h->h_table.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
  return RSPL_OK;
}

int check_size(int H, int W, int type, const char* who) {
  RSPL_CHECK_ARG(H > 0 && W > 0 && H <= rect::kMaxDim && W <= rect::kMaxDim, "%s: image %dx%d, sizes are 1..%d", who,
                 W, H, rect::kMaxDim);
  RSPL_CHECK_ARG(type == 0 || type == 1, "%s: distortion_type %d (0 radial-tangential, 1 fisheye)", who, type);
  return RSPL_OK;
}

}  // namespace

extern "C" int rspl_rect_build_maps(const rspl_rect_camera* cam, int distortion_type, int H, int W, float* map_x,
                                    float* map_y) {
  RSPL_CHECK_ARG(cam && map_x && map_y, "rspl_rect_build_maps: NULL argument");
  if (int rc = check_size(H, W, distortion_type, "rspl_rect_build_maps")) return rc;
  return build_maps(*cam, distortion_type, H, W, map_x, map_y);
}

extern "C" int rspl_rect_debug_fixed(const float* map_x, const float* map_y, size_t n, int H, int W, int16_t* ix,
                                     int16_t* iy, uint16_t* frac) {
  RSPL_CHECK_ARG((map_x && map_y && ix && iy && frac) || n == 0, "rspl_rect_debug_fixed: NULL argument");
  if (int rc = check_size(H, W, 0, "rspl_rect_debug_fixed")) return rc;
  for (size_t k = 0; k < n; k++) {
    int i, j, fx, fy;
    fix_axis(map_x[k], W, &i, &fx);
    fix_axis(map_y[k], H, &j, &fy);
    ix[k] = (int16_t)i;
    iy[k] = (int16_t)j;
    frac[k] = (uint16_t)(fx | fy << 5);
  }
  return RSPL_OK;
}

extern "C" int rspl_rect_debug_sizeof(int which) {
  return which == 0 ? (int)sizeof(rspl_rect_camera) : which == 1 ? (int)sizeof(rspl_rect_config) : -1;
}

extern "C" int rspl_rect_debug_copy(void* d_dst, const void* d_src, size_t bytes, void* stream) {
  RSPL_CHECK_ARG((d_dst && d_src) || bytes == 0, "rspl_rect_debug_copy: NULL argument");
  RSPL_CHECK_ARG(((uintptr_t)d_dst | (uintptr_t)d_src) % 16 == 0, "rspl_rect_debug_copy: pointers must be 16-byte aligned");
  RSPL_HIP(upload_mapped(d_dst, d_src, bytes, (hipStream_t)stream));
  return RSPL_OK;
}

extern "C" int rspl_rect_create(const rspl_rect_config* cfg, rspl_rect** out) {
  RSPL_CHECK_ARG(cfg && out, "rspl_rect_create: NULL argument");
  *out = nullptr;
  if (int rc = check_size(cfg->height, cfg->width, cfg->distortion_type, "rspl_rect_create")) return rc;
  RSPL_CHECK_ARG(cfg->max_batch > 0 && cfg->max_batch <= rect::kMaxBatch, "rspl_rect_create: max_batch %d, 1..%d",
                 cfg->max_batch, rect::kMaxBatch);
  const int H = cfg->height, W = cfg->width;
  const size_t px = (size_t)H * W, tn = (size_t)H * rect::table_pitch(W);
  auto* h = new rspl_rect();
  h->cfg = *cfg;
  for (int c = 0; c < 2; c++) {  // the maps first: a bad calibration is refused before a device is touched
    h->map_x[c].resize(px);
    h->map_y[c].resize(px);
    if (int rc = build_maps(cfg->cam[c], cfg->distortion_type, H, W, h->map_x[c].data(), h->map_y[c].data())) {
      delete h;
      return rc;
    }
  }
  h->h_table.resize(tn);
  Sizer sz;
  sz.take<uint32_t>(2 * tn);
  sz.take<uint8_t>(2 * px);
  sz.take<uint8_t>(2 * px);
  bool ok = hipSetDevice(cfg->device) == hipSuccess &&
            hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
            h->arena.reserve(sz.used + 256) == RSPL_OK;
  if (ok) {
    h->table = h->arena.take<uint32_t>(2 * tn);
    h->raw = h->arena.take<uint8_t>(2 * px);
    h->out = h->arena.take<uint8_t>(2 * px);
    ok = h->table && h->raw && h->out &&
         h->pinned.reserve(2 * px) == RSPL_OK && (h->h_raw = h->pinned.take<uint8_t>(2 * px, &h->h_raw_dev)) &&
         hipHostMalloc((void**)&h->h_out, 2 * px) == hipSuccess && upload_table(h, 0) == RSPL_OK &&
         upload_table(h, 1) == RSPL_OK;
  }
  if (!ok) {
    set_error("rspl_rect_create: device, stream or allocation failed");
    rspl_rect_destroy(h);
    return RSPL_E_DEVICE;
  }
  *out = h;
  return RSPL_OK;
}

extern "C" void rspl_rect_destroy(rspl_rect* h) {
  if (!h) return;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->pinned.release();
  if (h->h_out) (void)hipHostFree(h->h_out);
  h->arena.release();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int rspl_rect_get_maps(rspl_rect* h, int cam, float* map_x, float* map_y) {
  RSPL_CHECK_ARG(h && map_x && map_y && (cam == 0 || cam == 1), "rspl_rect_get_maps: bad argument");
  const size_t px = (size_t)h->cfg.height * h->cfg.width;
  memcpy(map_x, h->map_x[cam].data(), sizeof(float) * px);
  memcpy(map_y, h->map_y[cam].data(), sizeof(float) * px);
  return RSPL_OK;
}

extern "C" int rspl_rect_set_maps(rspl_rect* h, int cam, const float* map_x, const float* map_y) {
  RSPL_CHECK_ARG(h && map_x && map_y && (cam == 0 || cam == 1), "rspl_rect_set_maps: bad argument");
  const size_t px = (size_t)h->cfg.height * h->cfg.width;
  RSPL_HIP(hipSetDevice(h->cfg.device));
  RSPL_HIP(hipDeviceSynchronize());  // launches on the caller's streams may still read the table
  memcpy(h->map_x[cam].data(), map_x, sizeof(float) * px);
  memcpy(h->map_y[cam].data(), map_y, sizeof(float) * px);
  return upload_table(h, cam);
}

namespace {

int enqueue(rspl_rect* h, int batch, const uint8_t* d_raw, size_t raw_stride, size_t raw_pitch, const int* cam_index,
            uint8_t* d_out, size_t out_stride, size_t out_pitch, hipStream_t stream) {
  RSPL_CHECK_ARG(d_raw && d_out && cam_index, "rspl_rect_enqueue_device: NULL argument");
  const size_t H = h->cfg.height, W = h->cfg.width;
  RSPL_CHECK_ARG(raw_stride >= W && out_stride >= W, "strides %zu / %zu below the width %zu", raw_stride, out_stride, W);
  // (the kernel's offsets inside a source image are 32-bit)
  RSPL_CHECK_ARG(H * raw_stride < (size_t)1 << 31 && H * out_stride < (size_t)1 << 31 && raw_pitch <= (size_t)1 << 40 &&
                     out_pitch <= (size_t)1 << 40,
                 "rspl_rect_enqueue_device: stride or pitch too large");
  const size_t raw_image = (H - 1) * raw_stride + W, out_image = (H - 1) * out_stride + W;
  RSPL_CHECK_ARG(batch == 1 || (raw_pitch >= raw_image && out_pitch >= out_image),
                 "pitches %zu / %zu below an image (%zu / %zu bytes)", raw_pitch, out_pitch, raw_image, out_image);
  const uintptr_t r0 = (uintptr_t)d_raw, r1 = r0 + (batch - 1) * raw_pitch + raw_image;
  const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (batch - 1) * out_pitch + out_image;
  RSPL_CHECK_ARG(r1 <= o0 || o1 <= r0, "rspl_rect_enqueue_device: input and output ranges overlap");
  rect::Args a{};
  for (int b = 0; b < batch; b++) {
    RSPL_CHECK_ARG(cam_index[b] == 0 || cam_index[b] == 1, "cam_index[%d] = %d", b, cam_index[b]);
    a.cam_bits[b >> 5] |= (uint32_t)cam_index[b] << (b & 31);
  }
  a.tpitch = (uint32_t)rect::table_pitch((int)W);
  a.cam_pitch = H * (size_t)a.tpitch;
  a.table = h->table;
  a.src = d_raw;
  a.src_stride = (uint32_t)raw_stride;
  a.src_pitch = raw_pitch;
  a.dst = d_out;
  a.dst_stride = (uint32_t)out_stride;
  a.dst_pitch = out_pitch;
  a.H = (int)H;
  a.W = (int)W;
  a.batch = batch;
  a.dst_aligned = ((o0 | out_stride | out_pitch) & 3) == 0;
  RSPL_HIP(rect::remap(a, stream));
  return RSPL_OK;
}

}  // namespace

extern "C" int rspl_rect_enqueue_device(rspl_rect* h, int batch, const uint8_t* d_raw, size_t raw_stride,
                                        size_t raw_pitch, const int* cam_index, uint8_t* d_out, size_t out_stride,
                                        size_t out_pitch, void* stream) {
  RSPL_CHECK_ARG(h && batch >= 0, "rspl_rect_enqueue_device: bad argument");
  RSPL_CHECK_ARG(batch <= h->cfg.max_batch, "batch %d exceeds max_batch %d", batch, h->cfg.max_batch);
  if (batch == 0) return RSPL_OK;
  return enqueue(h, batch, d_raw, raw_stride, raw_pitch, cam_index, d_out, out_stride, out_pitch,
                 stream ? (hipStream_t)stream : h->stream);
}

extern "C" int rspl_rect_pair(rspl_rect* h, const uint8_t* left, const uint8_t* right, size_t stride,
                              uint8_t* left_rect, uint8_t* right_rect, size_t out_stride) {
  RSPL_CHECK_ARG(h && left && right && left_rect && right_rect, "rspl_rect_pair: NULL argument");
  const size_t H = h->cfg.height, W = h->cfg.width, px = H * W;
  RSPL_CHECK_ARG(stride >= W && out_stride >= W, "strides %zu / %zu below the width %zu", stride, out_stride, W);
  const uint8_t* in[2] = {left, right};
  uint8_t* res[2] = {left_rect, right_rect};
  RSPL_HIP(hipStreamSynchronize(h->stream));  // the pinned slot is free again
  for (int c = 0; c < 2; c++)
    for (size_t y = 0; y < H; y++) memcpy(h->h_raw + c * px + y * W, in[c] + y * stride, W);
  // raw images up by the copy kernel (copy_kernels.hip), remap in device memory, results back
  RSPL_HIP(upload_mapped(h->raw, h->h_raw_dev, 2 * px, h->stream));
  const int cams[2] = {0, 1};
  if (int rc = enqueue(h, 2, h->raw, W, px, cams, h->out, W, px, h->stream)) return rc;
  RSPL_HIP(hipMemcpyAsync(h->h_out, h->out, 2 * px, hipMemcpyDeviceToHost, h->stream));
  RSPL_HIP(hipStreamSynchronize(h->stream));
  for (int c = 0; c < 2; c++)
    for (size_t y = 0; y < H; y++) memcpy(res[c] + y * out_stride, h->h_out + c * px + y * W, W);
  return RSPL_OK;
}
