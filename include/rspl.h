/*
 * rspl.h -- C ABI of the MI355X-native SuperPoint -> SuperGlue -> local-BA hot path.
 *
 * Drop-in boundary for the reference's C++ API (llliuqingyu/RSPL-SLAM):
 *   SuperPoint      include/super_point.h:20-66     -> rspl_sp_*
 *   SuperGlue       include/super_glue.h:20-71      -> rspl_sg_*
 *   PointMatching   include/point_matching.h:7-18   -> rspl_pm_*
 *   LocalmapOptimization
 *                   include/g2o_optimization/g2o_optimization.h:15-19 -> rspl_ba_*
 *   FrameOptimization
 *                   include/g2o_optimization/g2o_optimization.h:20-22 -> rspl_frame_*
 *   SolvePnPWithCV  include/g2o_optimization/g2o_optimization.h:24    -> rspl_pnp_*
 *   Camera          include/camera.h:15-40          -> rspl_rect_*
 *   RCF             include/rcf.h:25-57             -> rspl_rcf_*
 * Plain pointers and sizes only; no Eigen / OpenCV / torch types.  Every call
 * returns RSPL_OK (0) or a negative RSPL_E_* code (rspl_last_error() has the
 * text).  Handles are NOT thread-safe: callers serialise, exactly as the
 * reference's MapBuilder::_gpu_mutex does (src/map_builder.cc:276-278).
 * Device memory is owned by the handle and allocated once at create time
 * (no per-call allocation, unlike Thirdparty/TensorRTBuffer buffers.h:209-233).
 *
 * Feature layout (SuperPoint output / SuperGlue input) is the reference's
 * Eigen::Matrix<double,259,Dynamic> column-major storage
 * (SuperPoint::process_output, src/super_point.cpp:285-319; resized at :298): feature i occupies doubles [259*i, 259*i+259):
 *   [0] score, [1] x, [2] y, [3..258] L2-normalised descriptor.
 */
#ifndef RSPL_H_
#define RSPL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSPL_OK 0
#define RSPL_E_ARG (-1)      /* bad argument / shape */
#define RSPL_E_WEIGHTS (-2)  /* weight blob missing or malformed */
#define RSPL_E_DEVICE (-3)   /* HIP runtime error */
#define RSPL_E_CAPACITY (-4) /* output or arena capacity exceeded */
#define RSPL_E_SOLVER (-5)   /* linear solve failed */

#define RSPL_FEATURE_ROWS 259

/* RSPL_PREC_FP16: fp16 MFMA operands, fp32 accumulation (the reference's TensorRT kFP16 engines,
 * src/super_point.cpp:97-99, src/super_glue.cpp:132).  RSPL_PREC_FP16X3 (SuperPoint only): split fp16 --
 * every activation and weight carried as hi + lo fp16, three fp16 MFMA products per step, fp32-grade
 * results (keypoint sets of the fp32 path) at the fp16 MFMA rate. */
enum { RSPL_PREC_FP32 = 0, RSPL_PREC_FP16 = 1, RSPL_PREC_FP16X3 = 2 };

const char* rspl_last_error(void);
const char* rspl_version(void);
/* ABI revision of the structs in this header; a consumer checks rspl_abi_version() ==
 * RSPL_ABI_VERSION at startup (the library writes caller-allocated structs such as
 * rspl_map_report at the size of ITS header).  2: rspl_map_report gained the stage times. */
#define RSPL_ABI_VERSION 2
int rspl_abi_version(void);

/* ------------------------------------------------------------------------ */
/* Runtime helpers (system ROCm HIP runtime).  Callers that share a process  */
/* with another HIP runtime (e.g. PyTorch's bundled one) use these instead,  */
/* so only one runtime ever touches the device.                              */
/* ------------------------------------------------------------------------ */
int rspl_device_count(int* count);
int rspl_set_device(int device);
int rspl_malloc(void** ptr, size_t bytes);
int rspl_free(void* ptr);
int rspl_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int rspl_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int rspl_memset(void* dst, int value, size_t bytes, void* stream);
int rspl_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int rspl_stream_create(void** stream);
/* high != 0: the device's highest stream priority (latency-critical chains) */
int rspl_stream_create_priority(void** stream, int high);
/* A stream whose kernels stay off reserve_cus CUs spread over the chip (HIP CU mask): the
 * throughput streams (SuperPoint / SuperGlue) leave those CUs free, so the latency-bound BA
 * chain never waits behind them for a CU slot. */
int rspl_stream_create_reserving(void** stream, int reserve_cus);
int rspl_stream_destroy(void* stream);
int rspl_stream_synchronize(void* stream);
int rspl_device_synchronize(void);
/* Cross-stream ordering without host synchronisation (pipelining SuperPoint of the
 * next frame beside SuperGlue of this one): record an event on one stream, make
 * another stream wait for it. */
int rspl_event_create(void** event);
int rspl_event_record(void* event, void* stream);
int rspl_stream_wait_event(void* stream, void* event);
int rspl_event_destroy(void* event);
/* HIP-event timer on a stream: rspl_timer_record(t, 0|1, stream) marks
 * start / stop; rspl_timer_elapsed_ms waits for stop and returns ms. */
typedef struct rspl_timer rspl_timer;
int rspl_timer_create(rspl_timer** t);
int rspl_timer_record(rspl_timer* t, int which, void* stream);
int rspl_timer_elapsed_ms(rspl_timer* t, float* ms);
void rspl_timer_destroy(rspl_timer* t);

/* ------------------------------------------------------------------------ */
/* SuperPoint: SuperPointConfig (include/read_configs.h:9-18) minus TRT-only */
/* fields; max_height/max_width size the device arena like the TRT profile   */
/* kMAX does (src/super_point.cpp:46-53).                                 */
/* ------------------------------------------------------------------------ */
typedef struct {
  int max_keypoints;         /* top-k; -1 keeps all, 0 yields no keypoints (top_k_keypoints, src/super_point.cpp:192-204);
                              * below -1 or above 16384 is RSPL_E_ARG */
  double keypoint_threshold; /* scores > threshold (src/super_point.cpp:154-165) */
  int remove_borders;        /* border in pixels (src/super_point.cpp:168-183) */
  int max_height;            /* arena sizing; H, W must be multiples of 8 */
  int max_width;
  int max_batch;             /* images per batched device call (>= 1) */
  int precision;             /* RSPL_PREC_FP32 (parity), RSPL_PREC_FP16 or RSPL_PREC_FP16X3 */
  int device;                /* HIP device ordinal */
} rspl_sp_config;

typedef struct rspl_sp rspl_sp;

/* SuperPoint::SuperPoint + build() (src/super_point.cpp:13-86).
 * weights_path: RSPLWT01 blob holding the reference state_dict
 * (convert2onnx/superpoint.py:86-105). */
int rspl_sp_create(const rspl_sp_config* cfg, const char* weights_path, rspl_sp** out);

/* SuperPoint::infer (src/super_point.cpp:104-135): rectified u8 image
 * (row stride in bytes) -> features[259 * capacity]; *n_out = keypoints. */
int rspl_sp_infer(rspl_sp* sp, const uint8_t* image, int height, int width, int stride,
                  double* features, int capacity, int* n_out);

/* Device-resident batched form: B images in device memory
 * (d_images + b*image_pitch), features to d_features + b*259*capacity,
 * counts to d_counts[b] (device int32).  stream may be NULL (handle stream). */
int rspl_sp_infer_device(rspl_sp* sp, const uint8_t* d_images, int batch, int height, int width,
                         int stride, size_t image_pitch, double* d_features, int capacity,
                         int32_t* d_counts, void* stream);

/* Intermediate maps of the last device call for image b (for tests):
 * scores [H*W] f32 after NMS, desc [256*(H/8)*(W/8)] f32 channel-major. */
int rspl_sp_debug_maps(rspl_sp* sp, int b, float* scores, float* desc);

/* Test hook: the device simple_nms (convert2onnx/superpoint.py:6-33, radius 4) of a host
 * score map [H][W] (any H, W within the arena) -> out [H][W]. */
int rspl_sp_debug_nms(rspl_sp* sp, const float* scores, int height, int width, float* out);

/* Test hook (RSPL_PREC_FP32 handles; otherwise RSPL_E_ARG): the tail every precision shares -- NMS with candidate
 * extraction, top-k and the fp32 descriptor sampler -- on host maps, through the same function and argument
 * construction as rspl_sp_infer_device, with the handle's own max_keypoints, keypoint_threshold and remove_borders.
 *   scores    f32 [B][H][W]              dense pre-NMS score maps, as the detector head leaves them
 *   desc      f32 [B][(H/8)*(W/8)][256]  dense descriptor maps in the device layout (cell-major)
 *   features  f64 [B][capacity][259]     in/out: uploaded as it stands (a test may prefill it), then downloaded;
 *                                        capacity = max_keypoints (16384 for -1, 1 for 0)
 *   counts [B] keypoints per image, cand_counts [B] the per-image candidate counter after NMS.
 * H, W multiples of 8 within the arena.  Keep-all (max_keypoints = -1) with more than 16384 candidates gives count 0
 * here exactly as rspl_sp_infer_device does, silently: only rspl_sp_infer reports it (RSPL_E_CAPACITY); cand_counts
 * shows it. */
int rspl_sp_debug_select(rspl_sp* sp, const float* scores, const float* desc, int batch, int height, int width,
                         double* features, int capacity, int32_t* counts, int32_t* cand_counts);

/* Test hook (RSPL_PREC_FP16 handles; otherwise RSPL_E_ARG): run ONE fp16 stage of the handle on host input,
 * through the same launcher call with the same arguments as rspl_sp_infer_device, and copy its output back.
 * height x width is the stage's OWN input level (the image for CONV1, the cell grid for the heads); fp16
 * activations travel as float.
 *   CONV1            in u8 [B][H][W]          -> out f32 [B][H/2][W/2][64]   (conv1a + conv1b + pool)
 *   CONV2A .. CONVPD in f32 [B][H][W][Cin]    -> out f32 [B][H or H/2][W or W/2][Cout] (NHWC; 2B, 3B pool)
 *   DET_HEAD         in f32 [B*H*W][512]      -> out f32 [B][8H][8W]         (dense score map)
 *   TAPS             in cells as DET_HEAD, scores f32 [B][8H][8W], kp int32 [B][kp_stride] flat pixel indices
 *                    (kp_counts[b] <= max_keypoints used) -> out f64 [B][max_keypoints][259], counts_out [B]
 * scores / kp / kp_counts / counts_out are read for TAPS only (NULL otherwise). */
enum {
  RSPL_SP_LAYER_CONV1 = 0, RSPL_SP_LAYER_CONV2A, RSPL_SP_LAYER_CONV2B, RSPL_SP_LAYER_CONV3A, RSPL_SP_LAYER_CONV3B,
  RSPL_SP_LAYER_CONV4A, RSPL_SP_LAYER_CONV4B, RSPL_SP_LAYER_CONVPD, RSPL_SP_LAYER_DET_HEAD, RSPL_SP_LAYER_TAPS
};
int rspl_sp_debug_layer(rspl_sp* sp, int stage, int batch, int height, int width, const void* in,
                        const float* scores, const int32_t* kp, const int32_t* kp_counts, int kp_stride,
                        void* out, int32_t* counts_out);

/* Per-stage device time (HIP events on the launch stream) summed over the calls
 * made since rspl_sp_profile(sp, 1).  Stages: 0 conv1a+conv1b+pool (fused),
 * 1 conv2a..conv4b, 2 convPa|convDa, 3 1x1 heads (softmax/d2s, L2 norm),
 * 4 NMS + candidates, 5 top-k, 6 descriptor sampling. */
#define RSPL_SP_STAGES 7
int rspl_sp_profile(rspl_sp* sp, int enable);
int rspl_sp_stage_times(rspl_sp* sp, float* ms, int* calls);

void rspl_sp_destroy(rspl_sp* sp);

/* ------------------------------------------------------------------------ */
/* SuperGlue: SuperGlueConfig (include/read_configs.h:20-28).               */
/* ------------------------------------------------------------------------ */
typedef struct {
  int image_width;   /* used by PointMatching::NormalizeKeypoints */
  int image_height;
  int max_keypoints; /* per image; arena sizing (the TRT profile allows 1024, src/super_glue.cpp:54-75) */
  int max_batch;     /* pairs per batched device call */
  int sinkhorn_iterations; /* 100 (convert2onnx/superglue.py:216) */
  int precision;
  int device;
} rspl_sg_config;

typedef struct rspl_sg rspl_sg;

int rspl_sg_create(const rspl_sg_config* cfg, const char* weights_path, rspl_sg** out);

/* SuperGlue::infer (src/super_glue.cpp:137-197): f0/f1 are 259 x n feature
 * matrices whose keypoints are ALREADY normalised (as PointMatching passes
 * them).  Outputs: indices0[n0], indices1[n1] (-1 = unmatched), mscores0[n0],
 * mscores1[n1]  (decode: src/super_glue.cpp:339-367). */
int rspl_sg_infer(rspl_sg* sg, const double* f0, int n0, const double* f1, int n1,
                  int32_t* indices0, int32_t* indices1, double* mscores0, double* mscores1);

/* Device-resident batched form.  Pair p reads f0 = d_feat0 + p*259*stride_feat,
 * n0 = n0[p] (DEVICE int32 counts, e.g. rspl_sp_infer_device's d_counts),
 * likewise image 1; writes d_idx0 + p*max_kp etc.
 * normalize != 0 applies PointMatching::NormalizeKeypoints on device first. */
int rspl_sg_infer_device(rspl_sg* sg, int batch, const double* d_feat0, const int* n0,
                         const double* d_feat1, const int* n1, int stride_feat, int normalize,
                         int32_t* d_idx0, int32_t* d_idx1, double* d_ms0, double* d_ms1,
                         void* stream);

/* As rspl_sg_infer_device, with the log-Sinkhorn and decode enqueued on post_stream (after
 * an event on stream): the next call's GNN on `stream` overlaps this call's Sinkhorn.
 * Results are complete when post_stream reaches this point.  The counts are snapshotted,
 * so the caller may reuse n0/n1 once `stream` has passed the call. */
int rspl_sg_infer_device2(rspl_sg* sg, int batch, const double* d_feat0, const int* n0,
                          const double* d_feat1, const int* n1, int stride_feat, int normalize,
                          int32_t* d_idx0, int32_t* d_idx1, double* d_ms0, double* d_ms1, void* stream,
                          void* post_stream);

/* Log-assignment Z [(n0+1)*(n1+1)] f32 of the last call, pair p (for tests).  n0, n1 are the counts of the
 * handle's last HOST call (rspl_sg_infer / rspl_pm_match): after a device-path call, size Z for those. */
int rspl_sg_debug_scores(rspl_sg* sg, int p, float* Z);

/* Sinkhorn health of the device paths.  The persistent log-Sinkhorn exchanges u / v between
 * co-resident workgroups with bounded spins; a pair whose exchange timed out sets a sticky
 * flag (its indices / scores are then invalid).  After synchronising the stream the results
 * were produced on, rspl_sg_status returns RSPL_OK, or RSPL_E_DEVICE with *pair_flags = the
 * bitmask of the failed pairs (bit 31 = any pair >= 31), and clears the flags.  rspl_sg_infer
 * and rspl_pm_match check it themselves. */
int rspl_sg_status(rspl_sg* sg, uint32_t* pair_flags);

/* Test hooks.  rspl_sg_debug_inject(sg, 1, limit): workgroup 0 of pair 0 reports an exchange
 * timeout at iteration 0 and every spin is bounded by `limit` polls (0 = the default), to
 * prove the failure reaches the caller.  rspl_sg_debug_sinkhorn: bins (alpha) + log_optimal_transport
 * (convert2onnx/superglue.py:185-205) of a host score matrix [n0][n1] -> Z [(n0+1)][(n1+1)].
 * rspl_sg_debug_decode: the device decode (src/super_glue.cpp:258-367) of a host Z. */
int rspl_sg_debug_inject(rspl_sg* sg, int inject, unsigned spin_limit);
int rspl_sg_debug_sinkhorn(rspl_sg* sg, const float* scores, int n0, int n1, float alpha, int iters, float* Z);
int rspl_sg_debug_decode(rspl_sg* sg, const float* Z, int n0, int n1, int32_t* indices0, int32_t* indices1,
                         double* mscores0, double* mscores1);
/* Test hook (RSPL_PREC_FP16 handles; otherwise RSPL_E_ARG): GNN layers [l0, l1) of the fp16 engine on host
 * descriptors, launched exactly as rspl_sg_infer_device launches them (fp16 shadow of X, the q / k / v prologue
 * with layer l0's weights, then one fused launch per layer, the same Q / K / V ping-pong parity), for the first
 * `batch` pairs.  X is the handle's WHOLE token buffer, f32 [2 * max_batch][max_keypoints][256] (set 2p = image 0
 * of pair p, 2p + 1 = image 1), uploaded, updated in place and copied back, so that a caller can see that nothing
 * outside the pairs it ran was written.  n0 / n1: host counts [batch].  Q (may be NULL): the next layer's q of
 * the batch's sets, fp16 bits [2 * batch][max_keypoints][256] (head-contiguous columns 64 h + d), written when
 * l1 < 18. */
int rspl_sg_debug_layers(rspl_sg* sg, int batch, float* X, const int32_t* n0, const int32_t* n1, int l0, int l1,
                         uint16_t* Q);

/* Test hook: the Sinkhorn kernel that rspl_sg_create chooses for a handle of (max_keypoints, max_batch) on a
 * device of cu_count CUs, under the RSPL_SG_SINK / RSPL_SG_SINK_G overrides as create reads them.  No device is
 * touched, except that cu_count 0 stands for the current device's CU count.
 * kind: 0 slab kernel, 1 slab kernel reading its slabs from global memory, 2 scaling form (nmax + 1 <= 448),
 * 3 scaling form (<= 640), 4 wide scaling form (<= 2112); groups: workgroups per pair; rows_per_wave: of the scaling
 * forms (0 for the slab kernel); ug / vg_granules: 8-byte exchange granules of the whole handle.  RSPL_E_ARG
 * where rspl_sg_create would refuse max_batch. */
typedef struct {
  int32_t kind, groups, rows_per_wave, reserved;
  uint64_t ug_granules, vg_granules;
} rspl_sg_sinkhorn_plan;
int rspl_sg_debug_sinkhorn_plan(int max_keypoints, int max_batch, int cu_count, rspl_sg_sinkhorn_plan* out);

/* Stages: 0 prep + keypoint encoder, 1 18 GNN layers, 2 final_proj + scores + bins,
 * 3 hand-over to the post stream (queueing behind the previous call's post work; no kernel),
 * 4 log-Sinkhorn (one kernel), 5 decode. */
#define RSPL_SG_STAGES 6
int rspl_sg_profile(rspl_sg* sg, int enable);
int rspl_sg_stage_times(rspl_sg* sg, float* ms, int* calls);

void rspl_sg_destroy(rspl_sg* sg);

/* ------------------------------------------------------------------------ */
/* PointMatching (src/point_matching.cc): normalise, SuperGlue, mutual check, */
/* DMatch(i, j, 1 - (ms0 + ms1)/2).  outlier_rejection (default off in the   */
/* reference) filters the matches through cv::findFundamentalMat(FM_RANSAC,  */
/* 3, 0.99) (:34-45) as rspl_fm_solve computes it, on an rspl_fm handle the  */
/* rspl_sg handle creates on first use (sized by its max_keypoints, freed by */
/* rspl_sg_destroy); the surviving matches stay in order.  Fewer than 7      */
/* matches, or no model: nothing is rejected.                                */
/* ------------------------------------------------------------------------ */
typedef struct {
  int32_t query_idx;
  int32_t train_idx;
  float distance;
} rspl_dmatch;

int rspl_pm_match(rspl_sg* sg, const double* f0, int n0, const double* f1, int n1,
                  rspl_dmatch* matches, int capacity, int* n_matches, int outlier_rejection);

/* ------------------------------------------------------------------------ */
/* Local bundle adjustment: LocalmapOptimization                            */
/* (src/g2o_optimization/g2o_optimization.cc:21-252).  Vertex ids of the    */
/* reference's std::maps are remapped to dense indices by the caller.       */
/* ------------------------------------------------------------------------ */
typedef struct {
  int n_cameras;
  const double* cameras;        /* [n][5] fx, fy, cx, cy, bf (include/camera.h:25-29) */

  int n_poses;
  const double* pose_q;         /* [n][4] rotation of T_wc, Eigen coeffs order (x, y, z, w) */
  const double* pose_p;         /* [n][3] translation of T_wc */
  const uint8_t* pose_fixed;    /* [n] Pose3d::fixed */

  int n_points;
  const double* points;         /* [n][3] world position */

  int n_lines;
  const double* lines;          /* [n][6] g2o::Line3D Pluecker (w, d) */

  int n_mono;                   /* MonoPointConstraint (types.h:54-78) */
  const int32_t* mono_pose;
  const int32_t* mono_point;
  const int32_t* mono_camera;   /* may be NULL -> camera 0 */
  const double* mono_obs;       /* [n][2] */

  int n_stereo;                 /* StereoPointConstraint (types.h:81-105) */
  const int32_t* stereo_pose;
  const int32_t* stereo_point;
  const int32_t* stereo_camera;
  const double* stereo_obs;     /* [n][3] u, v, u_right */

  int n_mono_line;              /* MonoLineConstraint (types.h:124-148) */
  const int32_t* mono_line_pose;
  const int32_t* mono_line_line;
  const int32_t* mono_line_camera;
  const double* mono_line_obs;  /* [n][4] x1 y1 x2 y2 */

  int n_stereo_line;            /* StereoLineConstraint (types.h:151-174) */
  const int32_t* stereo_line_pose;
  const int32_t* stereo_line_line;
  const int32_t* stereo_line_camera;
  const double* stereo_line_obs; /* [n][8] left x1 y1 x2 y2, right x1 y1 x2 y2 */

  /* OptimizationConfig (include/read_configs.h:50-56): chi2 thresholds; the
   * Huber deltas are (float)sqrt(threshold) (g2o_optimization.cc:77-78,125-126) */
  double th_mono_point, th_stereo_point, th_mono_line, th_stereo_line;
  int iterations_first;   /* 10 (g2o_optimization.cc:173) */
  int iterations_second;  /* 5  (g2o_optimization.cc:210) */
} rspl_ba_problem;

typedef struct {
  double* pose_q;     /* [n_poses][4] optimised T_wc rotation (x, y, z, w) */
  double* pose_p;     /* [n_poses][3] */
  double* points;     /* [n_points][3] */
  double* lines;      /* [n_lines][6] */
  uint8_t* mono_inlier;
  uint8_t* stereo_inlier;
  uint8_t* mono_line_inlier;
  uint8_t* stereo_line_inlier;
  double chi2_first;  /* robust chi2 at the end of the first optimize() */
  double chi2_second; /* chi2 at the end of the second optimize() */
  int iterations_done_first;
  int iterations_done_second;
} rspl_ba_result;

typedef struct {
  int max_poses;
  int max_points;
  int max_lines;
  int max_edges;      /* per edge type */
  int device;
} rspl_ba_config;

typedef struct rspl_ba rspl_ba;

int rspl_ba_create(const rspl_ba_config* cfg, rspl_ba** out);
int rspl_ba_local(rspl_ba* ba, const rspl_ba_problem* problem, rspl_ba_result* result);
void rspl_ba_destroy(rspl_ba* ba);
/* The reference's tracking thread (map_builder.cc:48-49, 188-276): rspl_ba_submit queues one local BA
 * call for the handle's native host thread, which runs the queued calls in order (rspl_ba_local each);
 * like the reference's feature thread it blocks while two calls are already waiting
 * (_tracking_data_buffer, map_builder.cc:176).  problem, its arrays and result must stay valid until
 * the call has run.  A queued call's inputs are read (staged) by a second host thread of the handle as
 * soon as a staging slot is free -- while the previous call still runs on the device -- so do not
 * modify a problem after submitting it.  rspl_ba_join waits until every queued call has run and returns the first failure
 * since the previous join (0: none), with the number of calls, their LM iterations (first + second
 * optimize) and their summed wall time in ms (each may be NULL).  Do not call rspl_ba_local on the
 * handle while calls are queued; rspl_ba_destroy runs the queued calls before it frees the handle. */
int rspl_ba_submit(rspl_ba* ba, const rspl_ba_problem* problem, rspl_ba_result* result);
int rspl_ba_join(rspl_ba* ba, long long* calls, long long* iterations, double* ms);
/* Run this handle's kernels only on the reserve_cus CUs that rspl_stream_create_reserving
 * streams leave free (0 = all CUs, highest stream priority: the default). */
int rspl_ba_use_reserved_cus(rspl_ba* ba, int reserve_cus);
/* Kernel timing (measurement): every `every`-th rspl_ba_local call (0: off) records HIP events on the
 * BA stream around each LM trial's two launches (device LM path); rspl_ba_kernel_times returns and
 * resets the totals -- ms[0] / launches[0]: Schur chunks + fused reduced-system solve, ms[1] /
 * launches[1]: update + cost + speculative linearisation -- over the trials that did work. */
int rspl_ba_kernel_timing(rspl_ba* ba, int every);
int rspl_ba_kernel_times(rspl_ba* ba, double* ms, long long* launches);
/* Per-call host timeline (measurement): the handle keeps the host timestamps of its last 4096 calls
 * (CLOCK_MONOTONIC seconds -- the clock of Python's time.perf_counter / time.monotonic on Linux).
 * Record of RSPL_BA_TRACE_W doubles: [0] submitted (rspl_ba_submit; rspl_ba_local: entry), [1] staging
 * started, [2] staging done, [3] device part started (tracking thread), [4] upload queued, [5] optimize(10)
 * stopped (mailbox read), [6] optimize(5) stopped, [7] call done (results written back), [8] staging slot,
 * [9] flags (1 staging slot, 2 edge-pair list, 4 pose-diagonal partials, 8 timing events: a buffer grown inside
 * the call; 16 optimize(5)'s setup ran from the speculative queue behind optimize(10)'s trials, 32 optimize(10)
 * needed trials beyond its first batch), [10] LM iterations, [11] 1 for rspl_ba_local, 0 for a submitted call.
 * rspl_ba_trace copies the oldest min(cap, recorded) records and clears the ring; *n = records copied. */
/* Line edges' Jacobians (EdgeSE3ProjectLine / EdgeStereoSE3ProjectLine do not override linearizeOplus, so
 * g2o differentiates them numerically: central difference, delta 1e-9).  0 (default): that central
 * difference; 1: its analytic delta -> 0 limit (truncation ~1e-18 relative; the central difference's own
 * cancellation noise, ~1e-7 relative, is absent -- results become smooth in the inputs). */
int rspl_ba_set_line_jacobian(rspl_ba* ba, int analytic);
#define RSPL_BA_TRACE_W 12
int rspl_ba_trace(rspl_ba* ba, double* out, int cap, int* n);
/* Test hook (host only, no device): the host staging of rspl_ba_local -- the edges of rank `rank` of
 * `nranks` (1: all) in landmark-CSR order -- with the host workers from par_edges edges (0: serial).
 * n_local = {local edges E, local point edges Ep}; lm_off [n_points + n_lines + 1]; per CSR position
 * k < E: type (0..3), pose, landmark (lines offset by n_points), camera, caller edge id (over the four
 * types in order), reduced pose id (-1: fixed or without edges); eobs: 4 doubles per point edge, then
 * 8 per line edge (arrays sized for all edges). */
int rspl_ba_debug_stage(const rspl_ba_problem* problem, int par_edges, int rank, int nranks, int* n_local,
                        int* lm_off, int8_t* etype, int* epose, int* elm, int* ecam, int* gmap, int* lpose,
                        double* eobs);
/* Test hooks (host only, no device): the Schur chunk geometry (ba::chunk_plan) of a window of n_landmarks
 * landmarks (points + lines) and n_poses optimised poses in a handle created for max_landmarks / max_poses.
 * chunks: Schur chunks of the window, grid: workgroups of the chunk kernel's launch (idle slots included),
 * ue_bpr: update workgroups per range when they follow the chunks' XCDs (else 0), slots: chunks the handle's
 * buffers hold.
 * rspl_ba_debug_chunk_geometry: per chunk c < chunks, chunks[6 c ...] = {pose pair, first landmark, end landmark
 * (clamped to n_landmarks), first chunk of its pose pair, end chunk of its pose pair, nominal end landmark};
 * order[vb] for vb < grid: the chunk that workgroup vb of the launch runs, -1 for an idle slot, -2 if the launch
 * order's geometry of that chunk disagrees with chunks[]. */
typedef struct {
  int32_t nchk, lmchunk, dsub, lmsub;
  int32_t chunks, grid, ue_bpr;
  int64_t slots;
} rspl_ba_chunk_plan;
int rspl_ba_debug_chunk_plan(int n_landmarks, int n_poses, int max_landmarks, int max_poses,
                             rspl_ba_chunk_plan* out);
int rspl_ba_debug_chunk_geometry(int n_landmarks, int n_poses, int max_landmarks, int max_poses, int32_t* chunks,
                                 int32_t* order);
/* Test hook (host only, no device): the segment offsets of the Schur chunks' edge-pair lists as the staging of
 * rspl_ba_local counts them for `problem` in a handle created for max_landmarks / max_poses -- pp_off[c] for
 * c <= *n_chunks (cap: ints of room): chunk c (rspl_ba_debug_chunk_geometry) owns pairs [pp_off[c], pp_off[c+1]),
 * one per (edge on the pair's first pose, edge on its second pose) of each landmark of its range. */
int rspl_ba_debug_pair_offsets(const rspl_ba_problem* problem, int max_landmarks, int max_poses, int32_t* pp_off,
                               int cap, int* n_chunks);
/* Test hooks (device) on the last completed unsharded rspl_ba_local call of the handle.
 * rspl_ba_debug_pairs: the edge-pair lists of its first optimize -- rebuild 0: as the call built them (*fused 1:
 * filled by the first pass against the staged offsets); rebuild 1: built again by the count / scan / fill launches
 * (the path of sharded handles and of windows beyond the device LM driver).  pp_off [*n_chunks + 1], pp:
 * {CSR position of the first pose's edge, of the second pose's edge, landmark, 0} per pair.
 * rspl_ba_debug_final: the inlier flags by the classify kernel's final pass, in the caller's edge order over the
 * four types; the final state on the device (T_dev [n_poses][8] T_cw: q w x y z, t, pad; X; L) and the T the
 * final kernel wrote for the host (T_out). */
int rspl_ba_debug_pairs(rspl_ba* ba, int rebuild, int32_t* pp_off, int cap_off, int32_t* pp, long long cap_pairs,
                        int* n_chunks, long long* n_pairs, int* fused);
int rspl_ba_debug_final(rspl_ba* ba, uint8_t* inlier, double* T_dev, double* T_out, double* X, double* L);

/* ------------------------------------------------------------------------ */
/* Landmark-sharded local BA: nranks handles -- one per  */
/* GPU (RCCL over xGMI), or several on one device (in-process group) -- each  */
/* call rspl_ba_local with the SAME problem.  Rank r keeps only the edges of  */
/* the landmarks it owns (landmark g owned by rank g % nranks: points first,  */
/* then lines, as in rspl_ba_problem), computes its Schur contribution       */
/* S_r = sum (Hpp - Hpl Hll^-1 Hlp) / b_r, and the ranks sum-all-reduce, per  */
/* LM trial, the reduced camera system (pose-pair blocks + gradients + the    */
/* landmark-inversion flag) and the trial's {chi2, LM scale, fail}; at        */
/* lambda-init the pose-block diagonals and each rank's landmark maximum.    */
/* Every rank factors the same reduced system, so the LM decisions agree.    */
/* Results are complete on every rank (owned landmarks and edge flags are    */
/* gathered by a final all-reduce).                                          */
/* ------------------------------------------------------------------------ */
/* in-place sum all-reduce of count doubles on a HIP stream (stream-ordered); 0 = ok */
typedef int (*rspl_allreduce_fn)(void* ctx, double* d_buf, size_t count, void* stream);
int rspl_ba_set_shard(rspl_ba* ba, int rank, int nranks, rspl_allreduce_fn allreduce, void* ctx);

/* RCCL communicator (librccl is loaded at first use).  Rank 0 makes the id, the
 * caller broadcasts its RSPL_COMM_ID_BYTES to the other ranks out of band
 * (e.g. torch.distributed), every rank creates its communicator. */
#define RSPL_COMM_ID_BYTES 128
typedef struct rspl_comm rspl_comm;
int rspl_comm_unique_id(uint8_t* id /* [RSPL_COMM_ID_BYTES] */);
int rspl_comm_create(const uint8_t* id, int rank, int nranks, int device, rspl_comm** out);
int rspl_comm_allreduce_sum(void* comm, double* d_buf, size_t count, void* stream);  /* an rspl_allreduce_fn */
void rspl_comm_destroy(rspl_comm* comm);
int rspl_ba_set_comm(rspl_ba* ba, rspl_comm* comm);

/* In-process group: nranks BA handles on ONE device, each driven by its own host
 * thread (a landmark-sharded solve inside one GPU; also how the sharded math is
 * tested on a single-GPU host).  The sum is formed in rank order on the device. */
typedef struct rspl_group rspl_group;
int rspl_group_create(int nranks, rspl_group** out);
void rspl_group_destroy(rspl_group* group);
int rspl_ba_set_group(rspl_ba* ba, rspl_group* group, int rank);

/* ------------------------------------------------------------------------ */
/* Tracking pose optimisation: FrameOptimization                            */
/* (src/g2o_optimization/g2o_optimization.cc:256-398, declared at           */
/* include/g2o_optimization/g2o_optimization.h:20-22; called per frame by   */
/* MapBuilder::FramePoseOptimization, src/map_builder.cc:583).  One pose     */
/* vertex, fixed world points, unary EdgeSE3ProjectXYZOnlyPose /            */
/* EdgeStereoSE3ProjectXYZOnlyPose edges with Huber kernels; 4 rounds of    */
/* optimize(10) from the initial pose with chi2 re-classification, kernels  */
/* dropped for the last round.  A batch of independent frames (one sequence */
/* each, or many sequences per GPU) runs in ONE kernel launch, one wavefront */
/* per frame.                                                               */
/* ------------------------------------------------------------------------ */
typedef struct {
  int n_cameras;
  const double* cameras;        /* [n][5] fx, fy, cx, cy, bf */
  double pose_q[4];             /* initial T_wc rotation (x, y, z, w) */
  double pose_p[3];             /* initial T_wc translation */
  int n_points;
  const double* points;         /* [n][3] world positions (Position3d, fixed) */
  int n_mono;                   /* MonoPointConstraint: id_point, id_camera, keypoint */
  const int32_t* mono_point;
  const int32_t* mono_camera;   /* may be NULL -> camera 0 */
  const double* mono_obs;       /* [n][2] */
  const uint8_t* mono_inlier_in;   /* Constraint::inlier on entry; NULL = all true (map_builder.cc:560) */
  int n_stereo;                 /* StereoPointConstraint */
  const int32_t* stereo_point;
  const int32_t* stereo_camera;
  const double* stereo_obs;     /* [n][3] u, v, u_right */
  const uint8_t* stereo_inlier_in;
  double th_mono_point, th_stereo_point;  /* OptimizationConfig (tracking) */
} rspl_frame_problem;

typedef struct {
  double pose_q[4];             /* optimised T_wc (x, y, z, w) */
  double pose_p[3];
  uint8_t* mono_inlier;         /* [n_mono] Constraint::inlier on exit (may be NULL) */
  uint8_t* stereo_inlier;
  int n_inliers;                /* FrameOptimization's return value */
  int rounds;                   /* optimize() rounds run (4, or 1 when < 10 edges) */
  int iterations[4];            /* LM iterations done per round */
  double chi2[4];               /* final (robust) chi2 per round */
} rspl_frame_result;

typedef struct {
  int max_batch;                /* frames per call */
  int max_edges;                /* total edges (mono + stereo) over a whole batch */
  int max_points;               /* total points over a whole batch */
  int device;
} rspl_frame_config;

typedef struct rspl_frame rspl_frame;

int rspl_frame_create(const rspl_frame_config* cfg, rspl_frame** out);
/* batch independent FrameOptimization calls; results[b] receives frame b.  Batches of more than 256
 * frames sum each frame's normal equations in another order (one wave per frame instead of four):
 * results then differ from a small batch's in the last bits, within the oracle tolerances. */
int rspl_frame_optimize(rspl_frame* h, const rspl_frame_problem* problems, int batch, rspl_frame_result* results);
void rspl_frame_destroy(rspl_frame* h);

/* ------------------------------------------------------------------------ */
/* SolvePnPWithCV (src/g2o_optimization/g2o_optimization.cc:402-461; declared at */
/* include/g2o_optimization/g2o_optimization.h:24, called per frame by          */
/* MapBuilder::FramePoseOptimization, src/map_builder.cc:515): the RANSAC of    */
/* cv::solvePnPRansac (5-point EPnP hypotheses, 100 iterations, 20 px, 0.99,    */
/* SOLVEPNP_ITERATIVE refinement on the inliers), zero distortion               */
/* (camera.cc:145-147).  The correspondences are the caller's already-filtered  */
/* (map point, keypoint) pairs (:417-431); the caller maps inlier slots back to  */
/* map-point ids (:452-457).  A batch of frames is one launch, one workgroup per */
/* frame, the hypotheses of a frame solved side by side.                        */
/* ------------------------------------------------------------------------ */
typedef struct {
  double fx, fy, cx, cy;        /* Camera::GetCamerMatrix */
  int n;                        /* correspondences; < 8 -> 0 inliers (:433) */
  const double* points;         /* [n][3] map points (world), rounded to float like cv::Point3f */
  const double* keypoints;      /* [n][2] pixels, rounded to float like cv::Point2f */
  int iterations;               /* 100 (:439); at most 128 */
  double reprojection_error;    /* 20.0 px */
  double confidence;            /* 0.99 */
} rspl_pnp_problem;

typedef struct {
  double Rwc[9];                /* row-major Rwc = Rcw^T (:447-449); valid when n_inliers > 0 */
  double twc[3];                /* -Rwc tcw */
  uint8_t* inlier;              /* [n] inlier mask of the RANSAC model (may be NULL) */
  int n_inliers;                /* SolvePnPWithCV's return value (cv_inliers.rows) */
  int hypotheses;               /* RANSAC iterations evaluated (adaptive) */
} rspl_pnp_result;

typedef struct {
  int max_batch;
  int max_points;               /* correspondences over a whole batch */
  int device;
} rspl_pnp_config;

typedef struct rspl_pnp rspl_pnp;

int rspl_pnp_create(const rspl_pnp_config* cfg, rspl_pnp** out);
int rspl_pnp_solve(rspl_pnp* h, const rspl_pnp_problem* problems, int batch, rspl_pnp_result* results);
void rspl_pnp_destroy(rspl_pnp* h);
/* debug (parity tests): frame `frame` of the last rspl_pnp_solve -- every hypothesis' inlier
   count (-1: the minimal solver failed) and R (row-major) | t, up to `max` hypotheses; returns
   the frame's hypothesis count or a negative error */
int rspl_pnp_debug_hypotheses(rspl_pnp* h, int frame, int max, int32_t* counts, double* poses);

/* ------------------------------------------------------------------------ */
/* Map-side local BA: the keyframe / map-point / map-line */
/* graph of the reference's Map (include/map.h:15-52) and                   */
/* Map::LocalMapOptimization (src/map.cc:537-808) around rspl_ba_local:      */
/* window selection (SearchNeighborFrames, :471-525; one extra fixed frame,  */
/* :593-606), the constraints that enter the BA (:608-707), outlier removal  */
/* (RemoveOutliers / RemoveLineOutliers, :712-757, :818-895), the            */
/* covisibility update (UpdateFrameConnection, :897-937), write-back and     */
/* line endpoints (UppdateMapline, :121-177).  Frames, map points and map    */
/* lines are named by id (shared_ptr -> id; a frame's map-point / map-line   */
/* slot holds an id or -1).  Equal covisibility weights are ordered by frame */
/* id (the reference: by FramePtr address, i.e. allocation order).          */
/* ------------------------------------------------------------------------ */
typedef struct {
  const double* camera;          /* [5] fx fy cx cy bf (Map::_camera) */
  /* OptimizationConfig (_backend_optimization_config, configs_euroc.yaml:56-61) */
  double th_mono_point, th_stereo_point, th_mono_line, th_stereo_line;
  int iterations_first, iterations_second;
} rspl_map_config;

typedef struct {
  int frame_id;
  double timestamp;
  const double* Twc;             /* [16] row-major 4x4 pose (Frame::GetPose) */
  int n_keypoints;
  const double* keypoints;       /* [n][3] x, y (features rows 1-2), u_right (< 0: mono) */
  int n_lines;
  const double* lines_left;      /* [n_lines][4] Frame::_lines */
  const double* lines_right;     /* [n_lines][4] Frame::_lines_right (may be NULL) */
  const uint8_t* lines_right_valid; /* [n_lines] (may be NULL: none) */
  const int32_t* pol_offsets;    /* [n_lines + 1] CSR of Frame::_points_on_lines (may be NULL) */
  const int32_t* pol_points;     /*   keypoint index */
  const double* pol_dist;        /*   distance */
  int parent_id;                 /* Frame::_parent (-1: none) */
} rspl_map_keyframe;

typedef struct {
  int n_poses, n_fixed, n_points, n_lines;
  int n_mono, n_stereo, n_mono_line, n_stereo_line;
  int n_point_outliers, n_line_outliers;
  double chi2_first, chi2_second;
  int iterations_first, iterations_second;
  /* host wall time of the call's stages, microseconds: window + constraint assembly, the GPU
   * LocalmapOptimization (rspl_ba_local incl. staging), outlier removal + covisibility + write-back */
  double assembly_us, ba_us, finish_us;
} rspl_map_report;

enum { RSPL_MAP_UNTRIANGULATED = 0, RSPL_MAP_GOOD = 1, RSPL_MAP_BAD = 2 };  /* Mappoint::Type */

typedef struct rspl_map rspl_map;
int rspl_map_create(const rspl_map_config* cfg, rspl_map** out);        /* Map::Map */
void rspl_map_destroy(rspl_map* m);
/* Map::InsertKeyframe's bookkeeping (_keyframes, _keyframe_ids; map.cc:24-28) */
int rspl_map_add_keyframe(rspl_map* m, const rspl_map_keyframe* kf);
int rspl_map_add_mappoint(rspl_map* m, int id, const double* p, int type);       /* Map::InsertMappoint */
int rspl_map_add_mapline(rspl_map* m, int id, const double* line3d, int type);   /* Map::InsertMapline */
/* Mappoint::AddObverser + Frame::InsertMappoint; Mapline::AddObverser + Frame::InsertMapline */
int rspl_map_add_point_observation(rspl_map* m, int point_id, int frame_id, int keypoint_idx);
int rspl_map_add_line_observation(rspl_map* m, int line_id, int frame_id, int line_idx);
/* bulk forms: n map points (types may be NULL: Good); n observations of frame_id */
int rspl_map_add_mappoints(rspl_map* m, int n, const int32_t* ids, const double* p, const int32_t* types);
int rspl_map_add_point_observations(rspl_map* m, int frame_id, int n, const int32_t* point_ids,
                                    const int32_t* keypoints);
int rspl_map_update_connections(rspl_map* m, int frame_id);             /* Map::UpdateFrameConnection */
/* Map::LocalMapOptimization(new_frame) with the local BA on `ba` (GPU) */
int rspl_map_local_optimization(rspl_map* m, int frame_id, rspl_ba* ba, rspl_map_report* report);
/* the same window / constraint selection without the BA (no write-back, no outlier removal) */
int rspl_map_assemble(rspl_map* m, int frame_id, rspl_map_report* report);
/* the rest of LocalMapOptimization (outlier removal, covisibility update, write-back, line
 * endpoints; map.cc:712-802) applied to the last assembled problem with a supplied BA result */
int rspl_map_finish(rspl_map* m, const rspl_ba_result* result, rspl_map_report* report);
/* the last assembled problem: ids of the dense poses / points / lines (ascending, the
 * LocalmapOptimization vertex order), and per constraint type t (mono, stereo, mono line, stereo
 * line) the dense pose / landmark index and the observation (2 / 3 / 4 / 8 doubles) */
int rspl_map_last_problem(const rspl_map* m, int32_t* pose_ids, uint8_t* pose_fixed, int32_t* point_ids,
                          int32_t* line_ids, int32_t* const* c_pose, int32_t* const* c_lm, double* const* c_obs);
int rspl_map_get_keyframe(const rspl_map* m, int frame_id, double* Twc, int* n_connections);
/* Frame::GetOrderedConnections(-1): ascending (weight, frame id) */
int rspl_map_get_connections(const rspl_map* m, int frame_id, int32_t* ids, int32_t* weights, int cap, int* n);
int rspl_map_get_mappoint(const rspl_map* m, int id, double* p, int* type, int* n_observers, int32_t* frames,
                          int32_t* keypoints, int cap);
int rspl_map_get_mapline(const rspl_map* m, int id, double* line3d, int* type, int* n_observers,
                         double* endpoints, int* endpoints_valid);
int rspl_map_get_frame_slots(const rspl_map* m, int frame_id, int32_t* mappoints, int32_t* maplines);
/* Map::SaveKeyframeTrajectory (map.cc:1007-1024): TUM "t tx ty tz qx qy qz qw", %.9f */
int rspl_map_save_trajectory(const rspl_map* m, const char* path);

/* ------------------------------------------------------------------------------------------ */
/* Line front end: the detector (cv::resize + FLD, restated, parity         */
/* unpinned), then the merge passes, the point-line assignment and the line matching.  The RCF */
/* edge net is not rebuilt (no weights): its edge map is the detector's input.                */
/* ------------------------------------------------------------------------------------------ */

/* LineDetector::LineExtractor after fld->detect (src/line_processor.cc:460-490): segments
 * [n][4] float as FLD returns them on the half-size image -> lines [n_out][4] double at full
 * size; do_merge runs MergeLines(0.05, 5, 15), FilterShortLines(30), MergeLines(0.03, 3, 50),
 * FilterShortLines(60) (:492-665, 11-24).  Host code (a sequential clustering); *n_out is set
 * even when it exceeds capacity (RSPL_E_CAPACITY). */
int rspl_line_extract(const float* segments, int n, int do_merge, double* lines, int capacity, int* n_out);

typedef struct rspl_lines rspl_lines;
typedef struct rspl_lines_config {
  int max_lines;   /* lines per image, <= 1024 */
  int max_points;  /* keypoints per image, <= 4096 */
  int max_pairs;   /* point-line pairs per image (the sum of the std::map sizes) */
  int max_matches; /* point matches per MatchLines call */
  int device;
} rspl_lines_config;

int rspl_lines_create(const rspl_lines_config* cfg, rspl_lines** out);
void rspl_lines_destroy(rspl_lines* h);
/* AssignPointsToLines(lines, points, relation) (src/line_processor.cc:163-216) on the GPU.
 * lines [n_lines][4] double; features = the 259 x N column-major keypoint records (x, y = rows
 * 1, 2).  relation as CSR: line i's points are point_idx[offsets[i] .. offsets[i+1]) in
 * ascending index order (the std::map<int, double> order) with dist[] = the map values. */
int rspl_lines_assign(rspl_lines* h, const double* lines, int n_lines, const double* features, int n_points,
                      int* offsets, int* point_idx, double* dist, int capacity);
/* MatchLines(points_on_line0, points_on_line1, point_matches, point_num0, point_num1, line_matches)
 * (src/line_processor.cc:221-283) on the GPU.  The relations as rspl_lines_assign returns them
 * (the distances are not needed); matches [n_matches][2] = (queryIdx, trainIdx);
 * line_matches [n_lines0]: the matched line of image 1, or -1. */
int rspl_lines_match(rspl_lines* h, const int* offsets0, const int* idx0, int n_lines0, const int* offsets1,
                     const int* idx1, int n_lines1, const int* matches, int n_matches, int n_points0, int n_points1,
                     int* line_matches);
/* The line part of Frame::AddLeftFeatures + Frame::AddRightFeatures (src/frame.cc:124-129,
 * 150-196): the stereo matches inside the disparity window (camera_limits = {MinXDiff,
 * MaxXDiff, MaxYDiff}, frame.cc:157-167), both images' point-line assignments (one launch),
 * MatchLines -> per left line the right line and its validity (line_matches[i] > 0, as the
 * reference tests it).  *n_kept_matches = the filtered stereo matches' count. */
int rspl_lines_stereo(rspl_lines* h, const double* lines_left, int n_left, const double* features_left,
                      int n_points_left, const double* lines_right, int n_right, const double* features_right,
                      int n_points_right, const int* stereo_matches, int n_matches, const double* camera_limits,
                      double* lines_right_out, uint8_t* lines_right_valid, int* n_kept_matches);
/* Device-resident rspl_lines_stereo for a GPU pipeline: lines (device [n][4] doubles), the
 * SuperPoint device features [2][feat_cap][259] (image 0 left, 1 right) with their device counts
 * [2], SuperGlue's device match index of each left keypoint (right keypoint or -1); outputs the
 * right line and validity per left line in device memory.  Stream-ordered: no host copy, no sync.
 * A point-line overflow of max_pairs leaves every line unmatched; rspl_lines_status reports it
 * once the stream has completed. */
int rspl_lines_stereo_device(rspl_lines* h, const double* d_lines_left, int n_left, const double* d_lines_right,
                             int n_right, const double* d_features, int feat_cap, const int32_t* d_counts,
                             const int32_t* d_match_idx, const double* camera_limits, double* d_lines_right_out,
                             uint8_t* d_lines_right_valid, void* stream);
int rspl_lines_status(rspl_lines* h, int* overflow);

/* LineDetector's detector (src/line_processor.cc:455-466): cv::resize(image, 0.5, 0.5,
 * INTER_LINEAR) and cv::ximgproc::FastLineDetector(length_threshold, distance_threshold,
 * canny_th1, canny_th2, canny_aperture_size, do_merge = false)->detect on the half image, as the
 * reference runs it on the RCF edge map (map_builder.cc:286, 327).  FLD is OpenCV contrib (not
 * vendored, absent): restated (oracle/fld_ref.py), parity unpinned.  The resize, the Sobel
 * gradients and Canny's non-maximum suppression / thresholds run on the GPU; hysteresis, chaining
 * and segment fitting on the host.  segments [n][4] float (x1 y1 x2 y2) on the HALF image, as
 * fld->detect returns them (rspl_line_extract scales and merges); even image sizes; *n_out is set
 * even when it exceeds capacity (RSPL_E_CAPACITY). */
typedef struct {
  int length_threshold;          /* 10 (configs/configs_euroc.yaml:31) */
  double distance_threshold;     /* 1.414213562 */
  double canny_th1, canny_th2;   /* 200, 250 */
  int canny_aperture_size;       /* 3 (the only size supported) */
} rspl_fld_config;
int rspl_lines_detect(rspl_lines* h, const uint8_t* image, int H, int W, int stride, const rspl_fld_config* cfg,
                      float* segments, int capacity, int* n_out);
/* LineDetector::LineExtractor (src/line_processor.cc:460-490) asynchronously: rspl_lines_detect +
 * rspl_line_extract (x2 scale, the merge passes when do_merge) on a native worker thread of the handle,
 * as the reference runs its line threads beside the point thread (map_builder.cc:285-290, 325-337).
 * The image must stay valid until rspl_lines_extract_wait returns; one job in flight per handle, and
 * no other call on the handle meanwhile.  _wait blocks for the job and writes lines [n][4] (full-size
 * x1 y1 x2 y2) and, when job_us is not NULL, the job's own duration on the worker (microseconds);
 * *n_out is set even when it exceeds capacity (RSPL_E_CAPACITY). */
int rspl_lines_extract_async(rspl_lines* h, const uint8_t* image, int H, int W, int stride,
                             const rspl_fld_config* cfg, int do_merge);
int rspl_lines_extract_wait(rspl_lines* h, double* lines, int capacity, int* n_out, double* job_us);
/* the same join, the lines copied into DEVICE memory d_lines [capacity][4] in stream order (from the
 * handle's pinned result buffer; no host synchronisation with the stream) -- the feed of
 * rspl_lines_stereo_device */
int rspl_lines_extract_wait_device(rspl_lines* h, double* d_lines, int capacity, int* n_out, double* job_us,
                                   void* stream);
/* debug (parity tests): the last rspl_lines_detect's half image and Canny classes (2 strong, 0
 * candidate, 1 none) for an H x W input, [H/2][W/2] each */
int rspl_lines_debug_canny(rspl_lines* h, int H, int W, uint8_t* half, uint8_t* cls);

/* The same detector, device-resident: `batch` (<= 2) u8 device images laid out as rspl_rcf_infer_device
 * writes them (image b at d_images + b * pitch, row stride `stride`, both in bytes) -> d_segments
 * [batch][capacity][4] float on the HALF image and d_counts [batch], both in device memory.  After the Canny
 * classes, hysteresis, 8-connected component labels, the chain walk (one lane per component), the segment fit
 * (one lane per chain) and the order by (seed, index within the chain) run as launches on `stream` (NULL: the
 * handle's): the segments, their count, order and orientation are rspl_lines_detect's; the endpoints come
 * from the device's fp64 atan2 / cos / sin and may differ from it by one float32 ulp.  Stream-ordered, never
 * waits for the device (the first call, and a larger image than any before, allocate scratch); calls on one
 * handle share that scratch and must be ordered among themselves.  d_counts[b] is the full count, the first
 * `capacity` segments are written.  RSPL_E_ARG, before any device call, for: batch outside [1, 2], odd sizes
 * or sizes below 4, stride < W, pitch < stride * (H - 1) + W, a half image whose two bitmasks
 * (H/2 * ceil(W/2 / 32) * 8 bytes) exceed the 147456-byte LDS budget (1920 x 1080 needs 129600).  An image
 * with more than 32768 edge pixels yields count 0 and status bit 1. */
int rspl_lines_detect_device(rspl_lines* h, const uint8_t* d_images, int batch, int H, int W, size_t stride,
                             size_t pitch, const rspl_fld_config* cfg, float* d_segments, int capacity,
                             int32_t* d_counts, void* stream);
/* the last rspl_lines_detect_device's overflow bits, OR-ed over its images, once its stream has completed:
 * 1 more than 32768 edge pixels, 2 more segments than `capacity`, 4 an internal loop bound was hit */
#define RSPL_FLD_ST_EDGE_PIXELS 1
#define RSPL_FLD_ST_SEGMENTS 2
#define RSPL_FLD_ST_LOGIC 4
int rspl_lines_detect_status(rspl_lines* h, int* status);
/* rspl_lines_extract_async with a device image: an event on `stream`, the device detector on the handle's own
 * stream behind it, its count and segments (at most 4096) copied to pinned memory, rspl_line_extract on the
 * worker.  Returns without waiting for the device; the image must stay valid until the job is waited for with
 * rspl_lines_extract_wait / _wait_device, whose job_us then spans submit to the worker's end. */
int rspl_lines_extract_async_device(rspl_lines* h, const uint8_t* d_image, int H, int W, size_t stride,
                                    const rspl_fld_config* cfg, int do_merge, void* stream);
/* debug (parity tests).  _hysteresis: a host class map [hh][hw] (2 strong, 0 candidate, 1 none) through the
 * hysteresis kernel -> edge bytes (0 / 255) after the corner zeroing.  _chains: a host edge map through the
 * label and walk kernels -> the chains sorted by seed: seeds [n] (pixel index), offsets [n + 1], points
 * [offsets[n]][2] (x, y); *n_chains is set even when a capacity is exceeded (RSPL_E_CAPACITY).
 * _fld_host: the host detector from an edge map, with no handle and no device: a sequential walk of `edges`,
 * then fit, filters and orientation against `half` -> segments as rspl_lines_detect orders them.
 * _fld_classes: the whole host half of rspl_lines_detect, likewise: a class map [hh][hw] through hysteresis and
 * the corner zeroing, then as _fld_host; *n_out is the count also when it exceeds `capacity`.
 * _fld_stats: image b's counters of the last device detection: edge pixels, components, chains, segments,
 * hysteresis passes, largest component, the walk's iteration count (its busiest lane), status.
 * _fld_profile / _fld_stage_ms: with profiling on, events around the stages of each rspl_lines_detect_device;
 * stage_ms waits for the last call and returns Canny classes, hysteresis, labels, walk, fit, order (ms). */
int rspl_lines_debug_hysteresis(rspl_lines* h, const uint8_t* cls, int hh, int hw, uint8_t* edges);
int rspl_lines_debug_chains(rspl_lines* h, const uint8_t* edges, int hh, int hw, int32_t* seeds, int32_t* offsets,
                            int32_t* points, int cap_chains, int cap_points, int* n_chains);
int rspl_lines_debug_fld_host(const uint8_t* half, const uint8_t* edges, int hh, int hw, const rspl_fld_config* cfg,
                              float* segments, int capacity, int* n_out);
int rspl_lines_debug_fld_classes(const uint8_t* half, const uint8_t* cls, int hh, int hw, const rspl_fld_config* cfg,
                                 float* segments, int capacity, int* n_out);
int rspl_lines_debug_fld_stats(rspl_lines* h, int b, int32_t* stats);
int rspl_lines_debug_fld_profile(rspl_lines* h, int enable);
int rspl_lines_debug_fld_stage_ms(rspl_lines* h, float* ms);

/* ------------------------------------------------------------------------ */
/* The tracking step itself: MapBuilder::TrackFrame + FramePoseOptimization  */
/* (src/map_builder.cc:448-611) for a batch of independent frames, from      */
/* SuperGlue's device indices to the pose and the track ids, as ONE          */
/* stream-ordered chain of launches with no host work in between:            */
/*   gather   mutual check (src/point_matching.cc:24-31), keyframe map-point */
/*            lookup, the ordered compaction into PnP correspondences and    */
/*            FrameOptimization edges, PnP's RANSAC subsets                  */
/*   PnP      the kernels of rspl_pnp_solve (100 iterations, 20 px, 0.99)    */
/*   seed     the 0.5 m / min_num_match gate (:517-521), T_wc -> T_cw        */
/*   optimise the kernel of rspl_frame_optimize                              */
/*   write-back  pose, track ids, kept matches (:586-608, :472-488)          */
/* rspl_track_enqueue never waits for the device; rspl_track_fetch waits for */
/* the one event the enqueue recorded.  Line tracking (MatchLines, :455, the  */
/* id copy of :490-501) and MapBuilder::AddKeyframe's decision (:616-636) are */
/* one more launch behind the write-back: rspl_track_enqueue_ext (below).    */
/* ------------------------------------------------------------------------ */
typedef struct {
  int max_batch;      /* frames per enqueue; also the number of keyframe slots */
  int max_keypoints;  /* keypoints per frame and per keyframe */
  int device;
} rspl_track_config;

#define RSPL_TRACK_NO_MAPPOINT 0   /* the keyframe keypoint has no map point */
#define RSPL_TRACK_GOOD 1          /* Mappoint::IsValid (src/mappoint.cc:51) */
#define RSPL_TRACK_NOT_GOOD 2      /* a map point that is not Good: matched, never an edge */

typedef struct {
  int slot;                     /* keyframe table (rspl_track_set_keyframe) */
  const double* d_features;     /* DEVICE SuperPoint records [cap][259] of the current frame (x, y = rows 1, 2) */
  const int32_t* d_n1;          /* DEVICE keypoint count of the current frame (clamped to max_keypoints) */
  const int32_t* d_idx0;        /* DEVICE SuperGlue indices0 [n0]: keyframe -> current */
  const int32_t* d_idx1;        /* DEVICE SuperGlue indices1 [n1]: current -> keyframe */
  const double* d_u_right;      /* DEVICE [n1] right-image u (> 0: a stereo edge), or NULL: every edge is mono */
  double fx, fy, cx, cy, bf;
  double last_Twc[16];          /* _last_frame->GetPose(), row-major 4x4 */
  double th_mono_point, th_stereo_point;  /* OptimizationConfig (tracking) */
  int min_num_match;            /* keyframe.min_num_match (configs/configs_euroc.yaml:43: 10) */
} rspl_track_frame;

typedef struct {
  double pose_q[4];             /* T_wc (x, y, z, w): the optimised pose when pose_set, else the last pose */
  double pose_p[3];
  int pose_set;                 /* n_inliers > min_num_match (:586) */
  int n_inliers;                /* FrameOptimization's return value = TrackFrame's */
  int n_pnp_inliers;            /* SolvePnPWithCV's return value */
  int pnp_used;                 /* 1: PnP's pose seeded the optimisation, 0: the last pose did */
  int n_keypoints;              /* the current frame's keypoint count as the device read it */
  int n_matches;                /* mutual matches */
  int n_kept;                   /* matches left after the removal of :472-488 */
  int n_mono, n_stereo;         /* edges */
  int rounds;                   /* as rspl_frame_result */
  int iterations[4];
  double chi2[4];
  /* per current keypoint, caller arrays of max_keypoints entries (each may be NULL); the first
   * n_keypoints are written */
  int32_t* match_kf;            /* the mutual partner in the keyframe before filtering, or -1 */
  int32_t* track_id;            /* the track id assigned (SetTrackId, :477), or -1.  As in the reference a
                                 * match survives only with inliers[idx1] > 0, strictly: a match whose
                                 * keyframe keypoint carries track id 0 is dropped */
  uint8_t* kept;                /* 1: the match stays in `matches` */
} rspl_track_result;

/* debug (parity tests): the intermediate stages of frame `frame` of the last enqueue, read back
 * after it completed.  Every pointer may be NULL.  K = max_keypoints. */
typedef struct {
  int n_corr;                   /* correspondences = edges */
  int n_mono, n_stereo;
  int32_t* corr_kp;             /* [K] PnP correspondence slot -> current keypoint (ascending) */
  int32_t* edge_kp;             /* [K] edge slot -> current keypoint (mono first, then stereo) */
  double* pnp_points;           /* [K][3] as PnP reads them (float-rounded) */
  double* pnp_keypoints;        /* [K][2] */
  double* edges;                /* [K][12] X[3], obs[3], cam[5], stereo -- the edge records */
  int n_subsets;                /* RANSAC subsets generated (0 when n_corr < 8) */
  int32_t* subsets;             /* [128][5] */
  double pnp_Rwc[9], pnp_twc[3];
  int pnp_n_inliers, pnp_hypotheses;
  uint8_t* pnp_inlier;          /* [K] per correspondence slot */
  double seed_q[4], seed_p[3];  /* the T_wc FrameOptimization started from (x, y, z, w) */
  int pnp_used;
  uint8_t* edge_inlier;         /* [K] FrameOptimization's flag per edge slot */
} rspl_track_debug;

typedef struct rspl_track rspl_track;

int rspl_track_create(const rspl_track_config* cfg, rspl_track** out);
void rspl_track_destroy(rspl_track* h);
/* The keyframe's table for slot `slot` (0 <= slot < max_batch): per keypoint j < n0 its map point's
 * world position points[3 j ..], state[j] (RSPL_TRACK_*) and track_id[j] (Frame::GetTrackId).  Host
 * arrays, copied before the call returns; the upload is asynchronous on `stream` (NULL: the
 * handle's), so enqueue on the same stream or order the streams with an event.  Call it again after
 * a local BA moved the points. */
int rspl_track_set_keyframe(rspl_track* h, int slot, int n0, const double* points, const uint8_t* state,
                            const int32_t* track_id, void* stream);
/* Enqueue the chain for frames[0 .. batch) on `stream` (NULL: the handle's; it may be the stream
 * SuperGlue's outputs are produced on).  Everything the host knows (batch, slots, thresholds, NULL
 * pointers) is checked before the first launch; device pointers are checked for NULL only.  No
 * host synchronisation.  One enqueue is in flight per handle: fetch before the next. */
int rspl_track_enqueue(rspl_track* h, int batch, const rspl_track_frame* frames, void* stream);
/* Wait for the last enqueue and copy its results out: results[b] receives frame b. */
int rspl_track_fetch(rspl_track* h, rspl_track_result* results);
int rspl_track_debug_stage(rspl_track* h, int frame, rspl_track_debug* out);
/* The DEVICE arrays of keyframe slot `slot` (points [max_keypoints][3], state, track id), for a producer
 * on the device (rspl_kf_enqueue's d_table_*); sets the slot's keypoint count to n0 as
 * rspl_track_set_keyframe does.  The producer and rspl_track_enqueue must be stream-ordered.  The
 * arrays can be read back with rspl_memcpy_d2h. */
int rspl_track_keyframe_table(rspl_track* h, int slot, int n0, double** d_points, uint8_t** d_state,
                              int32_t** d_track_id);

/* --- the tracking step's line side and keyframe decision ------------------------------------ */
/* The rest of MapBuilder::TrackFrame and what follows it for a tracked frame, as ONE more launch
 * behind the write-back of the chain above:
 *   line tracking   MatchLines between the keyframe's and the frame's points-on-lines
 *                   (src/map_builder.cc:450-455), fed with the matches BEFORE the removal of
 *                   :472-488 -- the pairs (match_kf[i], i) -- and the keyframe slot's n0 / the
 *                   frame's n1 as point counts; then the copy of the keyframe's line track ids and
 *                   map lines to the matched lines (:490-501).  Line j of the frame receives the id
 *                   and the map line of keyframe line i iff line_matches[i] == j and that id is
 *                   >= 0: id 0 IS propagated (unlike the points' `> 0`), the map line is copied
 *                   even when it is -1, everything else is -1.
 *   the decision    MapBuilder::AddKeyframe (:616-636) and _last_frame_track_well (:240) on the pose
 *                   and n_inliers rspl_track_result reports (the last pose when !pose_set, :217).
 *                   delta_angle = Eigen::AngleAxisd(R_kf^T R).angle(): rotation matrix ->
 *                   quaternion, 2 atan2(|vec|, |w|), in [0, pi].  The `ref_keyframe ==
 *                   _last_keyframe` test and the track_last_frame fallback (:218-236, :250) stay
 *                   with the caller.
 * The keyframe's AssignPointsToLines runs once per keyframe (rspl_track_set_keyframe_lines), the
 * frame's inside the added launch.  A point-line assignment that overflows max_pairs, on either
 * side, leaves every line of the frame unmatched and sets `overflow`; the point results and the
 * decision are unaffected.  rspl_track_enqueue / rspl_track_fetch are untouched by all of this. */
typedef struct {
  int max_lines;  /* lines per frame and per keyframe slot, 1 .. 1024 */
  int max_pairs;  /* point-line pairs per frame and per slot (the sum of the std::map sizes) */
} rspl_track_lines_config;
/* Once per handle, before the first line call: allocates the line buffers.  max_lines outside
 * [1, 1024], max_pairs <= 0 or a handle with max_keypoints > 4096 is RSPL_E_ARG, checked before
 * the device is touched. */
int rspl_track_enable_lines(rspl_track* h, const rspl_track_lines_config* cfg);
/* The lines of keyframe slot `slot`: DEVICE d_lines [n_lines][4] doubles, the keyframe's DEVICE
 * SuperPoint records d_features [cap][259] and keypoint count d_n0 (clamped to max_keypoints); HOST
 * line_track_id [n_lines] (Frame::GetLineTrackId) and line_slot [n_lines] (the id of the map line
 * held, or -1), copied before the call returns.  Stream-ordered like rspl_track_set_keyframe: one
 * launch (AssignPointsToLines and the keypoint -> lines incidence, kept in the slot), no host
 * synchronisation.  n_lines == 0 is valid (the device pointers may then be NULL).  A slot keeps its
 * lines until they are set again: call this for every new keyframe of the slot. */
int rspl_track_set_keyframe_lines(rspl_track* h, int slot, int n_lines, const double* d_lines,
                                  const double* d_features, const int32_t* d_n0, const int32_t* line_track_id,
                                  const int32_t* line_slot, void* stream);

typedef struct {
  const double* d_lines;        /* DEVICE [n_lines][4] doubles (rspl_lines_extract_wait_device) */
  int n_lines;                  /* 0: no line work for this frame */
  double kf_Twc[16];            /* _last_keyframe->GetPose(), row-major 4x4 */
  int kf_frame_id, frame_id;
  int max_num_match;            /* keyframe.max_num_match (configs/configs_euroc.yaml:44: 80) */
  double max_angle;             /* 0.52 */
  double max_distance;          /* 0.5 */
  int max_num_passed_frame;     /* 300 */
} rspl_track_frame_ext;

/* add_keyframe: the terms of AddKeyframe's return value (:631-634), non-zero = insert a keyframe */
#define RSPL_TRACK_KF_NOT_ENOUGH_MATCH 1     /* n_inliers < max_num_match */
#define RSPL_TRACK_KF_LARGE_DELTA_ANGLE 2    /* delta_angle > max_angle */
#define RSPL_TRACK_KF_LARGE_DISTANCE 4       /* delta_distance > max_distance */
#define RSPL_TRACK_KF_ENOUGH_PASSED_FRAME 8  /* frame_id - kf_frame_id > max_num_passed_frame */

typedef struct {
  int n_lines;
  int n_line_matches;           /* lines with a keyframe line */
  int n_line_tracks;            /* of those, the lines whose keyframe line carried a track id >= 0 */
  int overflow;                 /* 1: an assignment exceeded max_pairs, every line is unmatched */
  int tracked_well;             /* n_inliers >= min_num_match (:240) */
  int add_keyframe;             /* RSPL_TRACK_KF_* bits */
  double delta_angle, delta_distance;
  int passed_frames;
  /* per line of the frame, caller arrays of max_lines entries (each may be NULL); the first n_lines
   * are written */
  int32_t* line_match_kf;       /* the keyframe line, or -1 */
  int32_t* line_track_id;       /* SetLineTrackId (:498), or -1 */
  int32_t* line_slot;           /* InsertMapline (:499): the keyframe line's map line, or -1 */
} rspl_track_ext_result;

/* rspl_track_enqueue plus the launch above: the same chain with the same results, then the line
 * and decision kernel.  ext[b] goes with frames[b].  Checked before the first launch, besides what
 * rspl_track_enqueue checks: lines enabled, n_lines in [0, max_lines], d_lines != NULL when
 * n_lines > 0.  No host synchronisation and no host work between the launches. */
int rspl_track_enqueue_ext(rspl_track* h, int batch, const rspl_track_frame* frames, const rspl_track_frame_ext* ext,
                           void* stream);
/* rspl_track_fetch for an rspl_track_enqueue_ext: the same single wait; ext_results[b] receives
 * frame b's line results and decision. */
int rspl_track_fetch_ext(rspl_track* h, rspl_track_result* results, rspl_track_ext_result* ext_results);
/* debug (parity tests): the point-line assignments behind frame `frame` of the last (fetched)
 * rspl_track_enqueue_ext, read back as CSR -- line i's keypoints are point_idx[offsets[i] ..
 * offsets[i + 1]) ascending, dist[] the std::map values -- for the frame and for its keyframe slot.
 * offsets: max_lines + 1 entries, point_idx / dist: max_pairs entries; every pointer may be NULL.
 * After an overflow only the offsets are defined. */
typedef struct {
  int n_lines, kf_n_lines;
  int32_t *offsets, *point_idx;
  double* dist;
  int32_t *kf_offsets, *kf_point_idx;
  double* kf_dist;
} rspl_track_debug_lines_out;
int rspl_track_debug_lines(rspl_track* h, int frame, rspl_track_debug_lines_out* out);
/* The DEVICE arrays [max_lines] that receive line_track_id / line_slot of frame `frame` (< max_batch)
 * of every rspl_track_enqueue_ext, for a consumer on the device ordered behind the enqueue's stream. */
int rspl_track_frame_lines(rspl_track* h, int frame, int32_t** d_line_track_id, int32_t** d_line_slot);

/* ------------------------------------------------------------------------ */
/* Keyframe insertion, device side: what turns a tracked stereo frame into a */
/* keyframe between SuperGlue and the map, for a batch of independent frames */
/* as ONE launch behind SuperGlue's stereo pair on the caller's stream:      */
/*   mutual check            src/point_matching.cc:24-31                     */
/*   disparity window, u_right, depth   Frame::AddRightFeatures,             */
/*                           src/frame.cc:157-177 (its return value is       */
/*                           n_stereo_matches).  The depth is bf / (xl - xr) */
/*                           with the SIGNED difference: a right keypoint to */
/*                           the right of its partner passes the |dx| window,*/
/*                           gets a positive u_right and a negative depth,   */
/*                           and fails Frame::BackProjectPoint (:313)        */
/*   new track ids           MapBuilder::InsertKeyframe,                     */
/*                           src/map_builder.cc:660-665; with init = 1       */
/*                           MapBuilder::Init's order (:390-403): the        */
/*                           keypoints with depth > 0 first, then the rest   */
/*                           (the track ids passed in are ignored)           */
/*   new map points          Map::InsertKeyframe, src/map.cc:40-55, with     */
/*                           Camera::BackProjectStereo (src/camera.cc:150-161)*/
/*   the tracker's keyframe table (rspl_track_keyframe_table), optionally    */
/* rspl_kf_enqueue never waits for the device; rspl_kf_fetch waits for the   */
/* one event the enqueue recorded.  One enqueue is in flight per handle.     */
/* ------------------------------------------------------------------------ */
typedef struct {
  int max_batch;             /* frames per enqueue */
  int max_keypoints;         /* keypoints per image */
  int max_tri_points;        /* map points per rspl_kf_triangulate call (0: none) */
  int max_tri_observations;  /* observers, and poses, per rspl_kf_triangulate call */
  int device;
} rspl_kf_config;

typedef struct {
  const double* d_features_left;   /* DEVICE SuperPoint records [cap][259] (x, y = rows 1, 2) */
  const double* d_features_right;
  const int32_t* d_n_left;         /* DEVICE keypoint counts (clamped to max_keypoints) */
  const int32_t* d_n_right;
  const int32_t* d_idx0;           /* DEVICE SuperGlue indices0 [n_left]: left -> right */
  const int32_t* d_idx1;           /* DEVICE SuperGlue indices1 [n_right]: right -> left */
  /* host arrays of n entries, copied before the call returns; a keypoint past n has no id and no point */
  int n;
  const int32_t* track_id;         /* Frame::GetAllTrackIds, or NULL: all -1 */
  const int32_t* point_slot;       /* id of the map point the frame holds at the keypoint or -1; NULL: all -1 */
  const double* points;            /* [n][3] positions of the held points (with point_slot) */
  const uint8_t* state;            /* [n] RSPL_TRACK_* of the held points (with point_slot) */
  double fx, fy, cx, cy, bf;
  double min_x_diff, max_x_diff, max_y_diff;  /* Camera::MinXDiff / MaxXDiff / MaxYDiff */
  double Twc[16];                  /* Frame::GetPose, row-major 4x4 */
  int next_track_id;               /* MapBuilder::_track_id */
  int init;                        /* 1: MapBuilder::Init's id order, no map point without a depth */
  /* the tracker slot to fill (rspl_track_keyframe_table), all three or none: per keypoint the held
   * point's position and state or the new point's (RSPL_TRACK_NOT_GOOD for UnTriangulated,
   * RSPL_TRACK_NO_MAPPOINT where there is none) and the final track id */
  double* d_table_points;
  uint8_t* d_table_state;
  int32_t* d_table_track_id;
  int table_capacity;              /* entries the three arrays hold (the tracker's max_keypoints) */
} rspl_kf_frame;

#define RSPL_KF_NEW_NONE 0
#define RSPL_KF_NEW_GOOD 1            /* a new map point with a stereo position */
#define RSPL_KF_NEW_UNTRIANGULATED 2  /* a new map point without a position */

typedef struct {
  int n_keypoints;       /* left keypoints as the device read them */
  int n_matches;         /* mutual matches */
  int n_stereo_matches;  /* those inside the disparity window: AddRightFeatures' return value */
  int n_new_ids, n_new_points, n_new_good;
  int next_track_id;     /* the next free id */
  /* per left keypoint, caller arrays of max_keypoints entries (each may be NULL); the first n_keypoints
   * are written */
  double* u_right;       /* -1 without a kept match */
  double* depth;
  int32_t* track_id;
  uint8_t* new_point;    /* RSPL_KF_NEW_* */
  double* new_position;  /* [.][3], zeros unless RSPL_KF_NEW_GOOD */
} rspl_kf_result;

typedef struct rspl_kf rspl_kf;
int rspl_kf_create(const rspl_kf_config* cfg, rspl_kf** out);
void rspl_kf_destroy(rspl_kf* h);
int rspl_kf_enqueue(rspl_kf* h, int batch, const rspl_kf_frame* frames, void* stream);
int rspl_kf_fetch(rspl_kf* h, rspl_kf_result* results);

/* Map::TriangulateMappoint (src/map.cc:292-339) for n_points map points in one launch and one
 * synchronisation: poses Twc [n_poses][16] row-major, camera = fx fy cx cy, and a CSR of observers per
 * point in ascending frame id -- offsets [n_points + 1], obs_pose (index into Twc, or -1 for an
 * observer to skip: a frame that is not in the map) and obs_xy [.][2] (the keypoint).  Out: position
 * [n_points][3] and status [n_points] (RSPL_KF_TRI_*; the reference returns false for both failures).
 * The rank test is Eigen::ColPivHouseholderQR's with the threshold 1e-5.  h = NULL runs the host
 * instantiation of the same routine (csrc/kf_triangulate.hpp); the two agree bit for bit.
 * Deviation: Frame::GetKeypointPosition accepts idx == cols (src/frame.cc:215) and would read out of
 * bounds; callers pass a keypoint index >= the frame's keypoint count as an observer to skip. */
#define RSPL_KF_TRI_FEW 0   /* fewer than 2 valid observers */
#define RSPL_KF_TRI_OK 1
#define RSPL_KF_TRI_RANK 2  /* rank < 3 */
int rspl_kf_triangulate(rspl_kf* h, int n_poses, const double* Twc, const double* camera, int n_points,
                        const int32_t* offsets, const int32_t* obs_pose, const double* obs_xy, double* position,
                        uint8_t* status);

/* ------------------------------------------------------------------------ */
/* Keyframe insertion, map side: Map::InsertKeyframe (src/map.cc:24-109) in  */
/* one call, after MapBuilder::InsertKeyframe's line track ids               */
/* (src/map_builder.cc:668-673): the keyframe (:26-28), new map points from  */
/* `tracks` and AddObverser (:40-56), Map::TriangulateMappoint (:292-339)    */
/* for every UnTriangulated point with more than two observers (:57-59) as   */
/* one rspl_kf_triangulate batch on `kfh` (NULL: on the host), new map lines */
/* and observers (:68-92; Frame::TriangulateStereoLine returns false         */
/* unconditionally, src/frame.cc:443), Map::TriangulateMaplineByMappoints    */
/* (:341-419, host; cv::fitLine(DIST_L2) restated, parity unpinned) and, when*/
/* `ba` is given and the map has two keyframes, Map::LocalMapOptimization.   */
/* The first keyframe (:29) gets what MapBuilder::Init gives it              */
/* (src/map_builder.cc:390-437): its new points and lines with their         */
/* observers, no triangulation, no optimisation.                             */
/* Deviation: the reference silently replaces a map entry whose id exists    */
/* and orphans its observers; here a new landmark whose id is already in the */
/* map returns RSPL_E_ARG, before the map changes.                           */
/* ------------------------------------------------------------------------ */
typedef struct {
  /* per keypoint [n_keypoints]: the rspl_kf result, unchanged */
  const int32_t* track_id;
  const int32_t* point_slot;     /* id of the map point the frame holds or -1 */
  const uint8_t* new_point;      /* RSPL_KF_NEW_*; the new point's id is the track id */
  const double* new_position;    /* [.][3] */
  /* per line [n_lines] (each may be NULL: all -1) */
  const int32_t* line_track_id;  /* Frame::GetAllLineTrackId; < 0 takes the next id, ascending */
  const int32_t* line_slot;      /* id of the map line the frame holds or -1 */
  int* next_line_track_id;       /* MapBuilder::_line_track_id, in and out */
} rspl_map_tracks;

typedef struct {
  int n_new_points, n_new_lines;
  int n_tri_candidates, n_tri_ok, n_tri_rank_failures;
  int n_lines_triangulated;
  int optimized;                 /* 1: LocalMapOptimization ran; `optimization` is its report */
  double bookkeeping_us;         /* host wall time: keyframe, landmarks, observers, line triangulation */
  double triangulation_us;       /* the point-triangulation batch */
  rspl_map_report optimization;
} rspl_map_insert_report;

int rspl_map_insert_keyframe(rspl_map* m, const rspl_map_keyframe* kf, const rspl_map_tracks* tracks, rspl_kf* kfh,
                             rspl_ba* ba, rspl_map_insert_report* report);
/* a map line's observers in ascending frame id: the line index and Mapline::GetObverserEndpointStatus */
int rspl_map_get_mapline_observers(const rspl_map* m, int id, int32_t* frames, int32_t* lines,
                                   int32_t* endpoint_status, int cap, int* n_observers);

/* ------------------------------------------------------------------------ */
/* Stereo rectification: Camera::Camera's maps (src/camera.cc:9-63) and      */
/* Camera::UndistortImage (src/camera.cc:87-91), which MapBuilder::AddInput  */
/* runs on both images of every frame (src/map_builder.cc:53-60).  The maps  */
/* are cv::initUndistortRectifyMap (distortion_type 0, radial-tangential)    */
/* or cv::fisheye::initUndistortRectifyMap (distortion_type 1) restated, the */
/* remap is cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on u8 restated: its   */
/* fixed-point arithmetic (coordinates rounded half-to-even to 1/32 pixel,   */
/* integer weights summing to 32768) is followed bit for bit.  OpenCV itself */
/* is not linked, so parity with it is unpinned at the maps: the 3x3 inverse */
/* is Gauss-Jordan with partial pivoting where OpenCV uses LU / SVD, and     */
/* x = _x / _w is a division.  A caller who needs OpenCV's exact maps loads  */
/* them with rspl_rect_set_maps.                                             */
/* ------------------------------------------------------------------------ */
typedef struct {
  double K[9];  /* camera matrix, row-major */
  double D[8];  /* type 0: k1 k2 p1 p2 k3 k4 k5 k6; type 1: k1 k2 k3 k4 and four zeros.  The struct has no
                 * room for thin-prism / tilt terms: a caller holding non-zero ones must refuse them */
  double R[9];  /* rectifying rotation, row-major */
  double P[12]; /* new projection matrix 3x4, row-major; its left 3x3 is used */
} rspl_rect_camera;

typedef struct {
  int height, width;   /* of the raw and of the rectified images; 1..2044 each */
  int distortion_type; /* 0 radial-tangential, 1 equidistant / fisheye */
  rspl_rect_camera cam[2]; /* 0 left, 1 right */
  int max_batch;       /* images per rspl_rect_enqueue_device call, 1..1024 */
  int device;
} rspl_rect_config;

typedef struct rspl_rect rspl_rect;

/* Host only, no device: the float maps [H][W] of one camera.  RSPL_E_ARG for a singular P*R, non-finite
 * parameters, or a fisheye camera with D[4..7] != 0. */
int rspl_rect_build_maps(const rspl_rect_camera* cam, int distortion_type, int height, int width, float* map_x,
                         float* map_y);
/* Host only: the fixed-point table the kernel reads, for n map entries of an H x W source.  ix = floor of
 * the rounded coordinate in 1/32 pixel, frac = fx | fy << 5.  Coordinates whose taps all lie outside are
 * clamped: ix = -2 (left of the image, NaN, -inf) or ix = W, with a zero fraction; iy likewise with H. */
int rspl_rect_debug_fixed(const float* map_x, const float* map_y, size_t n, int height, int width, int16_t* ix,
                          int16_t* iy, uint16_t* frac);
/* sizeof of 0: rspl_rect_camera, 1: rspl_rect_config as the library was built (-1 otherwise) */
int rspl_rect_debug_sizeof(int which);
/* Measurement hook (tools/bench_rect.py): the copy kernel the handles upload with (copy_kernels.hip) on two
 * 16-byte aligned device pointers, as the yardstick of what moving an image's bytes costs. */
int rspl_rect_debug_copy(void* d_dst, const void* d_src, size_t bytes, void* stream);

/* Builds both cameras' maps and the device table once; all device memory is allocated here.  Bad sizes,
 * capacities and models are refused with RSPL_E_ARG before a device is touched. */
int rspl_rect_create(const rspl_rect_config* cfg, rspl_rect** out);
void rspl_rect_destroy(rspl_rect* h);
/* the float maps [H][W] of camera `cam` (0 / 1) as the handle holds them; set replaces them (maps
 * exported from OpenCV, for instance) and waits for the handle's earlier work */
int rspl_rect_get_maps(rspl_rect* h, int cam, float* map_x, float* map_y);
int rspl_rect_set_maps(rspl_rect* h, int cam, const float* map_x, const float* map_y);

/* Device in, device out, stream-ordered, never waits for the device: raw image b at d_raw + b*raw_pitch
 * (row stride raw_stride bytes) through the maps of camera cam_index[b] (host array) to d_out + b*out_pitch
 * (row stride out_stride) -- the layout rspl_sp_infer_device takes.  One launch for the whole batch.
 * Bytes between width and out_stride are not written.  Overlapping input and output ranges, strides below
 * the width, pitches below an image and batch > max_batch are RSPL_E_ARG.  stream may be NULL. */
int rspl_rect_enqueue_device(rspl_rect* h, int batch, const uint8_t* d_raw, size_t raw_stride, size_t raw_pitch,
                             const int* cam_index, uint8_t* d_out, size_t out_stride, size_t out_pitch,
                             void* stream);
/* Camera::UndistortImage: host images in (one row stride for both), rectified host images out. */
int rspl_rect_pair(rspl_rect* h, const uint8_t* left, const uint8_t* right, size_t stride, uint8_t* left_rect,
                   uint8_t* right_rect, size_t out_stride);

/* ------------------------------------------------------------------------ */
/* RCF edge network: RCF::infer (src/rcf.cpp:95-135), which                  */
/* MapBuilder::AddInput runs on both rectified images of every frame         */
/* (src/map_builder.cc:86-121) and whose edge image, not the camera image,   */
/* the line detector then reads (src/map_builder.cc:286, :327).  The network */
/* is the VGG16-based RCF of yun-liu/RCF-PyTorch, the weights an RSPLWT01     */
/* blob with that model's state_dict names (conv1_1 .. conv5_3, their _down   */
/* 1x1 convs, score_dsn1..5, score_fuse).  The input is the gray u8 image as  */
/* raw floats 0..255 (src/rcf.cpp:161-192; the three identical input          */
/* channels are folded into conv1_1's weights).  The reference's engine file  */
/* and ONNX are not available, so parity with its binding "230" is unpinned:  */
/* `output` selects which of the network's six maps becomes the edge image.   */
/* ------------------------------------------------------------------------ */
typedef struct {
  int max_height, max_width; /* 16..2048 each: every call's H, W lie in 16..max */
  int max_batch;             /* images per rspl_rcf_infer_device call, 1..64 */
  int precision;             /* RSPL_PREC_FP32 (the reference: kFP16 is commented out, src/rcf.cpp:51) or
                              * RSPL_PREC_FP16 */
  int output;                /* 0..4: sigmoid(so_1..5), 5: sigmoid(fuse) (RCF's result; the default to use) */
  int device;
} rspl_rcf_config;

typedef struct rspl_rcf rspl_rcf;

/* sizeof of 0: rspl_rcf_config as the library was built (-1 otherwise) */
int rspl_rcf_debug_sizeof(int which);
/* RCF::build (src/rcf.cpp:25-93) without an engine to deserialise: reads the blob, lays the weights out for
 * the kernels and allocates all device memory.  A bad config is RSPL_E_ARG before the blob or a device is
 * touched; a missing or mis-shaped tensor is RSPL_E_WEIGHTS and rspl_last_error() names it. */
int rspl_rcf_create(const rspl_rcf_config* cfg, const char* weights_path, rspl_rcf** out);
void rspl_rcf_destroy(rspl_rcf* h);
/* RCF::infer (src/rcf.cpp:95-135) with process_output's conversion (src/rcf.cpp:147-152): gray u8 host image
 * [H][stride] in, edge image [H][W] u8 out, (uint8)(unsigned)(255.0f - p * 255.0f). */
int rspl_rcf_infer(rspl_rcf* h, const uint8_t* image, int H, int W, size_t stride, uint8_t* edges);
/* The same on `batch` device images, image b at d_images + b*pitch with row stride `stride` bytes (the layout
 * rspl_rect_enqueue_device writes), edge image b to d_edges + b*out_pitch with row stride out_stride.
 * Stream-ordered, never waits for the device; bytes outside the W pixels of a row are not written.  H or W
 * outside 16..max, strides below W, pitches below an image and batch > max_batch are RSPL_E_ARG before any
 * device call.  stream may be NULL (the handle's own). */
int rspl_rcf_infer_device(rspl_rcf* h, const uint8_t* d_images, int batch, int H, int W, size_t stride, size_t pitch,
                          uint8_t* d_edges, size_t out_stride, size_t out_pitch, void* stream);
/* Parity hook: the pre-sigmoid map `which` (0..4: so_1..5 upsampled and cropped, 5: fuse) of image b of the
 * last call, [H][W] floats to the host.  Waits for that call. */
int rspl_rcf_debug_logits(rspl_rcf* h, int b, int which, float* out);
/* Device time per stage, from events on the call's stream (never a host wait): profile(1) starts collecting,
 * stage_times adds up the RSPL_RCF_STAGES segments of the calls since -- stages 1..5 (each its pool, its 3x3
 * convs and their side branches) and the tail -- in milliseconds, and the number of calls. */
#define RSPL_RCF_STAGES 6
int rspl_rcf_profile(rspl_rcf* h, int enable);
int rspl_rcf_stage_times(rspl_rcf* h, float* ms, int* calls);
/* Test hook: the 3x3 convolutions' workgroup tile, 8 or 16 rows (of 16 columns and 64 channels), for the calls
 * that follow; 0 (the default) chooses per layer from the launch's size, which small test images never carry
 * past the threshold.  The results do not depend on it, bit for bit. */
int rspl_rcf_debug_tile_rows(rspl_rcf* h, int rows);

/* ------------------------------------------------------------------------ */
/* F-matrix RANSAC: cv::findFundamentalMat(points0, points1, cv::FM_RANSAC,  */
/* 3, 0.99, inliers) as PointMatching::MatchingPoints calls it               */
/* (src/point_matching.cc:34-45), for a batch of independent frames.  A      */
/* restatement of OpenCV 4.2's published algorithm (tests/fm_ref.py states   */
/* it; OpenCV itself is not available, so parity with it is unpinned):       */
/* cv::RNG seeded (uint64)-1, subsets of 7 distinct indices, checkSubset,    */
/* the 7-point solver (up to three models), max(d1^2 s1, d2^2 s2) rounded to */
/* float against (float)(threshold^2), the sequential acceptance with        */
/* RANSACUpdateNumIters, no refit.  All iterations are solved side by side   */
/* on the device and the acceptance replayed afterwards.                     */
/*   n < 7   no model, nothing rejected: n_inliers = -1, inlier[] all 1      */
/*   n == 7  the 7-point solver directly, its first model, inlier[] all 1    */
/*   n >= 8  RANSAC; no model ever accepted: n_inliers = -1, inlier[] all 1  */
/* ------------------------------------------------------------------------ */
typedef struct {
  int max_batch;
  int max_matches; /* matches per frame; on the device-resident path also the keypoints per image considered */
  int max_iters;   /* 1000 (RANSACPointSetRegistrator's maxIters); at most 1000 */
  int device;
} rspl_fm_config;

typedef struct {
  int n;
  const double* points0; /* [n][2] pixels */
  const double* points1;
  double threshold;      /* 3.0 */
  double confidence;     /* 0.99 */
} rspl_fm_problem;

typedef struct {
  uint8_t* inlier; /* [n], may be NULL */
  int n_inliers;   /* -1: no model, nothing rejected */
  int hypotheses;  /* iterations evaluated */
  double F[9];     /* row-major, x1^T F x0 = 0; zeros without a model */
} rspl_fm_result;

typedef struct rspl_fm rspl_fm;

int rspl_fm_create(const rspl_fm_config* cfg, rspl_fm** out);
void rspl_fm_destroy(rspl_fm* h);
/* Host matches in, results out: the host draws the subsets, the device solves, counts and accepts (three
 * launches behind the upload), one wait. */
int rspl_fm_solve(rspl_fm* h, const rspl_fm_problem* problems, int batch, rspl_fm_result* results);

/* Device-resident: SuperPoint records [cap][259] (x, y = rows 1, 2) and device counts of both images, SuperGlue's
 * device indices in, filtered indices out: copies of d_idx0 / d_idx1 with both ends of every rejected match set
 * to -1 and everything else untouched (without a model: plain copies).  d_idx0_out / d_idx1_out drop into
 * rspl_track_frame.d_idx0 / d_idx1, d_idx0_out into rspl_lines_stereo_device's d_match_idx.  The mutual matches
 * are compacted in ascending index of image 0 (the DMatch order the subsets refer to).  Stream-ordered, no host
 * synchronisation; one enqueue in flight per handle; stream may be NULL (the handle's own).  The subsets come
 * from a table of raw RNG draws sized at create: it holds max_iters subsets and up to 256 redraws after a failed
 * checkSubset for every match count (a handle that cannot hold 32 is refused); a frame that needs more ends its
 * iterations there, where OpenCV would go on for up to 10000 attempts per iteration.  Keypoints past
 * max_matches in either image are not considered and their index entries are copied unchanged. */
typedef struct {
  const double* d_features0;
  const int32_t* d_n0;
  const double* d_features1;
  const int32_t* d_n1;
  const int32_t* d_idx0;
  const int32_t* d_idx1;
  int32_t* d_idx0_out;
  int32_t* d_idx1_out;
  double threshold, confidence;
} rspl_fm_frame;
int rspl_fm_enqueue(rspl_fm* h, int batch, const rspl_fm_frame* frames, void* stream);
/* Waits for the enqueue; inlier[] per compacted match (may be NULL; the caller sizes it for max_matches). */
int rspl_fm_fetch(rspl_fm* h, rspl_fm_result* results);

/* debug (parity tests) */
/* host: the subsets `iters` iterations draw for `count` float-rounded pairs, idx [iters][7]; *n_found of them
 * exist (getSubset gave up after 10000 attempts otherwise). */
int rspl_fm_debug_subsets(int count, int iters, const double* points0, const double* points1, int32_t* idx,
                          int* n_found);
/* host mirror of the kernel's 7-point solver (csrc/fm_solve.hpp): p0, p1 [7][2] -> F [3][9], *n_models */
int rspl_fm_debug_seven_point(const double* p0, const double* p1, double* F, int* n_models);
/* frame `frame` of the last solve / fetched enqueue: the first min(max, iterations solved) iterations' model
 * counts, inlier counts [max][3] and models [max][3][9]; returns how many, or a negative error */
int rspl_fm_debug_hypotheses(rspl_fm* h, int frame, int max, int32_t* n_models, int32_t* counts, double* F);

/* ------------------------------------------------------------------------ */
/* Local map tracking: Map::SearchByProjection (src/map.cc:952-1005) and     */
/* MapBuilder::TrackLocalMap (src/map_builder.cc:753-785) for a batch of     */
/* independent frames.  The reference never calls this path (DESIGN section  */
/* 9); it is restated from its text, and parity is with tests/lmap_ref.py.   */
/*   bank     one fp64 descriptor (256 values) per map point id: the one     */
/*            Map::InsertKeyframe stores at creation (map.cc:44-47)          */
/*   local    the ordered local map: ids (resolved to bank rows), positions  */
/*   search   per local point the frame does not hold: pc = Rwc^T (pw - twc),*/
/*            Camera::StereoProject, the strict image bounds, the candidates */
/*            of Frame::FindNeighborKeypoints(r, filter = true), best and    */
/*            second-best 2 (1 - d_point . d_kp), the 0.35 / 0.6 test.  An   */
/*            exact tie in the distance goes to the keypoint the reference's */
/*            64 x 48 grid walk visits first: argmin over (dist, gx, gy, idx)*/
/*   merge    the ordered good list; per keypoint the frame's own point or   */
/*            the LAST good projection that claims it (TrackLocalMap's loop) */
/*   chain    the merged table written into an rspl_track keyframe slot and  */
/*            rspl_track_enqueue behind it on the same stream                */
/* The descriptor distance has one summation order everywhere (lane l of 64  */
/* owns entries 4l..4l+3, ((a0 b0 + a1 b1) + a2 b2) + a3 b3, the 64 partials */
/* by the xor butterfly 32..1), so the device and rspl_lmap_debug_search_host*/
/* agree bit for bit.                                                        */
/* ------------------------------------------------------------------------ */
typedef struct {
  int max_bank_points;   /* descriptors the bank holds */
  int max_local_points;  /* local map points per rspl_lmap_set_local */
  int max_keypoints;     /* keypoints per frame, at most 8192 */
  int max_batch;
  int device;            /* < 0: a host-only handle -- bank and local-table bookkeeping with the descriptors kept
                          * on the host (rspl_lmap_store_host, rspl_lmap_set_local); every device call is refused */
  double radius;         /* 15 (r = 15 thr, thr = 1) */
  double max_distance;   /* 0.35 */
  double max_ratio;      /* 0.6 */
} rspl_lmap_config;

/* per local point, rspl_lmap_debug_points / rspl_lmap_debug_search_host */
#define RSPL_LMAP_NOT_SELECTED 0  /* the frame already holds this point */
#define RSPL_LMAP_BEHIND 1        /* pc.z <= 0 */
#define RSPL_LMAP_OFF_IMAGE 2     /* not 0 < u < W and 0 < v < H */
#define RSPL_LMAP_NO_CANDIDATE 3
#define RSPL_LMAP_FAILED 4        /* best >= max_distance or best >= max_ratio * second */
#define RSPL_LMAP_GOOD 5

typedef struct {
  const double* d_features;    /* DEVICE SuperPoint records [cap][259] (x, y = rows 1, 2; descriptor = rows 3..258) */
  const int32_t* d_n1;         /* DEVICE keypoint count (clamped to max_keypoints) */
  const double* d_u_right;     /* DEVICE [n1] right-image u, -1 without a stereo partner: the reference's dxr test.
                                * NULL: the dxr term is skipped (a tracking frame has no right image) */
  const int32_t* d_point_id;   /* DEVICE [n1] id of the non-bad map point keypoint i holds, or -1 */
  const double* d_point_xyz;   /* DEVICE [n1][3] its position (read where d_point_id >= 0) */
  const uint8_t* d_point_good; /* DEVICE [n1] 1: that point is Good (an edge of the pose optimisation), 0: held but
                                * not Good (RSPL_TRACK_NOT_GOOD in the chained table).  NULL: every held point is Good */
  double Twc[16];              /* the pose to project with, row-major 4x4 */
  double fx, fy, cx, cy, bf;
  int width, height;
} rspl_lmap_frame;

typedef struct {
  int n_keypoints;         /* as the device read it */
  int n_selected;          /* local points the frame does not hold */
  int n_projected;         /* ... in front of the camera and inside the image */
  int n_with_candidates;
  int n_good;
  /* caller arrays (each may be NULL) */
  int32_t* good_kp;        /* [max_local_points] the good projections in local-map order: keypoint ... */
  int32_t* good_point;     /* ... and LOCAL INDEX of the point; the first n_good are written */
  int32_t* assoc_id;       /* [max_keypoints] the merged table: map point id per keypoint or -1; the first
                            * n_keypoints are written */
} rspl_lmap_result;

typedef struct rspl_lmap rspl_lmap;

int rspl_lmap_create(const rspl_lmap_config* cfg, rspl_lmap** out);
void rspl_lmap_destroy(rspl_lmap* h);
/* Mappoint::SetDescriptor at creation: rows 3..258 of record keypoints[k] of the DEVICE records d_features become
 * the descriptor of map point ids[k] (ids, keypoints: host arrays, copied before the call returns; the copy is
 * stream-ordered on `stream`, NULL: the handle's).  An id the bank already has is overwritten; an id that does
 * not fit fails with RSPL_E_CAPACITY and stores nothing of the call. */
int rspl_lmap_store(rspl_lmap* h, int n, const int32_t* ids, const int32_t* keypoints, const double* d_features,
                    void* stream);
/* the same from host descriptors [n][256]; returns after the copy */
int rspl_lmap_store_host(rspl_lmap* h, int n, const int32_t* ids, const double* descriptors);
int rspl_lmap_bank_size(const rspl_lmap* h, int* n);
/* The local map, in order: ids[n] and positions[n][3] (host arrays, copied before the call returns; uploaded on
 * `stream`).  Ids are resolved to bank rows here -- the search reads the bank through that table, no descriptor
 * is copied.  An id without a descriptor fails with RSPL_E_ARG and rspl_last_error names it; the local map is
 * then unchanged. */
int rspl_lmap_set_local(rspl_lmap* h, int n, const int32_t* ids, const double* positions, void* stream);
/* Search + merge for frames[0 .. batch) against the local map on `stream` (NULL: the handle's).  No host
 * synchronisation; one enqueue in flight per handle: fetch before the next.  The enqueue's stream waits (on the
 * device) for the handle's last rspl_lmap_store and rspl_lmap_set_local, whatever streams they went to; what
 * produces the frame's own device arrays must be ordered before it by the caller. */
int rspl_lmap_enqueue(rspl_lmap* h, int batch, const rspl_lmap_frame* frames, void* stream);
/* Wait for the last enqueue; results[b] receives frame b. */
int rspl_lmap_fetch(rspl_lmap* h, rspl_lmap_result* results);
/* frame `frame` of the last fetched enqueue, per local point (arrays of the local map's length, each may be NULL):
 * status RSPL_LMAP_*, best_idx (-1: none), best and second (4.0 where nothing was below it) */
int rspl_lmap_debug_points(rspl_lmap* h, int frame, int32_t* status, int32_t* best_idx, double* best, double* second);
/* The chain: search, merge into t's keyframe slots tf[b].slot (through rspl_track_keyframe_table with n0 =
 * max_keypoints: t's max_keypoints must not be smaller) and rspl_track_enqueue(t, batch, tf, stream) with the
 * handle's identity indices in place of tf[b].d_idx0 / d_idx1 (both ignored).  Per keypoint j of the slot: the
 * frame's own point, else the winning projection (state RSPL_TRACK_GOOD, track id = the point's id), else
 * RSPL_TRACK_NO_MAPPOINT.  Results: rspl_track_fetch and rspl_lmap_fetch.  TrackLocalMap's gates (fewer than 3
 * good projections; n_inliers > min_num_match && n_inliers > num_inlier_thr) are the caller's, from the fetched
 * counts: the chain always runs.  As in the tracking step a point whose id is 0 is dropped by `> 0`.  The tracker
 * is handed the keypoint count the search used (*d_n1 clamped to this handle's max_keypoints), not tf[b].d_n1, so
 * both fetches report the same n_keypoints.  `t` must live on the handle's device.  When the call fails at frame b's
 * slot, the slots of frames before b keep the keypoint count max_keypoints that the call gave them. */
int rspl_lmap_track_enqueue(rspl_lmap* h, rspl_track* t, int batch, const rspl_lmap_frame* frames,
                            const rspl_track_frame* tf, void* stream);

/* debug (parity tests): the host instantiation of the search text (csrc/lmap_match.hpp) on host arrays */
typedef struct {
  int n_keypoints;
  const double* features;      /* [n_keypoints][259] */
  const double* u_right;       /* [n_keypoints] or NULL */
  const int32_t* point_id;     /* [n_keypoints] */
  int n_local;
  const int32_t* local_ids;    /* [n_local] */
  const double* local_pos;     /* [n_local][3] */
  const double* local_desc;    /* [n_local][256] */
  double Twc[16];
  double fx, fy, cx, cy, bf;
  int width, height;
  double radius, max_distance, max_ratio;
} rspl_lmap_host_problem;
int rspl_lmap_debug_search_host(const rspl_lmap_host_problem* p, int32_t* status, int32_t* best_idx, double* best,
                                double* second);

/* Local map selection on the native map (MapBuilder::UpdateReferenceFrame, UpdateLocalKeyframes,
 * UpdateLocalMappoints; src/map_builder.cc:684-734). */
/* point_ids[n]: the current frame's slots (map point id or -1; bad and unknown ids are skipped, untriangulated
 * ones count).  Every observer of those points other than current_frame_id that the map knows gets one vote per
 * point; the reference keyframe becomes the observer with the most votes (strictly; ties: the lowest frame id).
 * *ref = that frame (current_ref when nobody was counted), *changed = it differs from current_ref. */
int rspl_map_reference_keyframe(const rspl_map* m, int current_frame_id, int n, const int32_t* point_ids,
                                int current_ref, int* ref, int* changed);
/* The Good map points of ref_frame_id's neighbours, GetOrderedConnections(-1) order (ascending weight, frame id;
 * the reference keyframe itself is not walked), each frame's slots in keypoint order, first occurrence only.
 * *n = how many there are; ids / positions (each may be NULL) receive them when cap >= *n, otherwise nothing is
 * written and the call fails with RSPL_E_CAPACITY. */
int rspl_map_local_mappoints(const rspl_map* m, int ref_frame_id, int32_t* ids, double* positions, int cap, int* n);


/* ------------------------------------------------------------------------ */
/* Relocalisation: the search of the local table by descriptor alone.  The   */
/* reference has no such stage; parity is with           */
/* tests/reloc_ref.py.  D[i][p] = 2 (1 - q_i . d_p) for keypoint i of the    */
/* frame and entry p of the table rspl_lmap_set_local set:                   */
/*   per keypoint  best, arg (a tie keeps the lowest p), second (the second  */
/*                 smallest value; 4.0 where nothing is below it)            */
/*   per point     kbest, the lowest i that attains min_i D[i][p]            */
/*   pass          best < max_distance and best < max_ratio * second         */
/*   match         pass and (mutual == 0 or kbest[arg] == i)                 */
/* The device evaluates D on fp64 MFMA; its distances agree with the host's  */
/* fixed summation order to rounding (1e-13), its decisions exactly wherever */
/* no two candidates are closer than that.                                   */
/* ------------------------------------------------------------------------ */
typedef struct {
  double max_distance; /* 0.35 */
  double max_ratio;    /* 0.6 */
  int mutual;          /* != 0: a match must also be its point's nearest keypoint */
} rspl_lmap_global_params;

typedef struct {
  int n_keypoints; /* as the device read it (clamped to max_keypoints) */
  int n_local;
  int n_pass;
  int n_matched;
  /* caller arrays (each may be NULL) */
  int32_t* arg;         /* [max_keypoints] local index of the nearest point or -1; the first n_keypoints ... */
  double* best;         /* ... of these four are written */
  double* second;
  int32_t* match;       /* local index of the match or -1 */
  int32_t* kbest;       /* [max_local_points] nearest keypoint per local point or -1; the first n_local */
  /* the matches in ascending keypoint order, the first n_matched of each [max_keypoints] array */
  int32_t* match_kp;    /* keypoint index */
  int32_t* match_local; /* local index */
  int32_t* match_id;    /* map point id */
  double* match_pos;    /* [..][3] its position */
  double* match_xy;     /* [..][2] the keypoint (rows 1, 2 of its record) */
} rspl_lmap_global_result;

/* frames[b].d_features and d_n1 are read; every other field of rspl_lmap_frame is ignored.  Same stream rules as
 * rspl_lmap_enqueue: no host synchronisation, a device-side wait for the handle's last store / set_local, and one
 * enqueue in flight per handle whatever its kind (RSPL_E_ARG otherwise; rspl_lmap_set_local is refused in
 * between).  The first call allocates the search's partial arrays.  A host-only handle is refused. */
int rspl_lmap_global_enqueue(rspl_lmap* h, int batch, const rspl_lmap_frame* frames,
                             const rspl_lmap_global_params* params, void* stream);
/* Wait for the last global enqueue; results[b] receives frame b. */
int rspl_lmap_global_fetch(rspl_lmap* h, rspl_lmap_global_result* results);

/* debug (parity tests): the same contract on host arrays, distances in the fixed summation order of
 * csrc/lmap_match.hpp -- equal to tests/reloc_ref.py bit for bit; no device is touched */
typedef struct {
  int n_keypoints;
  const double* features;   /* [n_keypoints][259] */
  int n_local;
  const int32_t* local_ids; /* [n_local] */
  const double* local_pos;  /* [n_local][3] */
  const double* local_desc; /* [n_local][256] */
} rspl_lmap_global_host_problem;
int rspl_lmap_debug_global_host(const rspl_lmap_global_host_problem* p, const rspl_lmap_global_params* params,
                                rspl_lmap_global_result* result);
/* the tile geometry of the device search for a handle of these capacities: bank rows per workgroup, keypoints per
 * workgroup, descriptor entries per LDS slab (each may be NULL) */
int rspl_lmap_debug_global_plan(int max_keypoints, int max_local_points, int* chunk_rows, int* qtile_rows,
                                int* k_slab);

/* Every Good map point in ascending id order (the candidate table of a relocalisation over the whole map); the
 * cap / *n protocol of rspl_map_local_mappoints. */
int rspl_map_good_mappoints(const rspl_map* m, int32_t* ids, double* positions, int cap, int* n);


/* ------------------------------------------------------------------------ */
/* Loop closure: pose-graph optimisation over all keyframes on a tile-sparse */
/* fp64 Cholesky.  The reference has no such stage;      */
/* parity is with tests/pgo_ref.py.                                          */
/*   poses     T_wc: pose_q x y z w (as rspl_ba_problem), pose_p             */
/*   edge      measured Z = T_wi^-1 T_wj, weights (w_t, w_r);                */
/*             d = R_i^T (p_j - p_i), e_t = d - t_Z,                         */
/*             e_R = Log(R_Z^T R_i^T R_j) through the quaternion, w >= 0     */
/*   cost      F = sum w_t |e_t|^2 + w_r |e_R|^2                             */
/*   update    p <- p + dp, R <- R Exp(dphi) on the free poses               */
/*   LM        H = sum J^T W J, b = -sum J^T W e, lambda_0 = 1e-5 max diag H;*/
/*             a trial solves (H + lambda I) d = b by Cholesky;              */
/*             rho = (F - F_new) / (d^T (lambda d + b)); rho > 0 and F_new   */
/*             finite accepts: lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2;*/
/*             otherwise (a non-positive pivot included) lambda *= nu,       */
/*             nu *= 2; ten rejections in a row end the call; a trial whose  */
/*             predicted decrease d^T (lambda d + b) is at most 1e-12 F ends */
/*             it converged, the step not applied: F carries rounding noise  */
/*             of about 2 u |d| / |e| relative (1e-14 at metres of motion    */
/*             and centimetres of residual), below which rho's sign, and     */
/*             with it status and iteration count, would be noise            */
/* Refused with RSPL_E_ARG: no fixed pose; an edge with i == j or an index   */
/* out of range; a connected component with a free pose that has an edge but */
/* no fixed pose.  A free pose without an edge comes back unchanged (where no */
/* free pose has an edge: zero iterations, converged), an edge between fixed */
/* poses only adds to the cost, duplicate edges sum.                         */
/* ------------------------------------------------------------------------ */
#define RSPL_PGO_CONVERGED 0      /* an accepted step with max |d| < step_tol, a trial the cost cannot resolve, or
                                   * nothing to optimise */
#define RSPL_PGO_MAX_ITERATIONS 1 /* max_iterations accepted steps */
#define RSPL_PGO_STALLED 2        /* ten rejections in a row */

typedef struct rspl_pgo rspl_pgo;
typedef struct {
  int max_poses; /* 1..4096 */
  int max_edges;
  int max_tiles; /* 96 x 96 fp64 tiles of the factor the handle can hold (73728 bytes each) */
  int device;
} rspl_pgo_config;

typedef struct {
  int n_poses;
  const double* pose_q;      /* [n_poses][4] */
  const double* pose_p;      /* [n_poses][3] */
  const uint8_t* pose_fixed; /* [n_poses] */
  int n_edges;
  const int32_t* edge_i;     /* [n_edges] */
  const int32_t* edge_j;
  const double* edge_q;      /* [n_edges][4] */
  const double* edge_p;      /* [n_edges][3] */
  const double* edge_w;      /* [n_edges][2] (w_t, w_r) */
} rspl_pgo_problem;

typedef struct {
  int max_iterations; /* 0: 30 */
  double step_tol;    /* 0: 1e-10 */
} rspl_pgo_params;

typedef struct {
  double* pose_q; /* caller arrays [n_poses][4], [n_poses][3] */
  double* pose_p;
  int status;     /* RSPL_PGO_* */
  int iterations; /* accepted steps */
  int trials;
  int n_free;
  int n_tiles;        /* lower-triangle tiles an edge or a free pose touches */
  int n_filled_tiles; /* the same after the tile-level symbolic factorisation: what is stored and computed */
  double cost_initial, cost_final, lambda;
} rspl_pgo_result;

/* A handle allocates everything at create.  Free poses keep the caller's order; tile t holds free poses
 * 16 t .. 16 t + 15.  A problem beyond max_poses / max_edges, or whose plan needs more than max_tiles tiles, fails
 * with RSPL_E_CAPACITY before any launch; a factorisation that never succeeds fails with RSPL_E_SOLVER.  LM control
 * runs on the host with one synchronisation per trial.  The result repeats bit for bit from call to call. */
int rspl_pgo_create(const rspl_pgo_config* cfg, rspl_pgo** out);
void rspl_pgo_destroy(rspl_pgo* h);
int rspl_pgo_solve(rspl_pgo* h, const rspl_pgo_problem* problem, const rspl_pgo_params* params,
                   rspl_pgo_result* result);

/* debug (parity tests): the host twin -- the text of csrc/pgo_solve.hpp, the same tile plan and LM rule on plain
 * C++ tiles; no device is touched */
int rspl_pgo_debug_host(const rspl_pgo_problem* problem, const rspl_pgo_params* params, rspl_pgo_result* result);
/* debug: the tile plan of a problem, host only.  Each output may be NULL; tile_map [tiles_per_side][tiles_per_side]
 * (map_cap >= tiles_per_side^2 entries, RSPL_E_CAPACITY otherwise) receives the storage index of each filled
 * lower-triangle tile, -1 elsewhere. */
int rspl_pgo_debug_plan(const rspl_pgo_problem* problem, int* n_free, int* tiles_per_side, int* n_tiles,
                        int* n_filled_tiles, int32_t* tile_map, int map_cap);
/* debug: one linearisation at the problem's poses and one solve of (H + lambda I) delta = b on the device.
 * e [n_edges][6], b [6 n_free], delta [6 n_free], H_dense [6 n_free][6 n_free] (H without lambda; NULL is required
 * when 6 n_free > 1536); each may be NULL.  RSPL_E_SOLVER for a non-positive pivot. */
int rspl_pgo_debug_system(rspl_pgo* h, const rspl_pgo_problem* problem, double lambda, double* e, double* b,
                          double* H_dense, double* delta);

/* The pose graph of the native map.  Nodes: every keyframe in ascending id with its pose.  Edges: each keyframe's
 * parent edge plus every connection of weight >= min_weight, each unordered pair once as (lower id, higher id) in
 * ascending (i, j) order; edge_i / edge_j index the node list; Z = T_wi^-1 T_wj from the current poses;
 * edge_weight is the connection weight, 0 for a parent-only pair.  *n_nodes and *n_edges are always set; the arrays
 * (each may be NULL) are written when node_cap >= *n_nodes and edge_cap >= *n_edges, otherwise nothing is written
 * and the call fails with RSPL_E_CAPACITY. */
int rspl_map_pose_graph(const rspl_map* m, int min_weight, int32_t* frame_ids, double* pose_q, double* pose_p,
                        int node_cap, int* n_nodes, int32_t* edge_i, int32_t* edge_j, double* edge_q, double* edge_p,
                        int32_t* edge_weight, int edge_cap, int* n_edges);
/* Set the poses of the listed keyframes (an unknown or repeated frame id is RSPL_E_ARG before the map changes).
 * Every non-bad map point with a position and every map line moves rigidly with its anchor, X' = T' T^-1 X (a line's
 * Pluecker coordinates and endpoints by the same motion); the anchor is its lowest-id observer among the listed
 * frames, and a landmark no listed frame observes stays where it is. */
int rspl_map_apply_pose_graph(rspl_map* m, int n, const int32_t* frame_ids, const double* pose_q,
                              const double* pose_p);
/* Loop candidates for keyframe frame_id: every observer of point_ids[n] (map point id or -1; bad and unknown ids
 * are skipped) gets one vote per point; frame_id itself, its connections and the frames within min_gap frame ids
 * of it are left out.  Descending votes, ties to the lower id; the cap / *n protocol of rspl_map_local_mappoints. */
int rspl_map_loop_candidates(const rspl_map* m, int frame_id, int n, const int32_t* point_ids, int min_gap,
                             int32_t* ids, int32_t* votes, int cap, int* n_out);

#ifdef __cplusplus
}
#endif
#endif /* RSPL_H_ */
