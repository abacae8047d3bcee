"""Host-side mirror of the reference's C++ classes for the hot path, over the C ABI.

  SuperPoint     include/super_point.h:20-66      (build / infer)
  SuperGlue      include/super_glue.h:20-71       (build / infer)
  PointMatching  include/point_matching.h:7-18    (MatchingPoints / NormalizeKeypoints)
  LocalmapOptimization  include/g2o_optimization/g2o_optimization.h:15-19
  FrameOptimization     include/g2o_optimization/g2o_optimization.h:20-22
  SolvePnPWithCV        include/g2o_optimization/g2o_optimization.h:24

Same names and argument meaning as the reference; C++ out-parameters become
return values ((ok, features) for SuperPoint::infer, etc.).  Everything runs
in librspl.so on the MI355X -- no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from . import capi


@dataclass
class SuperPointConfig:               # include/read_configs.h:9-18 (+ device arena sizing)
    max_keypoints: int = 400
    keypoint_threshold: float = 0.004
    remove_borders: int = 4
    weights: str = ""                 # RSPLWT01 blob (replaces onnx_file / engine_file)
    max_height: int = 480
    max_width: int = 752
    max_batch: int = 2
    precision: int = capi.RSPL_PREC_FP32
    device: int = 0


class SuperPoint:
    """Mirror of class SuperPoint (include/super_point.h:20-66)."""

    def __init__(self, super_point_config: SuperPointConfig):
        self.config = super_point_config
        self._h = C.c_void_p()
        self._lib = capi.load()

    def build(self) -> bool:
        c = self.config
        cfg = capi.SpConfig(c.max_keypoints, c.keypoint_threshold, c.remove_borders, c.max_height, c.max_width,
                            c.max_batch, c.precision, c.device)
        rc = self._lib.rspl_sp_create(C.byref(cfg), c.weights.encode(), C.byref(self._h))
        self.error = None if rc == 0 else self._lib.rspl_last_error().decode()
        return rc == 0

    def _cap(self):
        k = self.config.max_keypoints  # -1 keeps all (up to 16384); 0 yields none (one slot, never written)
        return 16384 if k == -1 else max(k, 1)

    def infer(self, image: np.ndarray) -> Tuple[bool, np.ndarray]:
        """SuperPoint::infer (src/super_point.cpp:104-135): u8 [H, W] -> (ok, features [259, N])."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        H, W = img.shape
        cap = self._cap()
        out = np.empty((cap, 259), np.float64)
        n = C.c_int(0)
        rc = self._lib.rspl_sp_infer(self._h, img.ctypes.data, H, W, W, out.ctypes.data, cap, C.byref(n))
        if rc != 0:
            self.error = self._lib.rspl_last_error().decode()
            return False, np.zeros((259, 0))
        return True, np.ascontiguousarray(out[: n.value].T)

    def infer_device(self, d_images: int, batch: int, height: int, width: int, stride: int, pitch: int,
                     d_features: int, capacity: int, d_counts: int, stream: Optional[int] = None) -> None:
        """Batched device-resident form (pointers are device addresses, e.g. torch tensor data_ptr())."""
        capi.check(self._lib.rspl_sp_infer_device(self._h, d_images, batch, height, width, stride, pitch,
                                                  d_features, capacity, d_counts, stream), "rspl_sp_infer_device")

    STAGES = ("conv1a+1b+pool", "conv2a..conv4b", "convPa|convDa", "heads 1x1", "nms", "topk", "sample")

    def profile(self, enable: bool = True):
        capi.check(self._lib.rspl_sp_profile(self._h, int(enable)), "rspl_sp_profile")

    def stage_times(self):
        """(per-stage summed ms, calls) since profile(True)"""
        return capi.stage_times(None, self._lib.rspl_sp_stage_times, self._h, len(self.STAGES))

    def debug_nms(self, scores: np.ndarray) -> np.ndarray:
        """The device simple_nms (superpoint.py:6-33) of a host score map."""
        sc = np.ascontiguousarray(scores, np.float32)
        out = np.empty_like(sc)
        capi.check(self._lib.rspl_sp_debug_nms(self._h, sc.ctypes.data, sc.shape[0], sc.shape[1], out.ctypes.data),
                   "rspl_sp_debug_nms")
        return out

    LAYERS = ("conv1", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPD", "det_head", "taps")
    _LAYER_IO = {"conv1": (1, 64, True), "conv2a": (64, 64, False), "conv2b": (64, 64, True), "conv3a": (64, 128, False),
                 "conv3b": (128, 128, True), "conv4a": (128, 128, False), "conv4b": (128, 128, False),
                 "convPD": (128, 512, False)}

    def debug_layer(self, stage: str, x: np.ndarray, scores: Optional[np.ndarray] = None, keypoints=None):
        """rspl_sp_debug_layer: one fp16 stage of an RSPL_PREC_FP16 handle on host input (fp16 values as float32).
          conv1                 x u8 [B, H, W]              -> [B, H/2, W/2, 64]
          conv2a .. convPD      x [B, H, W, Cin]            -> [B, H(/2), W(/2), Cout]
          det_head              x cells [B, H8, W8, 512]    -> scores [B, 8 H8, 8 W8]
          taps                  x cells, scores [B, 8 H8, 8 W8], keypoints = per image a list of flat pixel
                                indices -> per image a feature block [n, 259] (float64)"""
        st = self.LAYERS.index(stage)
        B, H, W = x.shape[:3]
        if stage in self._LAYER_IO:
            cin, cout, pool = self._LAYER_IO[stage]
            xin = np.ascontiguousarray(x, np.uint8 if stage == "conv1" else np.float32)
            assert xin.shape == ((B, H, W) if stage == "conv1" else (B, H, W, cin)), xin.shape
            out = np.empty((B, H // 2, W // 2, cout) if pool else (B, H, W, cout), np.float32)
            capi.check(self._lib.rspl_sp_debug_layer(self._h, st, B, H, W, xin.ctypes.data, None, None, None, 0,
                                                     out.ctypes.data, None), "rspl_sp_debug_layer")
            return out
        xin = np.ascontiguousarray(x, np.float32)
        assert xin.shape == (B, H, W, 512), xin.shape
        if stage == "det_head":
            out = np.empty((B, 8 * H, 8 * W), np.float32)
            capi.check(self._lib.rspl_sp_debug_layer(self._h, st, B, H, W, xin.ctypes.data, None, None, None, 0,
                                                     out.ctypes.data, None), "rspl_sp_debug_layer")
            return out
        sc = np.ascontiguousarray(scores, np.float32)
        assert sc.shape == (B, 8 * H, 8 * W) and len(keypoints) == B
        stride = max(1, max(len(k) for k in keypoints))
        kp = np.zeros((B, stride), np.int32)
        cnt = np.array([len(k) for k in keypoints], np.int32)
        for b, k in enumerate(keypoints):
            kp[b, :len(k)] = k
        out = np.empty((B, self._cap(), 259), np.float64)
        cout = np.zeros(B, np.int32)
        capi.check(self._lib.rspl_sp_debug_layer(self._h, st, B, H, W, xin.ctypes.data, sc.ctypes.data, kp.ctypes.data,
                                                 cnt.ctypes.data, stride, out.ctypes.data, cout.ctypes.data),
                   "rspl_sp_debug_layer")
        return [out[b, :cout[b]].copy() for b in range(B)], cout

    def debug_select(self, scores: np.ndarray, desc: np.ndarray, fill: float = 0.0):
        """rspl_sp_debug_select: NMS + candidates, top-k and the fp32 sampler of an RSPL_PREC_FP32 handle on host maps,
        launched as rspl_sp_infer_device launches them.  scores [B, H, W] pre-NMS; desc [B, 256, H/8, W/8]
        (channel-major like the reference tensor; transposed here to the device's cell-major layout).  Every feature
        slot is prefilled with `fill`.  Returns (features [B, capacity, 259] float64 as downloaded, counts [B],
        cand_counts [B])."""
        sc = np.ascontiguousarray(scores, np.float32)
        B, H, W = sc.shape
        d = np.asarray(desc, np.float32)
        assert d.shape == (B, 256, H // 8, W // 8), d.shape
        d = np.ascontiguousarray(d.reshape(B, 256, -1).transpose(0, 2, 1))
        cap = self._cap()
        F = np.full((B, cap, 259), fill, np.float64)
        cnt, cand = np.zeros(B, np.int32), np.zeros(B, np.int32)
        capi.check(self._lib.rspl_sp_debug_select(self._h, sc.ctypes.data, d.ctypes.data, B, H, W, F.ctypes.data, cap,
                                                  cnt.ctypes.data, cand.ctypes.data), "rspl_sp_debug_select")
        return F, cnt, cand

    def debug_maps(self, b: int, height: int, width: int):
        s = np.empty((height, width), np.float32)
        d = np.empty((256, height // 8, width // 8), np.float32)
        capi.check(self._lib.rspl_sp_debug_maps(self._h, b, s.ctypes.data, d.ctypes.data), "rspl_sp_debug_maps")
        return s, d

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rspl_sp_destroy(self._h)
            self._h = C.c_void_p()


@dataclass
class SuperGlueConfig:                # include/read_configs.h:20-28 (+ arena sizing)
    image_width: int = 752
    image_height: int = 480
    weights: str = ""                 # RSPLWT01 blob (replaces onnx_file / engine_file)
    max_keypoints: int = 400
    max_batch: int = 2
    sinkhorn_iterations: int = 100
    precision: int = capi.RSPL_PREC_FP32
    device: int = 0


SINK_KINDS = ("slab", "slab_scratch", "sc", "sc10", "wide")  # rspl_sg_sinkhorn_plan.kind


def sinkhorn_plan(max_keypoints: int, max_batch: int = 1, cu_count: int = 0):
    """rspl_sg_debug_sinkhorn_plan: the Sinkhorn kernel a handle of this size gets on cu_count CUs (0: the current
    device's; any other value touches no device), under RSPL_SG_SINK / RSPL_SG_SINK_G.  Returns None where
    rspl_sg_create would refuse max_batch, else a dict (kind: one of SINK_KINDS)."""
    pl = capi.SgSinkhornPlan()
    if capi.load().rspl_sg_debug_sinkhorn_plan(max_keypoints, max_batch, cu_count, C.byref(pl)) != 0:
        return None
    return dict(kind=SINK_KINDS[pl.kind], groups=pl.groups, rows_per_wave=pl.rows_per_wave,
                ug_granules=pl.ug_granules, vg_granules=pl.vg_granules)


class SuperGlue:
    """Mirror of class SuperGlue (include/super_glue.h:20-71)."""

    def __init__(self, superglue_config: SuperGlueConfig):
        self.config = superglue_config
        self._h = C.c_void_p()
        self._lib = capi.load()
        self.error = None

    def build(self) -> bool:
        c = self.config
        cfg = capi.SgConfig(c.image_width, c.image_height, c.max_keypoints, c.max_batch, c.sinkhorn_iterations,
                            c.precision, c.device)
        rc = self._lib.rspl_sg_create(C.byref(cfg), c.weights.encode(), C.byref(self._h))
        self.error = None if rc == 0 else self._lib.rspl_last_error().decode()
        return rc == 0

    def infer(self, features0: np.ndarray, features1: np.ndarray):
        """SuperGlue::infer (src/super_glue.cpp:137-197) on NORMALISED 259 x n features.
        Returns (ok, indices0, indices1, mscores0, mscores1)."""
        f0 = np.ascontiguousarray(np.asarray(features0, np.float64).T)
        f1 = np.ascontiguousarray(np.asarray(features1, np.float64).T)
        n0, n1 = f0.shape[0], f1.shape[0]
        i0, i1 = np.empty(n0, np.int32), np.empty(n1, np.int32)
        m0, m1 = np.empty(n0, np.float64), np.empty(n1, np.float64)
        rc = self._lib.rspl_sg_infer(self._h, f0.ctypes.data, n0, f1.ctypes.data, n1, i0.ctypes.data, i1.ctypes.data,
                                     m0.ctypes.data, m1.ctypes.data)
        if rc != 0:
            self.error = self._lib.rspl_last_error().decode()
            return False, i0, i1, m0, m1
        return True, i0, i1, m0, m1

    def infer_device(self, batch: int, d_feat0: int, d_n0: int, d_feat1: int, d_n1: int, stride_feat: int,
                     normalize: bool, d_idx0: int, d_idx1: int, d_ms0: int, d_ms1: int, stream=None,
                     post_stream=None) -> None:
        """Device-resident batched SuperGlue; with post_stream, Sinkhorn + decode run there
        (results complete on post_stream) so the next call's GNN overlaps them."""
        if post_stream is None:
            capi.check(self._lib.rspl_sg_infer_device(self._h, batch, d_feat0, d_n0, d_feat1, d_n1, stride_feat,
                                                      int(normalize), d_idx0, d_idx1, d_ms0, d_ms1, stream),
                       "rspl_sg_infer_device")
        else:
            capi.check(self._lib.rspl_sg_infer_device2(self._h, batch, d_feat0, d_n0, d_feat1, d_n1, stride_feat,
                                                       int(normalize), d_idx0, d_idx1, d_ms0, d_ms1, stream,
                                                       post_stream), "rspl_sg_infer_device2")

    STAGES = ("prep+kenc", "gnn x18", "final+scores", "post hand-over", "sinkhorn", "decode")

    def profile(self, enable: bool = True):
        capi.check(self._lib.rspl_sg_profile(self._h, int(enable)), "rspl_sg_profile")

    def stage_times(self):
        return capi.stage_times(None, self._lib.rspl_sg_stage_times, self._h, len(self.STAGES))

    def debug_scores(self, p: int, n0: int, n1: int) -> np.ndarray:
        Z = np.empty((n0 + 1, n1 + 1), np.float32)
        capi.check(self._lib.rspl_sg_debug_scores(self._h, p, Z.ctypes.data), "rspl_sg_debug_scores")
        return Z

    def status(self):
        """rspl_sg_status: (ok, failed-pair bitmask) of the device paths since the last check
        (call after synchronising the stream the results were produced on)."""
        f = C.c_uint32(0)
        rc = self._lib.rspl_sg_status(self._h, C.byref(f))
        if rc != 0:
            self.error = self._lib.rspl_last_error().decode()
        return rc == 0, f.value

    def debug_inject(self, inject: bool, spin_limit: int = 0):
        capi.check(self._lib.rspl_sg_debug_inject(self._h, int(inject), spin_limit), "rspl_sg_debug_inject")

    def debug_sinkhorn(self, scores: np.ndarray, alpha: float, iters: int = 100):
        """bins + log_optimal_transport (superglue.py:185-205) of a host score matrix on the device.
        Returns (ok, Z)."""
        sc = np.ascontiguousarray(scores, np.float32)
        n0, n1 = sc.shape
        Z = np.empty((n0 + 1, n1 + 1), np.float32)
        rc = self._lib.rspl_sg_debug_sinkhorn(self._h, sc.ctypes.data, n0, n1, float(alpha), iters, Z.ctypes.data)
        if rc != 0:
            self.error = self._lib.rspl_last_error().decode()
        return rc == 0, Z

    def debug_decode(self, Z: np.ndarray):
        """The device decode (src/super_glue.cpp:258-367) of a host log-assignment matrix."""
        z = np.ascontiguousarray(Z, np.float32)
        n0, n1 = z.shape[0] - 1, z.shape[1] - 1
        i0, i1 = np.empty(n0, np.int32), np.empty(n1, np.int32)
        m0, m1 = np.empty(n0, np.float64), np.empty(n1, np.float64)
        capi.check(self._lib.rspl_sg_debug_decode(self._h, z.ctypes.data, n0, n1, i0.ctypes.data, i1.ctypes.data,
                                                  m0.ctypes.data, m1.ctypes.data), "rspl_sg_debug_decode")
        return i0, i1, m0, m1

    def debug_layers(self, batch: int, X: np.ndarray, n0, n1, l0: int, l1: int):
        """rspl_sg_debug_layers: GNN layers [l0, l1) of the fp16 engine on host descriptors X
        [2 * max_batch, max_keypoints, 256] (the handle's whole token buffer; the first `batch` pairs run).
        Returns (X after the layers, the next layer's q [2 * batch, max_keypoints, 256] float16 or None)."""
        c = self.config
        Xio = np.array(X, np.float32, order="C")
        assert Xio.shape == (2 * max(1, c.max_batch), c.max_keypoints, 256), Xio.shape
        a0, a1 = np.ascontiguousarray(n0, np.int32), np.ascontiguousarray(n1, np.int32)
        assert a0.shape == (batch,) and a1.shape == (batch,)
        Q = np.zeros((2 * batch, c.max_keypoints, 256), np.float16) if l1 < 18 else None
        capi.check(self._lib.rspl_sg_debug_layers(self._h, batch, Xio.ctypes.data, a0.ctypes.data, a1.ctypes.data, l0, l1,
                                                  Q.ctypes.data if Q is not None else None), "rspl_sg_debug_layers")
        return Xio, Q

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rspl_sg_destroy(self._h)
            self._h = C.c_void_p()


class PointMatching:
    """Mirror of class PointMatching (include/point_matching.h:7-18, src/point_matching.cc)."""

    def __init__(self, superglue_config: SuperGlueConfig):
        self._superglue_config = superglue_config
        self.superglue = SuperGlue(superglue_config)
        if not self.superglue.build():
            print("Erron in superglue building")   # src/point_matching.cc:8 (message kept verbatim)

    def MatchingPoints(self, features0: np.ndarray, features1: np.ndarray, outlier_rejection: bool = False):
        """Returns (num_matches, [(queryIdx, trainIdx, distance)])."""
        f0 = np.ascontiguousarray(np.asarray(features0, np.float64).T)
        f1 = np.ascontiguousarray(np.asarray(features1, np.float64).T)
        cap = max(1, min(f0.shape[0], f1.shape[0]))
        out = (capi.DMatch * cap)()
        n = C.c_int(0)
        capi.check(self.superglue._lib.rspl_pm_match(self.superglue.handle, f0.ctypes.data, f0.shape[0],
                                                     f1.ctypes.data, f1.shape[0], out, cap, C.byref(n),
                                                     int(outlier_rejection)), "rspl_pm_match")
        matches = [(out[i].query_idx, out[i].train_idx, out[i].distance) for i in range(n.value)]
        return n.value, matches

    @staticmethod
    def NormalizeKeypoints(features: np.ndarray, width: int, height: int) -> np.ndarray:
        """src/point_matching.cc:50-62 (host helper; the device path normalises in-kernel)."""
        g = np.array(features, np.float64, copy=True)
        scale = max(width, height) * 0.7
        g[1] = (features[1] - width // 2) / scale
        g[2] = (features[2] - height // 2) / scale
        return g


# ---------------------------------------------------------------------------
# Local BA: LocalmapOptimization (include/g2o_optimization/g2o_optimization.h:15-19)
# ---------------------------------------------------------------------------
class LocalBA:
    """Owns one rspl_ba handle (device arena sized once) and runs dense problems."""

    def __init__(self, max_poses=32, max_points=20000, max_lines=2000, max_edges=200000, device=0):
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.BaConfig(max_poses, max_points, max_lines, max_edges, device)
        capi.check(self._lib.rspl_ba_create(C.byref(cfg), C.byref(self._h)), "rspl_ba_create")

    def run(self, problem, out=None):
        """problem: ba_types.DenseProblem -> ba_types.DenseResult.  out: a DenseResult of a problem with
        the same shapes to write into (no per-call allocation; its previous contents are overwritten)."""
        from .ba_types import DenseResult
        res = out if out is not None and out.fits(problem) else DenseResult.alloc(problem)
        P, R = problem.to_ctypes(), res.to_ctypes()
        capi.check(self._lib.rspl_ba_local(self._h, C.byref(P), C.byref(R)), "rspl_ba_local")
        res.read_back(R)
        return res

    def submit(self, problem, out=None):
        """Queue `problem` for the handle's native tracking thread (rspl_ba_submit: runs the queued calls
        in order; blocks while two are waiting, as the reference's feature thread).  Returns the result
        buffer the call will write (read it after join()); problem and out are kept alive until then."""
        from .ba_types import DenseResult
        res = out if out is not None and out.fits(problem) else DenseResult.alloc(problem)
        P, R = problem.to_ctypes(), res.to_ctypes()
        inflight = self.__dict__.setdefault("_inflight", [])
        inflight.append((problem, res, P, R))
        capi.check(self._lib.rspl_ba_submit(self._h, C.byref(P), C.byref(R)), "rspl_ba_submit")
        return res

    def join(self):
        """Wait for every submitted call (rspl_ba_join); raises on the first failure.  Returns
        (calls, LM iterations summed over them, their summed wall time in ms) since the last join."""
        n, it, ms = C.c_longlong(), C.c_longlong(), C.c_double()
        rc = self._lib.rspl_ba_join(self._h, C.byref(n), C.byref(it), C.byref(ms))
        inflight, self._inflight = self.__dict__.get("_inflight", []), []
        for _, res, _, R in inflight:
            res.read_back(R)
        capi.check(rc, "rspl_ba_join")
        return n.value, it.value, ms.value

    def kernel_timing(self, every: int):
        """HIP-event timing of the LM trials' two launches on every `every`-th call (0: off)."""
        capi.check(self._lib.rspl_ba_kernel_timing(self._h, every), "rspl_ba_kernel_timing")

    def kernel_times(self):
        """{"chunks+solve": (total ms, launches), "update": (total ms, launches)} since the last read."""
        ms, n = (C.c_double * 2)(), (C.c_longlong * 2)()
        capi.check(self._lib.rspl_ba_kernel_times(self._h, ms, n), "rspl_ba_kernel_times")
        return {"chunks+solve": (ms[0], n[0]), "update": (ms[1], n[1])}

    def set_line_jacobian(self, analytic: bool):
        """Line edges' Jacobians: g2o's central difference (False, the default) or its analytic limit (True)."""
        capi.check(self._lib.rspl_ba_set_line_jacobian(self._h, 1 if analytic else 0), "rspl_ba_set_line_jacobian")

    def trace(self, cap=4096):
        """The host timeline of the calls since the last read (rspl_ba_trace): a list of dicts with
        capi.BA_TRACE_FIELDS (times in time.perf_counter seconds); [] with a library that lacks it."""
        if not hasattr(self._lib, "rspl_ba_trace"):
            return []
        buf, n = (C.c_double * (cap * capi.BA_TRACE_W))(), C.c_int()
        capi.check(self._lib.rspl_ba_trace(self._h, buf, cap, C.byref(n)), "rspl_ba_trace")
        a = np.frombuffer(buf, np.float64, n.value * capi.BA_TRACE_W).reshape(n.value, capi.BA_TRACE_W)
        return [dict(zip(capi.BA_TRACE_FIELDS, map(float, row))) for row in a]

    def debug_pairs(self, rebuild=False):
        """Test hook (rspl_ba_debug_pairs): the Schur chunks' edge-pair lists of the last run() -- (pp_off
        [chunks + 1], pp [pairs][4], fused) as that call built them, or (rebuild) built again by the count / scan /
        fill launches."""
        cap_off, cap = 1 << 16, 1 << 20
        while True:
            off, pp = np.zeros(cap_off, np.int32), np.zeros((cap, 4), np.int32)
            nc, n, fused = C.c_int(), C.c_longlong(), C.c_int()
            rc = self._lib.rspl_ba_debug_pairs(self._h, 1 if rebuild else 0, off.ctypes.data, cap_off, pp.ctypes.data,
                                               cap, C.byref(nc), C.byref(n), C.byref(fused))
            if rc and (nc.value + 1 > cap_off or n.value > cap) and cap < 1 << 26:
                cap_off, cap = max(cap_off, nc.value + 1), max(cap, int(n.value))
                continue
            capi.check(rc, "rspl_ba_debug_pairs")
            return off[:nc.value + 1].copy(), pp[:n.value].copy(), bool(fused.value)

    def debug_final(self, problem):
        """Test hook (rspl_ba_debug_final) after run(problem): {"inlier": flags by the classify kernel's final pass in
        the caller's order over the four edge types, "T_dev" / "points" / "lines": the final device state, "T_out":
        the poses the final kernel wrote for the host}."""
        E = sum(problem.n_edges(k) for k in ("mono", "stereo", "mono_line", "stereo_line"))
        npo, nq, nl = problem.pose_q.shape[0], problem.points.shape[0], problem.lines.shape[0]
        inl = np.full(max(E, 1), 255, np.uint8)
        Td, To = np.zeros((max(npo, 1), 8)), np.zeros((max(npo, 1), 8))
        X, L = np.zeros((max(nq, 1), 3)), np.zeros((max(nl, 1), 6))
        capi.check(self._lib.rspl_ba_debug_final(self._h, inl.ctypes.data, Td.ctypes.data, To.ctypes.data, X.ctypes.data,
                                                 L.ctypes.data), "rspl_ba_debug_final")
        return {"inlier": inl[:E], "T_dev": Td[:npo], "T_out": To[:npo], "points": X[:nq], "lines": L[:nl]}

    def use_reserved_cus(self, reserve_cus: int):
        """Confine this handle's kernels to the CUs reserving streams leave free (0 = all CUs)."""
        capi.check(self._lib.rspl_ba_use_reserved_cus(self._h, reserve_cus), "rspl_ba_use_reserved_cus")

    def set_group(self, group: "ShardGroup", rank: int):
        """Landmark-sharded solve: this handle is rank `rank` of an in-process group (one device)."""
        capi.check(self._lib.rspl_ba_set_group(self._h, group.handle, rank), "rspl_ba_set_group")
        self._shard = group  # keep the group alive while the handle uses it

    def set_shard(self, rank: int, nranks: int, host_allreduce):
        """Landmark-sharded solve over any host transport: host_allreduce(x) sums the float64 numpy
        array x in place across the ranks (e.g. a gloo / MPI all-reduce).  The device buffer of each
        per-trial all-reduce is staged through host memory (rspl_allreduce_fn, stream-ordered)."""
        lib = self._lib
        AR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

        def cb(ctx, d_buf, count, stream):
            try:
                h = np.empty(count, np.float64)
                if lib.rspl_memcpy_d2h(h.ctypes.data, d_buf, count * 8, stream):
                    return -1
                host_allreduce(h)
                return 1 if lib.rspl_memcpy_h2d(d_buf, h.ctypes.data, count * 8, stream) else 0
            except Exception:  # the C side turns a non-zero return into RSPL_E_DEVICE
                return -1
        self._ar_cb = AR(cb)  # keep the trampoline alive as long as the handle
        capi.check(lib.rspl_ba_set_shard(self._h, rank, nranks, self._ar_cb, None), "rspl_ba_set_shard")

    def set_comm(self, comm: "Comm"):
        """Landmark-sharded solve across processes / GPUs over RCCL (one rank per GPU)."""
        capi.check(self._lib.rspl_ba_set_comm(self._h, comm.handle), "rspl_ba_set_comm")
        self._shard = comm

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rspl_ba_destroy(self._h)
            self._h = C.c_void_p()


class ShardGroup:
    """rspl_group: nranks LocalBA handles on one device, each driven by its own host thread."""

    def __init__(self, nranks: int):
        self._lib = capi.load()
        self.handle = C.c_void_p()
        self.nranks = nranks
        capi.check(self._lib.rspl_group_create(nranks, C.byref(self.handle)), "rspl_group_create")

    def __del__(self):
        if getattr(self, "handle", None) and self.handle.value:
            self._lib.rspl_group_destroy(self.handle)
            self.handle = C.c_void_p()


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """RCCL unique id (rank 0 makes it; broadcast it out of band, e.g. with torch.distributed)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    capi.check(capi.load().rspl_comm_unique_id(buf), "rspl_comm_unique_id")
    return bytes(buf)


class Comm:
    """rspl_comm: an RCCL communicator (one rank per GPU, xGMI within the node)."""

    def __init__(self, unique_id: bytes, rank: int, nranks: int, device: int = 0):
        self._lib = capi.load()
        self.handle = C.c_void_p()
        self.rank, self.nranks = rank, nranks
        uid = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        capi.check(self._lib.rspl_comm_create(uid, rank, nranks, device, C.byref(self.handle)), "rspl_comm_create")

    def __del__(self):
        if getattr(self, "handle", None) and self.handle.value:
            self._lib.rspl_comm_destroy(self.handle)
            self.handle = C.c_void_p()


def broadcast_comm_id(group, make_id=comm_unique_id) -> bytes:
    """Rank 0 makes the RCCL id, every rank of the host group (hostgroup.HostGroup) receives it."""
    return group.broadcast_bytes(make_id() if group.rank == 0 else b"")


_default_ba = None


def LocalmapOptimization(poses, points, lines, camera_list, mono_point_constraints, stereo_point_constraints,
                         mono_line_constraints, stereo_line_constraints, cfg) -> None:
    """Same signature and in-place semantics as the reference (g2o_optimization.cc:21-252):
    poses / points / lines (dict id -> Pose3d / Position3d / Line3d) are updated, constraint
    ``inlier`` flags are written."""
    from . import ba_types as BT
    global _default_ba
    dp, ids = BT.pack_problem(poses, points, lines, camera_list, mono_point_constraints, stereo_point_constraints,
                              mono_line_constraints, stereo_line_constraints, cfg)
    need = (len(poses), len(points), len(lines),
            max(len(mono_point_constraints), len(stereo_point_constraints), len(mono_line_constraints),
                len(stereo_line_constraints)))
    if _default_ba is None or any(n > c for n, c in zip(need, _default_ba_caps)):
        caps = tuple(max(n, c) for n, c in zip(need, (32, 20000, 2000, 200000)))
        _default_ba = LocalBA(*caps)
        globals()["_default_ba_caps"] = caps
    res = _default_ba.run(dp)
    BT.unpack_result(res, ids, poses, points, lines, mono_point_constraints, stereo_point_constraints,
                     mono_line_constraints, stereo_line_constraints)


_default_ba_caps = (0, 0, 0, 0)


# ---------------------------------------------------------------------------
# Tracking pose optimisation: FrameOptimization (include/g2o_optimization/g2o_optimization.h:20-22)
# ---------------------------------------------------------------------------
class FrameBA:
    """Owns one rspl_frame handle; optimises a batch of independent frames in one launch."""

    def __init__(self, max_batch=64, max_edges=65536, max_points=65536, device=0):
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.FrameConfig(max_batch, max_edges, max_points, device)
        capi.check(self._lib.rspl_frame_create(C.byref(cfg), C.byref(self._h)), "rspl_frame_create")

    def run(self, problems):
        """problems: list of ba_types.FrameProblem -> list of ba_types.FrameResult"""
        from .ba_types import FrameResult, RsplFrameProblem, RsplFrameResult
        res = [FrameResult.alloc(p) for p in problems]
        P = (RsplFrameProblem * len(problems))(*[p.to_ctypes() for p in problems])
        R = (RsplFrameResult * len(problems))(*[r.to_ctypes() for r in res])
        capi.check(self._lib.rspl_frame_optimize(self._h, P, len(problems), R), "rspl_frame_optimize")
        for r, rc in zip(res, R):
            r.read_back(rc)
        return res

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rspl_frame_destroy(self._h)
            self._h = C.c_void_p()


_default_frame = None


def FrameOptimization(poses, points, camera_list, mono_point_constraints, stereo_point_constraints, cfg) -> int:
    """Same signature, in-place semantics and return value as the reference
    (g2o_optimization.cc:256-398): the single pose in ``poses`` is updated, constraint ``inlier``
    flags are written, and the number of inlier constraints is returned."""
    from . import ba_types as BT
    global _default_frame
    fp = BT.pack_frame_problem(poses, points, camera_list, mono_point_constraints, stereo_point_constraints, cfg)
    ne = len(mono_point_constraints) + len(stereo_point_constraints)
    if _default_frame is None or ne > _default_frame_cap[0] or len(points) > _default_frame_cap[1]:
        cap = (max(ne, 65536), max(len(points), 65536))
        _default_frame = FrameBA(max_batch=1, max_edges=cap[0], max_points=cap[1])
        globals()["_default_frame_cap"] = cap
    r = _default_frame.run([fp])[0]
    pose = next(iter(poses.values()))
    pose.q = r.pose_q.copy()
    pose.p = r.pose_p.copy()
    for c, f in zip(mono_point_constraints, r.inlier["mono"]):
        c.inlier = bool(f)
    for c, f in zip(stereo_point_constraints, r.inlier["stereo"]):
        c.inlier = bool(f)
    return r.n_inliers


_default_frame_cap = (0, 0)


# ---------------------------------------------------------------------------
# cv::findFundamentalMat(FM_RANSAC, 3, 0.99) as PointMatching::MatchingPoints calls it (point_matching.cc:34-45)
# ---------------------------------------------------------------------------
class FundamentalRansac:
    """Owns one rspl_fm handle: the F-matrix RANSAC of the outlier rejection for a batch of frames, every
    iteration's 7-point models solved and counted side by side, the sequential acceptance replayed on the
    device.  ``solve`` takes host points; ``enqueue`` / ``fetch`` are the device-resident chain from
    SuperGlue's device indices to filtered indices (``enqueue`` never waits for the device)."""

    def __init__(self, max_batch=1, max_matches=1024, max_iters=1000, device=0):
        self.max_batch, self.max_matches, self.max_iters = int(max_batch), int(max_matches), int(max_iters)
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.FmConfig(self.max_batch, self.max_matches, self.max_iters, device)
        capi.check(self._lib.rspl_fm_create(C.byref(cfg), C.byref(self._h)), "rspl_fm_create")
        self._batch = 0

    @staticmethod
    def _results(R, masks, sizes=None):
        out = []
        for k, (r, m) in enumerate(zip(R, masks)):
            n = sizes[k] if sizes is not None else int(np.count_nonzero(m != 255))
            out.append(dict(n_inliers=r.n_inliers, hypotheses=r.hypotheses, F=np.array(r.F[:]),
                            inlier=m[:n].copy()))
        return out

    def solve(self, problems, threshold=3.0, confidence=0.99):
        """problems: list of (points0 [n, 2], points1 [n, 2]) pixels.  Returns one dict per problem:
        n_inliers (-1: no model, nothing rejected), hypotheses (iterations evaluated), F [9], inlier [n] uint8."""
        keep, P, R = [], [], []
        for a, b in problems:
            p0 = np.ascontiguousarray(a, np.float64).reshape(-1, 2)
            p1 = np.ascontiguousarray(b, np.float64).reshape(-1, 2)
            if p0.shape != p1.shape:
                raise ValueError("FundamentalRansac.solve: points0 and points1 differ in length")
            inl = np.zeros(max(p0.shape[0], 1), np.uint8)
            keep.append((p0, p1, inl))
            P.append(capi.FmProblem(p0.shape[0], p0.ctypes.data_as(C.POINTER(C.c_double)),
                                    p1.ctypes.data_as(C.POINTER(C.c_double)), threshold, confidence))
            r = capi.FmResult()
            r.inlier = inl.ctypes.data_as(C.POINTER(C.c_uint8))
            R.append(r)
        Pa = (capi.FmProblem * max(len(P), 1))(*P)
        Ra = (capi.FmResult * max(len(R), 1))(*R)
        capi.check(self._lib.rspl_fm_solve(self._h, Pa, len(P), Ra), "rspl_fm_solve")
        self._batch = 0
        return self._results(Ra[:len(P)], [k[2] for k in keep], [k[0].shape[0] for k in keep])

    def enqueue(self, frames, stream=None, threshold=3.0, confidence=0.99):
        """frames: list of dicts with the device addresses ``d_features0``, ``d_n0``, ``d_features1``, ``d_n1``,
        ``d_idx0``, ``d_idx1``, ``d_idx0_out``, ``d_idx1_out`` (ints or capi.DeviceBuffer)."""
        F = (capi.FmFrame * max(len(frames), 1))()
        for f, d in zip(F, frames):
            for k in ("d_features0", "d_n0", "d_features1", "d_n1", "d_idx0", "d_idx1", "d_idx0_out", "d_idx1_out"):
                v = d.get(k)
                setattr(f, k, v.ptr if isinstance(v, capi.DeviceBuffer) else v)
            f.threshold = d.get("threshold", threshold)
            f.confidence = d.get("confidence", confidence)
        capi.check(self._lib.rspl_fm_enqueue(self._h, len(frames), F, _stream_handle(stream)), "rspl_fm_enqueue")
        self._batch = len(frames)

    def fetch(self):
        """Wait for the last enqueue.  One dict per frame as ``solve`` returns, inlier per compacted mutual
        match (ascending index of image 0)."""
        if self._batch == 0:
            return []
        R = (capi.FmResult * self._batch)()
        masks = []
        for r in R:
            m = np.full(self.max_matches, 255, np.uint8)  # the library writes 0 / 1 for the frame's matches
            r.inlier = m.ctypes.data_as(C.POINTER(C.c_uint8))
            masks.append(m)
        capi.check(self._lib.rspl_fm_fetch(self._h, R), "rspl_fm_fetch")
        return self._results(R, masks)

    def debug_hypotheses(self, frame=0, max_hyps=1000):
        """the iterations solved for frame `frame` of the last solve / fetched enqueue: (n_models int32 [k],
        counts int32 [k, 3] (-1 where there is no model), F [k, 3, 9])"""
        nm = np.zeros(max_hyps, np.int32)
        cnt = np.zeros((max_hyps, 3), np.int32)
        F = np.zeros((max_hyps, 3, 9))
        k = self._lib.rspl_fm_debug_hypotheses(self._h, frame, max_hyps, nm.ctypes.data, cnt.ctypes.data, F.ctypes.data)
        if k < 0:
            capi.check(k, "rspl_fm_debug_hypotheses")
        nm, cnt, F = nm[:k], cnt[:k].copy(), F[:k].copy()
        dead = np.arange(3)[None, :] >= nm[:, None]
        cnt[dead] = -1
        F[dead] = 0.0
        return nm, cnt, F

    @staticmethod
    def debug_subsets(count, iters, points0, points1):
        """host: the subsets `iters` iterations draw for `count` pairs, int32 [found, 7]"""
        p0 = np.ascontiguousarray(points0, np.float64).reshape(-1, 2)
        p1 = np.ascontiguousarray(points1, np.float64).reshape(-1, 2)
        if p0.shape[0] != count or p1.shape[0] != count:
            raise ValueError("debug_subsets: points do not match count")
        idx = np.zeros((max(iters, 1), 7), np.int32)
        n = C.c_int(0)
        capi.check(capi.load().rspl_fm_debug_subsets(count, iters, p0.ctypes.data, p1.ctypes.data, idx.ctypes.data,
                                                     C.byref(n)), "rspl_fm_debug_subsets")
        return idx[:n.value].copy()

    @staticmethod
    def debug_seven_point(p0, p1):
        """host mirror of the kernel's 7-point solver: [7, 2], [7, 2] -> models [k, 9]"""
        a = np.ascontiguousarray(p0, np.float64).reshape(7, 2)
        b = np.ascontiguousarray(p1, np.float64).reshape(7, 2)
        F = np.zeros((3, 9))
        n = C.c_int(0)
        capi.check(capi.load().rspl_fm_debug_seven_point(a.ctypes.data, b.ctypes.data, F.ctypes.data, C.byref(n)),
                   "rspl_fm_debug_seven_point")
        return F[:n.value].copy()

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rspl_fm_destroy(self._h)
            self._h = C.c_void_p()


# ---------------------------------------------------------------------------
# SolvePnPWithCV (include/g2o_optimization/g2o_optimization.h:24, g2o_optimization.cc:402-461)
# ---------------------------------------------------------------------------
class PnP:
    """Owns one rspl_pnp handle: cv::solvePnPRansac's RANSAC (5-point EPnP hypotheses side by
    side) + refinement, for a batch of frames in one launch."""

    def __init__(self, max_batch=64, max_points=65536, device=0):
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.PnpConfig(max_batch, max_points, device)
        capi.check(self._lib.rspl_pnp_create(C.byref(cfg), C.byref(self._h)), "rspl_pnp_create")

    def solve(self, frames, iterations=100, reprojection_error=20.0, confidence=0.99):
        """frames: list of (K4 = (fx, fy, cx, cy), points [n, 3], keypoints [n, 2]).
        Returns a list of (n_inliers, Rwc [3, 3], twc [3], inlier mask [n] uint8, hypotheses)."""
        keep, P, R = [], [], []
        for K4, pts, kps in frames:
            p3 = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
            p2 = np.ascontiguousarray(kps, np.float64).reshape(-1, 2)
            inl = np.zeros(max(p3.shape[0], 1), np.uint8)
            keep.append((p3, p2, inl))
            P.append(capi.PnpProblem(K4[0], K4[1], K4[2], K4[3], p3.shape[0],
                                     p3.ctypes.data_as(C.POINTER(C.c_double)),
                                     p2.ctypes.data_as(C.POINTER(C.c_double)), iterations, reprojection_error,
                                     confidence))
            r = capi.PnpResult()
            r.inlier = inl.ctypes.data_as(C.POINTER(C.c_uint8))
            R.append(r)
        Pa = (capi.PnpProblem * len(P))(*P)
        Ra = (capi.PnpResult * len(R))(*R)
        capi.check(self._lib.rspl_pnp_solve(self._h, Pa, len(P), Ra), "rspl_pnp_solve")
        return [(r.n_inliers, np.array(r.Rwc[:]).reshape(3, 3), np.array(r.twc[:]), k[2][:k[0].shape[0]].copy(),
                 r.hypotheses) for r, k in zip(Ra, keep)]

    def debug_hypotheses(self, frame=0, max_hyps=128):
        """every hypothesis of frame `frame` of the last solve: (counts int32 [k], -1 = the
        minimal solver failed; poses [k, 12] = R row-major | t)"""
        cnt = np.zeros(max_hyps, np.int32)
        poses = np.zeros((max_hyps, 12))
        k = self._lib.rspl_pnp_debug_hypotheses(self._h, frame, max_hyps, cnt.ctypes.data_as(C.c_void_p),
                                                poses.ctypes.data_as(C.c_void_p))
        if k < 0:
            capi.check(k, "rspl_pnp_debug_hypotheses")
        return cnt[:k], poses[:k]

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rspl_pnp_destroy(self._h)
            self._h = C.c_void_p()


_default_pnp = None


def SolvePnPWithCV(K4, points, keypoints, point_ids=None):
    """The reference's SolvePnPWithCV over already-filtered correspondences (:417-431): returns
    (n_inliers, pose Twc 4x4, inliers) where inliers[i] = point_ids[i] for RANSAC inliers, else -1
    (:452-457; point_ids defaults to the correspondence index)."""
    global _default_pnp
    n = len(points)
    if _default_pnp is None or n > _default_pnp_cap[0]:
        cap = max(n, 65536)
        _default_pnp = PnP(max_batch=1, max_points=cap)
        globals()["_default_pnp_cap"] = (cap,)
    k, Rwc, twc, inl, _ = _default_pnp.solve([(K4, points, keypoints)])[0]
    T = np.eye(4)
    if k > 0:
        T[:3, :3] = Rwc
        T[:3, 3] = twc
    ids = np.arange(n) if point_ids is None else np.asarray(point_ids)
    return k, T, np.where(inl.astype(bool), ids, -1)


_default_pnp_cap = (0,)


# ---------------------------------------------------------------------------
# The tracking step: MapBuilder::TrackFrame + FramePoseOptimization (src/map_builder.cc:448-611)
# ---------------------------------------------------------------------------
TRACK_NO_MAPPOINT, TRACK_GOOD, TRACK_NOT_GOOD = 0, 1, 2  # RSPL_TRACK_*: the keyframe table's states
# RSPL_TRACK_KF_*: the terms of MapBuilder::AddKeyframe in a fetched ``add_keyframe``
TRACK_KF_NOT_ENOUGH_MATCH, TRACK_KF_LARGE_DELTA_ANGLE, TRACK_KF_LARGE_DISTANCE, TRACK_KF_ENOUGH_PASSED_FRAME = 1, 2, 4, 8


class Tracker:
    """Owns one rspl_track handle: SuperGlue's device indices -> pose, inliers and track ids for a batch
    of independent frames as one stream-ordered chain of launches.  ``enqueue`` never waits for the
    device; ``fetch`` waits for the one event it recorded."""

    def __init__(self, max_batch=1, max_keypoints=1024, device=0):
        if max_batch <= 0 or max_keypoints <= 0:  # before the library (and a device) is touched
            raise ValueError(f"Tracker: max_batch {max_batch} and max_keypoints {max_keypoints} must be positive")
        self.max_batch, self.max_keypoints = int(max_batch), int(max_keypoints)
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.TrackConfig(self.max_batch, self.max_keypoints, device)
        capi.check(self._lib.rspl_track_create(C.byref(cfg), C.byref(self._h)), "rspl_track_create")
        self._batch = 0
        self._ext = False  # the last enqueue took the line / decision path

    def set_keyframe(self, slot, points, state, track_id, stream=None):
        """The keyframe's table: per keypoint its map point's world position [n0, 3], state [n0]
        (TRACK_*) and track id [n0].  Host arrays; the upload is asynchronous on ``stream``."""
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        st = np.ascontiguousarray(state, np.uint8).reshape(-1)
        tid = np.ascontiguousarray(track_id, np.int32).reshape(-1)
        if not (pts.shape[0] == st.shape[0] == tid.shape[0]):
            raise ValueError("set_keyframe: points, state and track_id differ in length")
        capi.check(self._lib.rspl_track_set_keyframe(self._h, slot, pts.shape[0], pts.ctypes.data, st.ctypes.data,
                                                     tid.ctypes.data, _stream_handle(stream)),
                   "rspl_track_set_keyframe")

    @staticmethod
    def _frame_descs(frames):
        """rspl_track_frame records of ``enqueue``'s dicts (a missing device address stays NULL)"""
        F = (capi.TrackFrameDesc * max(len(frames), 1))()
        for f, d in zip(F, frames):
            f.slot = d.get("slot", 0)
            for k in ("d_features", "d_n1", "d_idx0", "d_idx1", "d_u_right"):
                v = d.get(k)
                setattr(f, k, v.ptr if isinstance(v, capi.DeviceBuffer) else v)
            f.fx, f.fy, f.cx, f.cy, f.bf = [float(x) for x in d["cam"]]
            f.last_Twc[:] = list(np.asarray(d["last_Twc"], np.float64).reshape(16))
            f.th_mono_point = d.get("th_mono_point", 5.991)
            f.th_stereo_point = d.get("th_stereo_point", 7.815)
            f.min_num_match = d.get("min_num_match", 10)
        return F

    def _enqueued_by(self, batch):
        """another handle (LocalMap.track_enqueue) issued rspl_track_enqueue for ``batch`` frames: ``fetch`` is next"""
        self._batch, self._ext = int(batch), False

    def enqueue(self, frames, stream=None):
        """frames: list of dicts with the device addresses ``d_features``, ``d_n1``, ``d_idx0``, ``d_idx1``
        (ints or capi.DeviceBuffer), optional ``d_u_right``, ``slot`` (default 0), ``cam`` = (fx, fy, cx, cy,
        bf), ``last_Twc`` [4, 4], and optional ``th_mono_point`` / ``th_stereo_point`` (5.991 / 7.815) and
        ``min_num_match`` (10).

        When any frame carries ``d_lines`` or ``keyframe`` the batch goes through rspl_track_enqueue_ext (after
        ``enable_lines``): line tracking against the slot's ``set_keyframe_lines`` and the keyframe decision.
        ``d_lines`` (device [n_lines, 4] doubles) comes with ``n_lines``; ``keyframe`` = dict(Twc [4, 4],
        frame_id) is the last keyframe, ``frame_id`` this frame's; optional ``max_num_match`` (80),
        ``max_angle`` (0.52), ``max_distance`` (0.5), ``max_num_passed_frame`` (300)."""
        F = self._frame_descs(frames)
        self._ext = any("d_lines" in d or "keyframe" in d for d in frames)
        if not self._ext:
            capi.check(self._lib.rspl_track_enqueue(self._h, len(frames), F, _stream_handle(stream)),
                       "rspl_track_enqueue")
        else:
            X = (capi.TrackFrameExt * max(len(frames), 1))()
            for x, d in zip(X, frames):
                v = d.get("d_lines")
                x.d_lines = v.ptr if isinstance(v, capi.DeviceBuffer) else v
                x.n_lines = int(d.get("n_lines", 0))
                kf = d.get("keyframe", {})
                x.kf_Twc[:] = list(np.asarray(kf.get("Twc", np.eye(4)), np.float64).reshape(16))
                x.kf_frame_id, x.frame_id = int(kf.get("frame_id", 0)), int(d.get("frame_id", 0))
                x.max_num_match = int(d.get("max_num_match", 80))
                x.max_angle = float(d.get("max_angle", 0.52))
                x.max_distance = float(d.get("max_distance", 0.5))
                x.max_num_passed_frame = int(d.get("max_num_passed_frame", 300))
            capi.check(self._lib.rspl_track_enqueue_ext(self._h, len(frames), F, X, _stream_handle(stream)),
                       "rspl_track_enqueue_ext")
        self._batch = len(frames)

    def fetch(self):
        """Wait for the last enqueue.  Returns one dict per frame: pose_q (x, y, z, w), pose_p, pose_set,
        n_inliers, n_pnp_inliers, pnp_used, n_keypoints, n_matches, n_kept, n_mono, n_stereo, rounds,
        iterations, chi2 and, per current keypoint, match_kf, track_id, kept.  After an enqueue whose
        frames carried ``d_lines`` or ``keyframe``, also n_lines, n_line_matches, n_line_tracks, overflow,
        tracked_well, add_keyframe (TRACK_KF_* bits), delta_angle, delta_distance, passed_frames and, per
        line of the frame, line_match_kf, line_track_id, line_slot."""
        if self._batch == 0:
            return []
        K = self.max_keypoints
        R = (capi.TrackResult * self._batch)()
        arrs = []
        for r in R:
            a = (np.full(K, -1, np.int32), np.full(K, -1, np.int32), np.zeros(K, np.uint8))
            r.match_kf, r.track_id, r.kept = a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data
            arrs.append(a)
        if not self._ext:
            capi.check(self._lib.rspl_track_fetch(self._h, R), "rspl_track_fetch")
        else:
            ML = self.max_lines
            X = (capi.TrackExtResult * self._batch)()
            larrs = []
            for x in X:
                la = tuple(np.full(ML, -1, np.int32) for _ in range(3))
                x.line_match_kf, x.line_track_id, x.line_slot = (v.ctypes.data for v in la)
                larrs.append(la)
            capi.check(self._lib.rspl_track_fetch_ext(self._h, R, X), "rspl_track_fetch_ext")
        out = []
        for r, a in zip(R, arrs):
            n = r.n_keypoints
            out.append(dict(pose_q=np.array(r.pose_q[:]), pose_p=np.array(r.pose_p[:]), pose_set=bool(r.pose_set),
                            n_inliers=r.n_inliers, n_pnp_inliers=r.n_pnp_inliers, pnp_used=bool(r.pnp_used),
                            n_keypoints=n, n_matches=r.n_matches, n_kept=r.n_kept, n_mono=r.n_mono,
                            n_stereo=r.n_stereo, rounds=r.rounds, iterations=tuple(r.iterations[:]),
                            chi2=tuple(r.chi2[:]), match_kf=a[0][:n].copy(), track_id=a[1][:n].copy(),
                            kept=a[2][:n].astype(bool)))
        if self._ext:
            for o, x, la in zip(out, X, larrs):
                n = x.n_lines
                o.update(n_lines=n, n_line_matches=x.n_line_matches, n_line_tracks=x.n_line_tracks,
                         overflow=bool(x.overflow), tracked_well=bool(x.tracked_well), add_keyframe=x.add_keyframe,
                         delta_angle=x.delta_angle, delta_distance=x.delta_distance, passed_frames=x.passed_frames,
                         line_match_kf=la[0][:n].copy(), line_track_id=la[1][:n].copy(), line_slot=la[2][:n].copy())
        return out

    def enable_lines(self, max_lines=512, max_pairs=65536):
        """Allocate the line side (rspl_track_enable_lines), once per Tracker: up to ``max_lines`` lines per
        frame and per keyframe slot, ``max_pairs`` point-line pairs per frame and per slot."""
        cfg = capi.TrackLinesConfig(int(max_lines), int(max_pairs))
        capi.check(self._lib.rspl_track_enable_lines(self._h, C.byref(cfg)), "rspl_track_enable_lines")
        self.max_lines, self.max_pairs = int(max_lines), int(max_pairs)

    def set_keyframe_lines(self, slot, n_lines, d_lines, d_features, d_n0, line_track_id, line_slot, stream=None):
        """The lines of keyframe slot ``slot``: device lines [n_lines, 4], the keyframe's device SuperPoint
        records and keypoint count (ints or capi.DeviceBuffer), host line track ids and map-line ids [n_lines]."""
        tid = np.ascontiguousarray(line_track_id, np.int32).reshape(-1)
        sl = np.ascontiguousarray(line_slot, np.int32).reshape(-1)
        if not (len(tid) == len(sl) == n_lines):
            raise ValueError("set_keyframe_lines: line_track_id and line_slot must have n_lines entries")
        ptr = [v.ptr if isinstance(v, capi.DeviceBuffer) else v for v in (d_lines, d_features, d_n0)]
        capi.check(self._lib.rspl_track_set_keyframe_lines(self._h, slot, n_lines, *ptr, tid.ctypes.data,
                                                           sl.ctypes.data, _stream_handle(stream)),
                   "rspl_track_set_keyframe_lines")

    def frame_lines(self, frame=0):
        """The device arrays [max_lines] that receive frame ``frame``'s line_track_id / line_slot, for a
        consumer on the device."""
        t, s = C.c_void_p(), C.c_void_p()
        capi.check(self._lib.rspl_track_frame_lines(self._h, frame, C.byref(t), C.byref(s)), "rspl_track_frame_lines")
        return dict(line_track_id=t.value, line_slot=s.value, capacity=self.max_lines)

    def debug_lines(self, frame=0):
        """The point-line assignments behind frame ``frame`` of the last (fetched) enqueue with lines, as CSR
        triples (offsets, point_idx, dist): ``frame`` for the frame's lines, ``keyframe`` for its slot's."""
        D = capi.TrackDebugLines()
        ML, cap = self.max_lines, self.max_pairs
        a = dict(offsets=np.zeros(ML + 1, np.int32), point_idx=np.zeros(cap, np.int32), dist=np.zeros(cap),
                 kf_offsets=np.zeros(ML + 1, np.int32), kf_point_idx=np.zeros(cap, np.int32), kf_dist=np.zeros(cap))
        for k, v in a.items():
            setattr(D, k, v.ctypes.data)
        capi.check(self._lib.rspl_track_debug_lines(self._h, frame, C.byref(D)), "rspl_track_debug_lines")

        def csr(off, idx, dist, nl):
            off = off[:nl + 1].copy()
            n = int(off[-1]) if off[-1] <= cap else 0
            return off, idx[:n].copy(), dist[:n].copy()
        return dict(frame=csr(a["offsets"], a["point_idx"], a["dist"], D.n_lines),
                    keyframe=csr(a["kf_offsets"], a["kf_point_idx"], a["kf_dist"], D.kf_n_lines))

    def debug_stage(self, frame=0):
        """The stages of frame ``frame`` of the last (fetched) enqueue, for the parity tests: the compacted
        correspondences and edges, the RANSAC subsets, PnP's result, the seed pose and FrameOptimization's
        per-edge flags."""
        K = self.max_keypoints
        D = capi.TrackDebug()
        a = dict(corr_kp=np.zeros(K, np.int32), edge_kp=np.zeros(K, np.int32), pnp_points=np.zeros((K, 3)),
                 pnp_keypoints=np.zeros((K, 2)), edges=np.zeros((K, 12)), subsets=np.zeros((128, 5), np.int32),
                 pnp_inlier=np.zeros(K, np.uint8), edge_inlier=np.zeros(K, np.uint8))
        for k, v in a.items():
            setattr(D, k, v.ctypes.data)
        capi.check(self._lib.rspl_track_debug_stage(self._h, frame, C.byref(D)), "rspl_track_debug_stage")
        n = D.n_corr
        return dict(n_corr=n, n_mono=D.n_mono, n_stereo=D.n_stereo, corr_kp=a["corr_kp"][:n], edge_kp=a["edge_kp"][:n],
                    pnp_points=a["pnp_points"][:n], pnp_keypoints=a["pnp_keypoints"][:n], edges=a["edges"][:n],
                    subsets=a["subsets"][:D.n_subsets], pnp_Rwc=np.array(D.pnp_Rwc[:]).reshape(3, 3),
                    pnp_twc=np.array(D.pnp_twc[:]), pnp_n_inliers=D.pnp_n_inliers, pnp_hypotheses=D.pnp_hypotheses,
                    pnp_inlier=a["pnp_inlier"][:n], seed_q=np.array(D.seed_q[:]), seed_p=np.array(D.seed_p[:]),
                    pnp_used=bool(D.pnp_used), edge_inlier=a["edge_inlier"][:n])

    def keyframe_table(self, slot, n0):
        """The device arrays of keyframe slot ``slot`` (points, state, track id) for a producer on the
        device (KeyframeBuilder.enqueue's ``table``); sets the slot's keypoint count to ``n0``."""
        p, s, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        capi.check(self._lib.rspl_track_keyframe_table(self._h, slot, n0, C.byref(p), C.byref(s), C.byref(t)),
                   "rspl_track_keyframe_table")
        return dict(points=p.value, state=s.value, track_id=t.value, capacity=self.max_keypoints)

    def debug_keyframe_table(self, slot, n0):
        """Slot ``slot``'s first ``n0`` table entries read back: (points [n0, 3], state, track_id)."""
        t = self.keyframe_table(slot, n0)
        pts, st, tid = np.zeros((n0, 3)), np.zeros(n0, np.uint8), np.zeros(n0, np.int32)
        for a, k in ((pts, "points"), (st, "state"), (tid, "track_id")):
            if a.nbytes:
                capi.check(self._lib.rspl_memcpy_d2h(a.ctypes.data, t[k], a.nbytes, None), "rspl_memcpy_d2h")
        return pts, st, tid

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rspl_track_destroy(self._h)
            self._h = C.c_void_p()


# ---------------------------------------------------------------------------
# Local map tracking: Map::SearchByProjection (src/map.cc:952-1005) and MapBuilder::TrackLocalMap
# (src/map_builder.cc:753-785) -- dead code in the reference, restated (tests/lmap_ref.py)
# ---------------------------------------------------------------------------
LMAP_NOT_SELECTED, LMAP_BEHIND, LMAP_OFF_IMAGE, LMAP_NO_CANDIDATE, LMAP_FAILED, LMAP_GOOD = range(6)  # RSPL_LMAP_*


def _lmap_frames(frames):
    F = (capi.LmapFrame * max(len(frames), 1))()
    for f, d in zip(F, frames):
        for k in ("d_features", "d_n1", "d_u_right", "d_point_id", "d_point_xyz", "d_point_good"):
            v = d.get(k)
            setattr(f, k, v.ptr if isinstance(v, capi.DeviceBuffer) else v)
        f.Twc[:] = list(np.asarray(d["Twc"], np.float64).reshape(16))
        f.fx, f.fy, f.cx, f.cy, f.bf = [float(x) for x in d["cam"]]
        f.width, f.height = int(d["width"]), int(d["height"])
    return F


class LocalMap:
    """Owns one rspl_lmap handle: the descriptor bank (one fp64 descriptor per map point id, the one stored at the
    point's creation), the ordered local map, and the search by projection of a batch of frames against it --
    alone (``enqueue``) or chained into a Tracker (``track_enqueue``).  Neither enqueue waits for the device.
    ``device`` < 0: a host-only handle (bank and local-table bookkeeping, no device side)."""

    def __init__(self, max_bank_points=65536, max_local_points=8192, max_keypoints=1024, max_batch=1, device=0,
                 radius=15.0, max_distance=0.35, max_ratio=0.6):
        if min(max_bank_points, max_local_points, max_keypoints, max_batch) <= 0:  # before the library is touched
            raise ValueError(f"LocalMap: capacities {max_bank_points}, {max_local_points}, {max_keypoints}, "
                             f"{max_batch} must be positive")
        self.max_local_points, self.max_keypoints, self.max_batch = int(max_local_points), int(max_keypoints), int(max_batch)
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.LmapConfig(int(max_bank_points), self.max_local_points, self.max_keypoints, self.max_batch, device,
                              radius, max_distance, max_ratio)
        capi.check(self._lib.rspl_lmap_create(C.byref(cfg), C.byref(self._h)), "rspl_lmap_create")
        self._batch = 0
        self.n_local = 0

    def store(self, ids, keypoints, d_features, stream=None):
        """Mappoint::SetDescriptor at creation: the descriptors of records ``keypoints`` of the device records
        ``d_features`` [cap, 259] become those of map points ``ids``."""
        a, k = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(keypoints, np.int32)
        if a.shape != k.shape:
            raise ValueError("LocalMap.store: ids and keypoints differ in length")
        d = d_features.ptr if isinstance(d_features, capi.DeviceBuffer) else d_features
        capi.check(self._lib.rspl_lmap_store(self._h, len(a), a.ctypes.data, k.ctypes.data, d, _stream_handle(stream)),
                   "rspl_lmap_store")

    def store_host(self, ids, descriptors):
        a = np.ascontiguousarray(ids, np.int32)
        D = np.ascontiguousarray(descriptors, np.float64).reshape(-1, 256)
        if len(a) != len(D):
            raise ValueError("LocalMap.store_host: ids and descriptors differ in length")
        capi.check(self._lib.rspl_lmap_store_host(self._h, len(a), a.ctypes.data, D.ctypes.data), "rspl_lmap_store_host")

    def bank_size(self) -> int:
        n = C.c_int()
        capi.check(self._lib.rspl_lmap_bank_size(self._h, C.byref(n)), "rspl_lmap_bank_size")
        return n.value

    def set_local(self, ids, positions, stream=None):
        """The local map in order: ids [n] and world positions [n, 3]; every id must have a descriptor."""
        a = np.ascontiguousarray(ids, np.int32)
        P = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        if len(a) != len(P):
            raise ValueError("LocalMap.set_local: ids and positions differ in length")
        capi.check(self._lib.rspl_lmap_set_local(self._h, len(a), a.ctypes.data, P.ctypes.data, _stream_handle(stream)),
                   "rspl_lmap_set_local")
        self.n_local = len(a)

    def enqueue(self, frames, stream=None):
        """frames: list of dicts with the device addresses ``d_features``, ``d_n1``, ``d_point_id``, ``d_point_xyz``
        (ints or capi.DeviceBuffer), optional ``d_u_right`` (None: no dxr term) and ``d_point_good``, ``Twc``
        [4, 4], ``cam`` = (fx, fy, cx, cy, bf), ``width``, ``height``."""
        capi.check(self._lib.rspl_lmap_enqueue(self._h, len(frames), _lmap_frames(frames), _stream_handle(stream)),
                   "rspl_lmap_enqueue")
        self._batch = len(frames)

    def track_enqueue(self, tracker: "Tracker", frames, track_frames, stream=None):
        """The chain: search, merge into ``tracker``'s keyframe slots, then the tracking step.  ``track_frames``:
        Tracker.enqueue's dicts (``slot``, ``d_features``, ``d_n1``, optional ``d_u_right``, ``cam``, ``last_Twc``,
        thresholds); their indices are the handle's own.  Results: ``tracker.fetch()`` and ``fetch()``."""
        if len(frames) != len(track_frames):
            raise ValueError("LocalMap.track_enqueue: frames and track_frames differ in length")
        T = tracker._frame_descs(track_frames)  # (their d_idx0 / d_idx1 are ignored by the library)
        capi.check(self._lib.rspl_lmap_track_enqueue(self._h, tracker._h, len(frames), _lmap_frames(frames), T,
                                                     _stream_handle(stream)), "rspl_lmap_track_enqueue")
        self._batch = len(frames)
        tracker._enqueued_by(len(frames))

    def fetch(self):
        """Wait for the last enqueue.  One dict per frame: n_keypoints, n_selected, n_projected, n_with_candidates,
        n_good, good_kp / good_point (the good projections in local order: keypoint, local index) and assoc_id
        (the merged table: map point id per keypoint or -1)."""
        if self._batch == 0:
            return []
        R = (capi.LmapResult * self._batch)()
        arrs = []
        for r in R:
            a = (np.full(self.max_local_points, -1, np.int32), np.full(self.max_local_points, -1, np.int32),
                 np.full(self.max_keypoints, -1, np.int32))
            r.good_kp, r.good_point, r.assoc_id = (v.ctypes.data for v in a)
            arrs.append(a)
        capi.check(self._lib.rspl_lmap_fetch(self._h, R), "rspl_lmap_fetch")
        return [dict(n_keypoints=r.n_keypoints, n_selected=r.n_selected, n_projected=r.n_projected,
                     n_with_candidates=r.n_with_candidates, n_good=r.n_good, good_kp=a[0][:r.n_good].copy(),
                     good_point=a[1][:r.n_good].copy(), assoc_id=a[2][:r.n_keypoints].copy()) for r, a in zip(R, arrs)]

    def global_enqueue(self, frames, max_distance=0.35, max_ratio=0.6, mutual=True, stream=None):
        """The search of the local table by descriptor alone (relocalisation): mutual nearest neighbours with a
        ratio test.  frames: ``enqueue``'s dicts, of which only ``d_features`` and ``d_n1`` are read.  Never waits
        for the device; ``global_fetch`` is next."""
        F = (capi.LmapFrame * max(len(frames), 1))()
        for f, d in zip(F, frames):
            for k in ("d_features", "d_n1"):
                v = d.get(k)
                setattr(f, k, v.ptr if isinstance(v, capi.DeviceBuffer) else v)
        gp = capi.LmapGlobalParams(float(max_distance), float(max_ratio), int(bool(mutual)))
        capi.check(self._lib.rspl_lmap_global_enqueue(self._h, len(frames), F, C.byref(gp), _stream_handle(stream)),
                   "rspl_lmap_global_enqueue")
        self._gbatch = len(frames)

    def global_fetch(self):
        """Wait for the last global enqueue.  One dict per frame: the counts n_keypoints, n_local, n_pass, n_matched;
        per keypoint arg, best, second, match (local index or -1); per local point kbest; and the matches in
        ascending keypoint order: match_kp, match_local, match_id, match_pos [n, 3], match_xy [n, 2]."""
        B = getattr(self, "_gbatch", 0)
        if B == 0:
            return []
        R = (capi.LmapGlobalResult * B)()
        arrs = [_global_result_arrays(r, self.max_keypoints, self.max_local_points) for r in R]
        capi.check(self._lib.rspl_lmap_global_fetch(self._h, R), "rspl_lmap_global_fetch")
        return [_global_result_dict(r, a) for r, a in zip(R, arrs)]

    def debug_points(self, frame=0):
        """frame ``frame`` of the last fetched enqueue, per local point: dict(status LMAP_*, best_idx, best, second)"""
        n = max(self.n_local, 1)
        st, bi, b, s = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n), np.zeros(n)
        capi.check(self._lib.rspl_lmap_debug_points(self._h, frame, st.ctypes.data, bi.ctypes.data, b.ctypes.data,
                                                    s.ctypes.data), "rspl_lmap_debug_points")
        n = self.n_local
        return dict(status=st[:n], best_idx=bi[:n], best=b[:n], second=s[:n])

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rspl_lmap_destroy(self._h)
            self._h = C.c_void_p()


def lmap_search_host(features, point_id, local_ids, local_pos, local_desc, Twc, cam, width, height, u_right=None,
                     radius=15.0, max_distance=0.35, max_ratio=0.6):
    """rspl_lmap_debug_search_host: the host instantiation of the search text (no device is touched).
    features [n1, 259]; returns dict(status, best_idx, best, second) per local point."""
    F = np.ascontiguousarray(features, np.float64).reshape(-1, 259)
    pid = np.ascontiguousarray(point_id, np.int32)
    ids = np.ascontiguousarray(local_ids, np.int32)
    pos = np.ascontiguousarray(local_pos, np.float64).reshape(-1, 3)
    D = np.ascontiguousarray(local_desc, np.float64).reshape(-1, 256)
    ur = np.ascontiguousarray(u_right, np.float64) if u_right is not None else None
    if len(pid) != len(F) or not (len(ids) == len(pos) == len(D)) or (ur is not None and len(ur) != len(F)):
        raise ValueError("lmap_search_host: array lengths differ")
    p = capi.LmapHostProblem()
    p.n_keypoints, p.features, p.point_id = len(F), F.ctypes.data, pid.ctypes.data
    p.u_right = ur.ctypes.data if ur is not None else None
    p.n_local, p.local_ids, p.local_pos, p.local_desc = len(ids), ids.ctypes.data, pos.ctypes.data, D.ctypes.data
    p.Twc[:] = list(np.asarray(Twc, np.float64).reshape(16))
    p.fx, p.fy, p.cx, p.cy, p.bf = [float(x) for x in cam]
    p.width, p.height = int(width), int(height)
    p.radius, p.max_distance, p.max_ratio = radius, max_distance, max_ratio
    n = max(len(ids), 1)
    st, bi, b, s = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n), np.zeros(n)
    capi.check(capi.load().rspl_lmap_debug_search_host(C.byref(p), st.ctypes.data, bi.ctypes.data, b.ctypes.data,
                                                       s.ctypes.data), "rspl_lmap_debug_search_host")
    n = len(ids)
    return dict(status=st[:n], best_idx=bi[:n], best=b[:n], second=s[:n])


def _global_result_arrays(r, K, L):
    K, L = max(K, 1), max(L, 1)
    a = dict(arg=np.full(K, -1, np.int32), best=np.full(K, 4.0), second=np.full(K, 4.0), match=np.full(K, -1, np.int32),
             kbest=np.full(L, -1, np.int32), match_kp=np.full(K, -1, np.int32), match_local=np.full(K, -1, np.int32),
             match_id=np.full(K, -1, np.int32), match_pos=np.zeros((K, 3)), match_xy=np.zeros((K, 2)))
    for k, v in a.items():
        setattr(r, k, v.ctypes.data)
    return a


def _global_result_dict(r, a):
    out = dict(n_keypoints=r.n_keypoints, n_local=r.n_local, n_pass=r.n_pass, n_matched=r.n_matched)
    for k in ("arg", "best", "second", "match"):
        out[k] = a[k][:r.n_keypoints].copy()
    out["kbest"] = a["kbest"][:r.n_local].copy()
    for k in ("match_kp", "match_local", "match_id", "match_pos", "match_xy"):
        out[k] = a[k][:r.n_matched].copy()
    return out


def lmap_global_host(features, local_ids, local_pos, local_desc, max_distance=0.35, max_ratio=0.6, mutual=True):
    """rspl_lmap_debug_global_host: the global search's contract on host arrays, distances in the fixed summation
    order (no device is touched).  features [n1, 259]; returns ``LocalMap.global_fetch``'s dict."""
    F = np.ascontiguousarray(features, np.float64).reshape(-1, 259)
    ids = np.ascontiguousarray(local_ids, np.int32)
    pos = np.ascontiguousarray(local_pos, np.float64).reshape(-1, 3)
    D = np.ascontiguousarray(local_desc, np.float64).reshape(-1, 256)
    if not (len(ids) == len(pos) == len(D)):
        raise ValueError("lmap_global_host: array lengths differ")
    p = capi.LmapGlobalHostProblem(len(F), F.ctypes.data, len(ids), ids.ctypes.data, pos.ctypes.data, D.ctypes.data)
    gp = capi.LmapGlobalParams(float(max_distance), float(max_ratio), int(bool(mutual)))
    r = capi.LmapGlobalResult()
    a = _global_result_arrays(r, len(F), len(ids))
    capi.check(capi.load().rspl_lmap_debug_global_host(C.byref(p), C.byref(gp), C.byref(r)),
               "rspl_lmap_debug_global_host")
    return _global_result_dict(r, a)


def lmap_global_plan(max_keypoints, max_local_points):
    """rspl_lmap_debug_global_plan: (chunk_rows, qtile_rows, k_slab) of the device search for these capacities"""
    c, q, k = C.c_int(), C.c_int(), C.c_int()
    capi.check(capi.load().rspl_lmap_debug_global_plan(int(max_keypoints), int(max_local_points), C.byref(c),
                                                       C.byref(q), C.byref(k)), "rspl_lmap_debug_global_plan")
    return c.value, q.value, k.value


def Relocalise(map_, local_map: LocalMap, tracker: "Tracker", pnp: "PnP", frame: dict, candidates=None,
               ref_keyframe: Optional[int] = None, min_num_match=10, num_inlier_thr=10, stream=None):
    """Find the camera again without a pose prior (the reference has no such stage: its tracking gives up for good).

    1. candidates: ``(ids, positions)`` sets the local table, ``"map"`` takes ``map_.GoodMappoints()``, None keeps
       the table as set; 2. the global descriptor search (``LocalMap.global_enqueue``) -- fewer than
       max(8, min_num_match) matches: (-1, info), stage "search"; 3. ``pnp.solve`` on the matches (100 iterations,
       20 px, 0.99) -- fewer than min_num_match inliers: (-1, info), stage "pnp"; 4. ``TrackLocalMap`` with
       Twc = last_Twc = PnP's pose (``ref_keyframe`` as there), whose (n_inliers, result) is returned, stage "track".
    ``frame``: TrackLocalMap's dict (its ``Twc`` / ``last_Twc`` are replaced); ``info`` / result carry ``stage``,
    ``n_matched`` and, from step 3 on, ``pnp_inliers`` and ``pnp_Twc``.  Two host synchronisations by design."""
    if isinstance(candidates, str):
        if candidates != "map":
            raise ValueError(f"Relocalise: candidates {candidates!r}")
        candidates = map_.GoodMappoints()
    if candidates is not None:
        local_map.set_local(candidates[0], candidates[1], stream)
    local_map.global_enqueue([frame], stream=stream)
    g = local_map.global_fetch()[0]
    info = dict(stage="search", n_matched=g["n_matched"], n_pass=g["n_pass"])
    if g["n_matched"] < max(8, min_num_match):
        return -1, info
    cam = frame["cam"]
    k, Rwc, twc, inl, _ = pnp.solve([(tuple(cam[:4]), g["match_pos"], g["match_xy"])], 100, 20.0, 0.99)[0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rwc, twc
    info.update(stage="pnp", pnp_inliers=k, pnp_Twc=T)
    if k < min_num_match:
        return -1, info
    n, out = TrackLocalMap(map_, local_map, tracker, dict(frame, Twc=T, last_Twc=T), ref_keyframe, min_num_match,
                           num_inlier_thr, stream)
    out.update(info, stage="track")
    return n, out


def TrackLocalMap(map_, local_map: LocalMap, tracker: "Tracker", frame: dict, ref_keyframe: Optional[int] = None,
                  min_num_match=10, num_inlier_thr=10, stream=None):
    """Reference-shaped MapBuilder::TrackLocalMap (map_builder.cc:753-785) for one frame.

    ``frame``: dict with the device addresses ``d_features``, ``d_n1``, ``d_point_id``, ``d_point_xyz`` (optional
    ``d_u_right``, ``d_point_good``, ``d_track_u_right`` -- the pose optimisation's stereo observations), ``Twc`` (the
    pose to project with, also the last pose of the 0.5 m gate unless ``last_Twc`` is given), ``cam``, ``width``,
    ``height`` and optional ``slot``.  ``ref_keyframe``: when given, the local map is first rebuilt from ``map_``
    (UpdateLocalKeyframes / UpdateLocalMappoints; every point needs a descriptor in the bank); None keeps the local
    map as it was set.  Returns (n_inliers or -1, result): -1 with fewer than 3 good projections or unless
    n_inliers > min_num_match and n_inliers > num_inlier_thr; on success result holds ``pose_q``, ``pose_p``,
    ``track_id`` (per keypoint, -1: none) and the search's counts."""
    if ref_keyframe is not None:
        ids, pos = map_.LocalMappoints(ref_keyframe)
        local_map.set_local(ids, pos, stream)
    tf = dict(slot=frame.get("slot", 0), d_features=frame["d_features"], d_n1=frame["d_n1"],
              d_u_right=frame.get("d_track_u_right"), cam=frame["cam"], last_Twc=frame.get("last_Twc", frame["Twc"]),
              min_num_match=min_num_match)
    local_map.track_enqueue(tracker, [frame], [tf], stream)
    t, s = tracker.fetch()[0], local_map.fetch()[0]
    out = dict(s, n_inliers=t["n_inliers"], pose_set=t["pose_set"])
    if s["n_good"] < 3:
        return -1, out
    n = t["n_inliers"]
    if not (n > min_num_match and n > num_inlier_thr):
        return -1, out
    out.update(pose_q=t["pose_q"], pose_p=t["pose_p"], track_id=t["track_id"])
    return n, out


# ---- loop closure: pose-graph optimisation ---------------------------------------------------
PGO_CONVERGED, PGO_MAX_ITERATIONS, PGO_STALLED = 0, 1, 2  # RSPL_PGO_*


def _pgo_problem(pose_q, pose_p, pose_fixed, edge_i, edge_j, edge_q, edge_p, edge_w):
    """(PgoProblem, the arrays it points into)"""
    q = np.ascontiguousarray(pose_q, np.float64).reshape(-1, 4)
    p = np.ascontiguousarray(pose_p, np.float64).reshape(-1, 3)
    fx = np.ascontiguousarray(pose_fixed, np.uint8).reshape(-1)
    ei = np.ascontiguousarray(edge_i, np.int32).reshape(-1)
    ej = np.ascontiguousarray(edge_j, np.int32).reshape(-1)
    eq = np.ascontiguousarray(edge_q, np.float64).reshape(-1, 4)
    ep = np.ascontiguousarray(edge_p, np.float64).reshape(-1, 3)
    ew = np.ascontiguousarray(edge_w, np.float64).reshape(-1, 2)
    if not (len(q) == len(p) == len(fx)) or not (len(ei) == len(ej) == len(eq) == len(ep) == len(ew)):
        raise ValueError("pose graph: array lengths differ")
    keep = (q, p, fx, ei, ej, eq, ep, ew)
    P = capi.PgoProblem(len(q), q.ctypes.data, p.ctypes.data, fx.ctypes.data, len(ei), ei.ctypes.data, ej.ctypes.data,
                        eq.ctypes.data, ep.ctypes.data, ew.ctypes.data)
    return P, keep


def _pgo_run(fn, what, P, max_iterations, step_tol):
    q, p = np.empty((P.n_poses, 4)), np.empty((P.n_poses, 3))
    R = capi.PgoResult()
    R.pose_q, R.pose_p = q.ctypes.data, p.ctypes.data
    pr = capi.PgoParams(int(max_iterations), float(step_tol))
    capi.check(fn(C.byref(P), C.byref(pr), C.byref(R)), what)
    return dict(pose_q=q, pose_p=p, status=R.status, iterations=R.iterations, trials=R.trials, n_free=R.n_free,
                n_tiles=R.n_tiles, n_filled_tiles=R.n_filled_tiles, cost_initial=R.cost_initial,
                cost_final=R.cost_final, lam=R.lambda_)


class PoseGraph:
    """Owns one rspl_pgo handle: LM over a pose graph on a tile-sparse fp64 Cholesky (the loop-closure correction).
    ``solve`` takes T_wc poses (q xyzw, p), a fixed mask and edges (i, j, Z = T_wi^-1 T_wj as q, p, weights (w_t, w_r))
    and returns a dict: pose_q, pose_p, status (PGO_*), iterations, trials, both costs, lam and the plan's counts."""

    def __init__(self, max_poses=1024, max_edges=8192, max_tiles=512, device=0):
        self._lib = capi.load()
        self._h = C.c_void_p()
        self.max_poses, self.max_edges, self.max_tiles = int(max_poses), int(max_edges), int(max_tiles)
        cfg = capi.PgoConfig(self.max_poses, self.max_edges, self.max_tiles, int(device))
        capi.check(self._lib.rspl_pgo_create(C.byref(cfg), C.byref(self._h)), "rspl_pgo_create")

    def solve(self, pose_q, pose_p, pose_fixed, edge_i, edge_j, edge_q, edge_p, edge_w, max_iterations=0, step_tol=0.0):
        P, keep = _pgo_problem(pose_q, pose_p, pose_fixed, edge_i, edge_j, edge_q, edge_p, edge_w)
        return _pgo_run(lambda *a: self._lib.rspl_pgo_solve(self._h, *a), "rspl_pgo_solve", P, max_iterations, step_tol)

    def system(self, pose_q, pose_p, pose_fixed, edge_i, edge_j, edge_q, edge_p, edge_w, lam, dense=True):
        """rspl_pgo_debug_system: (e [E][6], b, H dense or None, delta) of one linearisation and one solve at lam"""
        P, keep = _pgo_problem(pose_q, pose_p, pose_fixed, edge_i, edge_j, edge_q, edge_p, edge_w)
        n = 6 * int((keep[2] == 0).sum())
        e, b, d = np.zeros((P.n_edges, 6)), np.zeros(n), np.zeros(n)
        H = np.zeros((n, n)) if dense else None
        capi.check(self._lib.rspl_pgo_debug_system(self._h, C.byref(P), float(lam), e.ctypes.data, b.ctypes.data,
                                                   H.ctypes.data if dense else None, d.ctypes.data),
                   "rspl_pgo_debug_system")
        return e, b, H, d

    def close(self):
        if self._h:
            self._lib.rspl_pgo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()


def pgo_system(pose_graph: PoseGraph, *problem, lam, dense=True):
    """rspl_pgo_debug_system on a PoseGraph handle (see PoseGraph.system)"""
    return pose_graph.system(*problem, lam=lam, dense=dense)


def pgo_host(pose_q, pose_p, pose_fixed, edge_i, edge_j, edge_q, edge_p, edge_w, max_iterations=0, step_tol=0.0):
    """rspl_pgo_debug_host: the solver's host twin (same arithmetic text, tile plan and LM rule); no device"""
    P, keep = _pgo_problem(pose_q, pose_p, pose_fixed, edge_i, edge_j, edge_q, edge_p, edge_w)
    return _pgo_run(capi.load().rspl_pgo_debug_host, "rspl_pgo_debug_host", P, max_iterations, step_tol)


def pgo_plan(pose_fixed, edge_i, edge_j, tile_map=False):
    """rspl_pgo_debug_plan: dict n_free, tiles_per_side, n_tiles, n_filled_tiles (and tile_map [nt][nt])"""
    n = len(pose_fixed)
    q = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1))
    ne = len(edge_i)
    P, keep = _pgo_problem(q, np.zeros((n, 3)), pose_fixed, edge_i, edge_j, np.tile(q[:1], (ne, 1)), np.zeros((ne, 3)),
                           np.ones((ne, 2)))
    nf, nt, ns, nfl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    lib = capi.load()
    capi.check(lib.rspl_pgo_debug_plan(C.byref(P), C.byref(nf), C.byref(nt), C.byref(ns), C.byref(nfl), None, 0),
               "rspl_pgo_debug_plan")
    out = dict(n_free=nf.value, tiles_per_side=nt.value, n_tiles=ns.value, n_filled_tiles=nfl.value)
    if tile_map:
        tm = np.empty((nt.value, nt.value), np.int32)
        capi.check(lib.rspl_pgo_debug_plan(C.byref(P), None, None, None, None, tm.ctypes.data, tm.size),
                   "rspl_pgo_debug_plan")
        out["tile_map"] = tm
    return out


def _rt_to_qp(R, t):
    """a rotation matrix and a translation as (q xyzw, p)"""
    from .trajectory import quat_from_R
    q = quat_from_R(np.asarray(R, np.float64))
    return q / np.linalg.norm(q), np.asarray(t, np.float64).copy()


def CloseLoop(map_, local_map: LocalMap, pnp: "PnP", pose_graph: PoseGraph, frame: dict, keyframe_id: int,
              min_votes=20, min_inliers=30, min_gap=10, min_weight=1, stream=None):
    """Loop closure for keyframe ``keyframe_id``, whose features are ``frame`` (``d_features``, ``d_n1``, ``cam``):

    1. the global descriptor search of the frame over ``map_.GoodMappoints()``; 2. ``map_.LoopCandidates`` on the
    matched ids -- a best candidate below ``min_votes``: (False, info), stage "vote"; 3. ``pnp.solve`` (100
    iterations, 20 px, 0.99, as ``Relocalise``) on the matches whose point the candidate or one of its connections
    observes -- fewer than ``min_inliers`` inliers: (False, info), stage "pnp"; 4. ``map_.PoseGraph(min_weight)`` plus
    one loop edge from the candidate to the keyframe with Z = T_cand^-1 T_pnp, all weights 1, the lowest-id keyframe
    fixed; 5. ``pose_graph.solve``, then ``map_.ApplyPoseGraph``.  Returns (True, info) with ``cost_initial``,
    ``cost_final``, ``iterations``, ``status``, ``candidate``, ``votes``, ``pnp_inliers``.  Tracker slots and the
    local table hold the old poses and positions afterwards: refresh them."""
    ids, pos = map_.GoodMappoints()
    local_map.set_local(ids, pos, stream)
    local_map.global_enqueue([frame], stream=stream)
    g = local_map.global_fetch()[0]
    nm = g["n_matched"]
    mid = np.asarray(g["match_id"][:nm], np.int32)
    cand, votes = map_.LoopCandidates(keyframe_id, mid, min_gap)
    info = dict(stage="vote", n_matched=nm, candidate=int(cand[0]) if len(cand) else -1,
                votes=int(votes[0]) if len(votes) else 0)
    if len(cand) == 0 or votes[0] < min_votes:
        return False, info
    c = int(cand[0])
    near = {c} | {f for _, f in map_.GetOrderedConnections(c)}
    keep = np.array([k for k in range(nm) if near & set(map_.GetMappoint(int(mid[k]))[2])], np.int64)
    cam = frame["cam"]
    k, Rwc, twc, inl, _ = pnp.solve([(tuple(cam[:4]), g["match_pos"][:nm][keep], g["match_xy"][:nm][keep])], 100, 20.0,
                                    0.99)[0]
    info.update(stage="pnp", n_near=len(keep), pnp_inliers=k)
    if k < min_inliers:
        return False, info
    G = map_.PoseGraph(min_weight)
    fid = G["frame_ids"]
    ic, ik = int(np.searchsorted(fid, c)), int(np.searchsorted(fid, keyframe_id))
    Tc = map_.GetPose(c)
    Rz = Tc[:3, :3].T @ np.asarray(Rwc).reshape(3, 3)
    lq, lp = _rt_to_qp(Rz, Tc[:3, :3].T @ (np.asarray(twc, np.float64) - Tc[:3, 3]))
    fixed = np.zeros(len(fid), np.uint8)
    fixed[0] = 1
    E = len(G["edge_i"]) + 1
    out = pose_graph.solve(G["pose_q"], G["pose_p"], fixed, np.append(G["edge_i"], ic), np.append(G["edge_j"], ik),
                           np.vstack([G["edge_q"], lq]), np.vstack([G["edge_p"], lp]), np.ones((E, 2)))
    map_.ApplyPoseGraph(fid, out["pose_q"], out["pose_p"])
    info.update(stage="done", cost_initial=out["cost_initial"], cost_final=out["cost_final"],
                iterations=out["iterations"], status=out["status"], pnp_Rwc=np.asarray(Rwc).reshape(3, 3),
                pnp_twc=np.asarray(twc, np.float64))
    return True, info


from .synthetic import stereo_window  # noqa: E402  (Camera's disparity window from bf and the depth thresholds)

KF_NEW_NONE, KF_NEW_GOOD, KF_NEW_UNTRIANGULATED = 0, 1, 2  # RSPL_KF_NEW_*
KF_TRI_FEW, KF_TRI_OK, KF_TRI_RANK = 0, 1, 2               # RSPL_KF_TRI_*


class KeyframeBuilder:
    """Owns one rspl_kf handle: SuperGlue's device indices of a stereo pair -> u_right, depth, new track
    ids, new map points and (optionally) a Tracker slot, for a batch of independent frames in one launch
    (MapBuilder::InsertKeyframe, Frame::AddRightFeatures, the map-point half of Map::InsertKeyframe); and
    Map::TriangulateMappoint as one batched call.  ``enqueue`` never waits for the device."""

    def __init__(self, max_batch=1, max_keypoints=1024, max_tri_points=4096, max_tri_observations=65536, device=0):
        if max_batch <= 0 or max_keypoints <= 0 or max_tri_points < 0 or max_tri_observations < 0:
            raise ValueError(f"KeyframeBuilder: bad capacities {max_batch}, {max_keypoints}, {max_tri_points}, "
                             f"{max_tri_observations}")
        self.max_batch, self.max_keypoints = int(max_batch), int(max_keypoints)
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.KfConfig(self.max_batch, self.max_keypoints, int(max_tri_points), int(max_tri_observations), device)
        capi.check(self._lib.rspl_kf_create(C.byref(cfg), C.byref(self._h)), "rspl_kf_create")
        self._batch = 0

    def enqueue(self, frames, stream=None):
        """frames: list of dicts with the device addresses ``d_features_left``, ``d_features_right``,
        ``d_n_left``, ``d_n_right``, ``d_idx0``, ``d_idx1`` (ints or capi.DeviceBuffer), ``cam`` = (fx, fy, cx,
        cy, bf), ``Twc`` [4, 4], ``next_track_id``, and optional ``window`` = (min_x_diff, max_x_diff,
        max_y_diff; default stereo_window(bf)), ``init`` (False), the host arrays ``track_id``, ``point_slot``, ``points``, ``state`` and
        ``table`` (Tracker.keyframe_table's dict)."""
        F = (capi.KfFrameDesc * max(len(frames), 1))()
        keep = []
        for f, d in zip(F, frames):
            for k in ("d_features_left", "d_features_right", "d_n_left", "d_n_right", "d_idx0", "d_idx1"):
                v = d.get(k)
                setattr(f, k, v.ptr if isinstance(v, capi.DeviceBuffer) else v)
            n = 0
            for k, dt in (("track_id", np.int32), ("point_slot", np.int32), ("points", np.float64), ("state", np.uint8)):
                if d.get(k) is not None:
                    a = np.ascontiguousarray(d[k], dt)
                    keep.append(a)
                    setattr(f, k, a.ctypes.data)
                    n = max(n, len(a))
            f.n = n
            f.fx, f.fy, f.cx, f.cy, f.bf = [float(x) for x in d["cam"]]
            f.min_x_diff, f.max_x_diff, f.max_y_diff = [float(x) for x in d.get("window") or stereo_window(f.bf)]
            f.Twc[:] = list(np.asarray(d["Twc"], np.float64).reshape(16))
            f.next_track_id = int(d.get("next_track_id", 0))
            f.init = int(bool(d.get("init", False)))
            t = d.get("table")
            if t is not None:
                f.d_table_points, f.d_table_state, f.d_table_track_id = t["points"], t["state"], t["track_id"]
                f.table_capacity = t["capacity"]
        capi.check(self._lib.rspl_kf_enqueue(self._h, len(frames), F, _stream_handle(stream)), "rspl_kf_enqueue")
        self._batch = len(frames)

    def fetch(self):
        """Wait for the last enqueue.  One dict per frame: the counts n_keypoints, n_matches,
        n_stereo_matches, n_new_ids, n_new_points, n_new_good, next_track_id and, per left keypoint, u_right,
        depth, track_id, new_point (KF_NEW_*), new_position [n, 3]."""
        if self._batch == 0:
            return []
        K = self.max_keypoints
        R = (capi.KfResult * self._batch)()
        arrs = []
        for r in R:
            a = dict(u_right=np.zeros(K), depth=np.zeros(K), track_id=np.zeros(K, np.int32),
                     new_point=np.zeros(K, np.uint8), new_position=np.zeros((K, 3)))
            for k, v in a.items():
                setattr(r, k, v.ctypes.data)
            arrs.append(a)
        capi.check(self._lib.rspl_kf_fetch(self._h, R), "rspl_kf_fetch")
        self._batch = 0
        out = []
        for r, a in zip(R, arrs):
            n = r.n_keypoints
            d = {k: getattr(r, k) for k in ("n_keypoints", "n_matches", "n_stereo_matches", "n_new_ids",
                                            "n_new_points", "n_new_good", "next_track_id")}
            d.update({k: v[:n].copy() for k, v in a.items()})
            out.append(d)
        return out

    def triangulate(self, Twc, camera, offsets, obs_pose, obs_xy, host=False):
        """Map::TriangulateMappoint for len(offsets) - 1 points (a CSR of observers in ascending frame id;
        obs_pose -1 skips one).  ``host``: the host instantiation of the same routine.  Returns (position
        [n, 3], status [n] KF_TRI_*)."""
        return triangulate_points(Twc, camera, offsets, obs_pose, obs_xy, None if host else self)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.rspl_kf_destroy(self._h)
            self._h = C.c_void_p()


def triangulate_points(Twc, camera, offsets, obs_pose, obs_xy, kf: Optional[KeyframeBuilder] = None):
    """rspl_kf_triangulate; ``kf`` None runs the host instantiation (no device is touched)."""
    T = np.ascontiguousarray(Twc, np.float64).reshape(-1, 16)
    cam = np.ascontiguousarray(camera, np.float64)[:4].copy()
    off = np.ascontiguousarray(offsets, np.int32)
    op = np.ascontiguousarray(obs_pose, np.int32)
    xy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
    n = len(off) - 1
    pos, st = np.zeros((max(n, 0), 3)), np.zeros(max(n, 0), np.uint8)
    lib = capi.load()
    capi.check(lib.rspl_kf_triangulate(kf._h if kf is not None else None, len(T), T.ctypes.data, cam.ctypes.data, n,
                                       off.ctypes.data, op.ctypes.data, xy.ctypes.data, pos.ctypes.data,
                                       st.ctypes.data), "rspl_kf_triangulate")
    return pos, st


def _stream_handle(stream):
    return stream.handle if isinstance(stream, capi.Stream) else stream


_default_tracker = None


def TrackFrame(frame0, frame1, matches, camera, last_Twc, cfg=None, min_num_match=10):
    """Reference-shaped MapBuilder::TrackFrame (map_builder.cc:448-504) over host data, in place.

    frame0: dict(points [n0, 3], state [n0], track_id [n0]) -- the keyframe's map points per keypoint;
    frame1: dict(features [259, n1] as SuperPoint returns them, optional u_right [n1], track_id [n1] int
    array, pose [4, 4]); matches: list of (queryIdx, trainIdx) into frame0 / frame1; camera = (fx, fy,
    cx, cy, bf).  As the reference does it sets frame1["pose"] and frame1["track_id"][idx1] and erases
    the matches that did not survive -- when more than min_num_match inliers are left -- and returns the
    inlier count."""
    global _default_tracker
    F1 = np.ascontiguousarray(frame1["features"], np.float64)
    n0, n1 = len(frame0["state"]), F1.shape[1]
    cap = max(n0, n1, 1)
    if _default_tracker is None or cap > _default_tracker.max_keypoints:
        _default_tracker = Tracker(max_batch=1, max_keypoints=max(cap, 1024))
    tr = _default_tracker
    idx0 = np.full(max(n0, 1), -1, np.int32)
    idx1 = np.full(max(n1, 1), -1, np.int32)
    for q, t in matches:
        idx0[q], idx1[t] = t, q
    bufs = []

    def dev(a):
        b = capi.DeviceBuffer(max(a.nbytes, 8))
        if a.nbytes:
            b.upload(a)
        bufs.append(b)
        return b

    fr = dict(d_features=dev(np.ascontiguousarray(F1.T)), d_n1=dev(np.array([n1], np.int32)), d_idx0=dev(idx0),
              d_idx1=dev(idx1), cam=camera, last_Twc=last_Twc, min_num_match=min_num_match)
    if frame1.get("u_right") is not None:
        fr["d_u_right"] = dev(np.ascontiguousarray(frame1["u_right"], np.float64))
    if cfg is not None:
        fr["th_mono_point"], fr["th_stereo_point"] = cfg.mono_point, cfg.stereo_point
    tr.set_keyframe(0, frame0["points"], frame0["state"], frame0["track_id"])
    tr.enqueue([fr])
    r = tr.fetch()[0]
    if r["pose_set"]:
        T = np.eye(4)
        from .synthetic import quat_xyzw_to_R
        T[:3, :3] = quat_xyzw_to_R(r["pose_q"])
        T[:3, 3] = r["pose_p"]
        frame1["pose"] = T
        for q, t in matches:
            if r["kept"][t]:
                frame1["track_id"][t] = r["track_id"][t]
        matches[:] = [(q, t) for q, t in matches if r["kept"][t]]
    return r["n_inliers"]
