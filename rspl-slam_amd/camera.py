"""Camera: the reference's calibration class (include/camera.h, src/camera.cc) over librspl's rspl_rect_*.

``Camera(camera_file)`` reads the OpenCV-YAML calibration the reference's configs carry, builds both cameras'
undistort-rectify maps (cv::initUndistortRectifyMap or its fisheye twin, restated in csrc/rect.cpp) and
``UndistortImage`` remaps a raw stereo pair on the device (cv::remap, INTER_LINEAR, restated in
csrc/rect_kernels.hip).  ``Rectifier`` is the handle underneath, for callers that hold K, D, R, P themselves
or maps exported from OpenCV.  There is no CPU remap: without the library or a device, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import capi

MAX_DIM = 2044  # rect::kMaxDim: the table's 11-bit coordinates
MAX_BATCH = 1024


def read_opencv_yaml(path):
    """The subset of cv::FileStorage's YAML the calibration files use: ``key: scalar`` lines and
    ``key: !!opencv-matrix`` blocks (rows, cols, dt, data: [...], possibly over several lines), behind a
    ``%YAML:1.0`` directive.  Matrices come back as float64 arrays [rows, cols]."""
    with open(path) as f:
        lines = [ln.split("#", 1)[0].rstrip() for ln in f]
    out, i = {}, 0
    while i < len(lines):
        ln = lines[i]
        i += 1
        if not ln.strip() or ln.startswith("%") or ln.strip() == "---":
            continue
        m = re.match(r"^([A-Za-z_][\w.]*)\s*:\s*(.*)$", ln)
        if not m:
            raise ValueError(f"{path}: cannot read line {i}: {ln!r}")
        key, val = m.group(1), m.group(2).strip()
        if val.startswith("!!opencv-matrix"):
            block = []
            while i < len(lines) and (not lines[i].strip() or lines[i][0] in " \t"):
                block.append(lines[i].strip())
                i += 1
            text = " ".join(block)
            rc = {k: int(v) for k, v in re.findall(r"\b(rows|cols)\s*:\s*(\d+)", text)}
            data = re.search(r"data\s*:\s*\[(.*?)\]", text)
            if "rows" not in rc or "cols" not in rc or data is None:
                raise ValueError(f"{path}: matrix {key} lacks rows, cols or data")
            vals = [float(t) for t in data.group(1).replace(",", " ").split()]
            if len(vals) != rc["rows"] * rc["cols"]:
                raise ValueError(f"{path}: matrix {key} has {len(vals)} values for {rc['rows']}x{rc['cols']}")
            out[key] = np.array(vals, np.float64).reshape(rc["rows"], rc["cols"])
        else:
            try:
                out[key] = int(val)
            except ValueError:
                try:
                    out[key] = float(val)
                except ValueError:
                    out[key] = val.strip("\"'")
    return out


def rect_camera(K, D, R, P, distortion_type=0) -> capi.RectCamera:
    """K [3,3], D (k1 k2 p1 p2 [k3 [k4 k5 k6]] or the fisheye k1..k4), R [3,3], P [3,4] as a RectCamera.
    Thin-prism / tilt terms (coefficients past the eighth) must be zero: they are not modelled."""
    K, R, P = (np.asarray(a, np.float64) for a in (K, R, P))
    D = np.asarray(D, np.float64).ravel()
    if K.size != 9 or R.size != 9 or P.size != 12:
        raise ValueError(f"camera: K, R, P have {K.size}, {R.size}, {P.size} entries; 9, 9, 12 expected")
    limit = 4 if distortion_type == 1 else 8
    if np.any(D[limit:] != 0):
        raise ValueError(f"camera: distortion coefficients past the {limit}th are not modelled and must be 0")
    c = capi.RectCamera()
    c.K[:] = K.ravel().tolist()
    c.R[:] = R.ravel().tolist()
    c.P[:] = P.ravel().tolist()
    c.D[:] = (D[:limit].tolist() + [0.0] * 8)[:8]
    return c


def build_maps(cam: capi.RectCamera, distortion_type, height, width):
    """The float maps (map_x, map_y) [H, W] of one camera, on the host (rspl_rect_build_maps)."""
    mx, my = np.empty((height, width), np.float32), np.empty((height, width), np.float32)
    capi.check(capi.load().rspl_rect_build_maps(C.byref(cam), int(distortion_type), int(height), int(width),
                                                mx.ctypes.data, my.ctypes.data), "rspl_rect_build_maps")
    return mx, my


def _ptr(v):
    return v.ptr if isinstance(v, capi.DeviceBuffer) else v


def _stream(s):
    return s.handle if isinstance(s, capi.Stream) else s


class Rectifier:
    """Owns one rspl_rect handle: both cameras' maps as a fixed-point table on the device."""

    def __init__(self, height, width, cams, distortion_type=0, max_batch=2, device=0):
        if not (0 < height <= MAX_DIM and 0 < width <= MAX_DIM):
            raise ValueError(f"Rectifier: image {width}x{height}, sizes are 1..{MAX_DIM}")
        if not 0 < max_batch <= MAX_BATCH or distortion_type not in (0, 1):
            raise ValueError(f"Rectifier: max_batch {max_batch}, distortion_type {distortion_type}")
        self.height, self.width, self.max_batch = int(height), int(width), int(max_batch)
        self.distortion_type = int(distortion_type)
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.RectConfig(self.height, self.width, self.distortion_type, (capi.RectCamera * 2)(*cams),
                              self.max_batch, device)
        capi.check(self._lib.rspl_rect_create(C.byref(cfg), C.byref(self._h)), "rspl_rect_create")

    def get_maps(self, cam):
        mx = np.empty((self.height, self.width), np.float32)
        my = np.empty_like(mx)
        capi.check(self._lib.rspl_rect_get_maps(self._h, cam, mx.ctypes.data, my.ctypes.data), "rspl_rect_get_maps")
        return mx, my

    def set_maps(self, cam, map_x, map_y):
        """Replace camera ``cam``'s maps, e.g. by maps exported from OpenCV's initUndistortRectifyMap."""
        mx, my = (np.ascontiguousarray(m, np.float32) for m in (map_x, map_y))
        if mx.shape != (self.height, self.width) or my.shape != mx.shape:
            raise ValueError(f"set_maps: maps {mx.shape}, {my.shape}; {(self.height, self.width)} expected")
        capi.check(self._lib.rspl_rect_set_maps(self._h, cam, mx.ctypes.data, my.ctypes.data), "rspl_rect_set_maps")

    def enqueue_device(self, d_raw, raw_stride, raw_pitch, cam_index, d_out, out_stride, out_pitch, stream=None):
        """Remap len(cam_index) raw device images (d_raw + b*raw_pitch) through the maps of camera
        cam_index[b] into d_out + b*out_pitch, stream-ordered; never waits for the device."""
        idx = (C.c_int * max(len(cam_index), 1))(*[int(c) for c in cam_index])
        capi.check(self._lib.rspl_rect_enqueue_device(self._h, len(cam_index), _ptr(d_raw), raw_stride, raw_pitch, idx,
                                                      _ptr(d_out), out_stride, out_pitch, _stream(stream)),
                   "rspl_rect_enqueue_device")

    def pair(self, left, right):
        """Host pair in, rectified host pair out (Camera::UndistortImage)."""
        left, right = np.asarray(left), np.asarray(right)
        shape = (self.height, self.width)
        if left.shape != shape or right.shape != shape or left.dtype != np.uint8 or right.dtype != np.uint8:
            raise ValueError(f"pair: u8 images of shape {shape} expected, got {left.shape} {left.dtype}, "
                             f"{right.shape} {right.dtype}")
        if left.strides != right.strides or left.strides[1] != 1 or left.strides[0] < self.width:
            left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
        lo, ro = np.empty(shape, np.uint8), np.empty(shape, np.uint8)
        capi.check(self._lib.rspl_rect_pair(self._h, left.ctypes.data, right.ctypes.data, left.strides[0],
                                            lo.ctypes.data, ro.ctypes.data, self.width), "rspl_rect_pair")
        return lo, ro

    def close(self):
        if self._h:
            self._lib.rspl_rect_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Camera:
    """include/camera.h.  The calibration is read at construction; the device handle is created on the
    first rectification, so the accessors work without a device."""

    _MATS = ("LEFT.K", "RIGHT.K", "LEFT.P", "RIGHT.P", "LEFT.R", "RIGHT.R", "LEFT.D", "RIGHT.D")

    def __init__(self, camera_file, max_batch=2, device=0):
        cfg = read_opencv_yaml(camera_file)
        missing = [k for k in self._MATS if not isinstance(cfg.get(k), np.ndarray) or cfg[k].size == 0]
        if missing or not cfg.get("image_height") or not cfg.get("image_width"):
            raise ValueError(f"{camera_file}: calibration parameters to rectify stereo are missing: "
                             f"{missing or 'image_height / image_width'}")
        for k in ("bf", "depth_lower_thr", "depth_upper_thr", "max_y_diff"):
            if k not in cfg:
                raise ValueError(f"{camera_file}: {k} is missing")
        self._image_height, self._image_width = int(cfg["image_height"]), int(cfg["image_width"])
        self._bf = float(cfg["bf"])
        self._depth_lower_thr, self._depth_upper_thr = float(cfg["depth_lower_thr"]), float(cfg["depth_upper_thr"])
        self._max_x_diff = self._bf / self._depth_lower_thr
        self._min_x_diff = self._bf / self._depth_upper_thr
        self._max_y_diff = float(cfg["max_y_diff"])
        P_l = cfg["LEFT.P"]
        self._fx, self._fy, self._cx, self._cy = P_l[0, 0], P_l[1, 1], P_l[0, 2], P_l[1, 2]
        self._fx_inv, self._fy_inv = 1.0 / self._fx, 1.0 / self._fy
        self.distortion_type = int(cfg.get("distortion_type", 0))
        if self.distortion_type not in (0, 1):
            self.distortion_type = 1  # camera.cc:52-62: anything but 0 takes the fisheye branch
        self.cams = [rect_camera(cfg[s + ".K"], cfg[s + ".D"], cfg[s + ".R"], cfg[s + ".P"], self.distortion_type)
                     for s in ("LEFT", "RIGHT")]
        self._max_batch, self._device = max_batch, device
        self._rect = None

    @property
    def rectifier(self) -> Rectifier:
        if self._rect is None:
            self._rect = Rectifier(self._image_height, self._image_width, self.cams, self.distortion_type,
                                   self._max_batch, self._device)
        return self._rect

    def maps(self, cam):
        """(map_x, map_y) of camera 0 / 1: the reference's _mapl1/_mapl2, _mapr1/_mapr2.  Host only."""
        return build_maps(self.cams[cam], self.distortion_type, self._image_height, self._image_width)

    def UndistortImage(self, image_left, image_right):
        return self.rectifier.pair(image_left, image_right)

    def undistort_device(self, d_raw, raw_stride, raw_pitch, cam_index, d_out, out_stride, out_pitch, stream=None):
        """The device form: see Rectifier.enqueue_device.  The output layout is rspl_sp_infer_device's."""
        self.rectifier.enqueue_device(d_raw, raw_stride, raw_pitch, cam_index, d_out, out_stride, out_pitch, stream)

    def ImageHeight(self):
        return float(self._image_height)

    def ImageWidth(self):
        return float(self._image_width)

    def BF(self):
        return self._bf

    def Fx(self):
        return self._fx

    def Fy(self):
        return self._fy

    def Cx(self):
        return self._cx

    def Cy(self):
        return self._cy

    def DepthLowerThr(self):
        return self._depth_lower_thr

    def DepthUpperThr(self):
        return self._depth_upper_thr

    def MaxXDiff(self):
        return self._max_x_diff

    def MinXDiff(self):
        return self._min_x_diff

    def MaxYDiff(self):
        return self._max_y_diff

    def GetCamerMatrix(self):
        return np.array([[self._fx, 0.0, self._cx], [0.0, self._fy, self._cy], [0.0, 0.0, 1.0]])

    def GetDistCoeffs(self):
        return np.zeros((5, 1))

    def BackProjectMono(self, keypoint):
        return np.array([(keypoint[0] - self._cx) * self._fx_inv, (keypoint[1] - self._cy) * self._fy_inv, 1.0])

    def BackProjectStereo(self, keypoint):
        d = self._bf / (keypoint[0] - keypoint[2])
        return self.BackProjectMono(keypoint[:2]) * d
