"""RCF: the reference's edge network (include/rcf.h, src/rcf.cpp) over librspl's rspl_rcf_*.

``RCF(weights)`` loads an RSPLWT01 blob with the VGG16-based RCF's state_dict names (weights.rcf_shapes) and
``infer(image)`` returns the u8 edge image RCF::infer produces (src/rcf.cpp:95-159), which the line detector
reads in place of the camera image (src/map_builder.cc:286, :327).  ``infer_device`` is the stream-ordered
form on device images, in the layout ``Rectifier.enqueue_device`` writes.  There is no CPU path: without the
library or a device, the calls raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

STAGES = 6  # RSPL_RCF_STAGES
OUTPUT_FUSE = 5  # which of the six maps is the edge image: 0..4 sigmoid(so_1..5), 5 sigmoid(fuse)


def _ptr(v):
    return v.ptr if isinstance(v, capi.DeviceBuffer) else v


def _stream(s):
    return s.handle if isinstance(s, capi.Stream) else s


class RCF:
    """Owns one rspl_rcf handle: the weights and every activation buffer on the device."""

    def __init__(self, weights, max_height=480, max_width=752, max_batch=2, precision=capi.RSPL_PREC_FP32,
                 output=OUTPUT_FUSE, device=0):
        self.max_height, self.max_width, self.max_batch = int(max_height), int(max_width), int(max_batch)
        self.precision, self.output = int(precision), int(output)
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.RcfConfig(self.max_height, self.max_width, self.max_batch, self.precision, self.output, device)
        capi.check(self._lib.rspl_rcf_create(C.byref(cfg), str(weights).encode(), C.byref(self._h)), "rspl_rcf_create")

    def infer(self, image):
        """Gray u8 host image [H, W] in, u8 edge image [H, W] out (RCF::infer)."""
        image = np.asarray(image)
        if image.ndim != 2 or image.dtype != np.uint8:
            raise ValueError(f"infer: a gray u8 image expected, got {image.shape} {image.dtype}")
        if image.strides[1] != 1 or image.strides[0] < image.shape[1]:
            image = np.ascontiguousarray(image)
        H, W = image.shape
        edges = np.empty((H, W), np.uint8)
        capi.check(self._lib.rspl_rcf_infer(self._h, image.ctypes.data, H, W, image.strides[0], edges.ctypes.data),
                   "rspl_rcf_infer")
        return edges

    def infer_device(self, d_images, batch, H, W, stride, pitch, d_edges, out_stride, out_pitch, stream=None):
        """``batch`` device images (d_images + b*pitch, row stride ``stride``) to edge images at
        d_edges + b*out_pitch (row stride out_stride), stream-ordered; never waits for the device."""
        capi.check(self._lib.rspl_rcf_infer_device(self._h, _ptr(d_images), int(batch), int(H), int(W), stride, pitch,
                                                   _ptr(d_edges), out_stride, out_pitch, _stream(stream)),
                   "rspl_rcf_infer_device")

    def debug_logits(self, b, which, H, W):
        """The pre-sigmoid map ``which`` (0..4 so_1..5, 5 fuse) of image b of the last call, [H, W] float32."""
        out = np.empty((H, W), np.float32)
        capi.check(self._lib.rspl_rcf_debug_logits(self._h, int(b), int(which), out.ctypes.data),
                   "rspl_rcf_debug_logits")
        return out

    def profile(self, enable=True):
        capi.check(self._lib.rspl_rcf_profile(self._h, int(bool(enable))), "rspl_rcf_profile")

    def stage_times(self):
        """([ms of stages 1..5 and the tail, summed over the profiled calls], calls)"""
        return capi.stage_times(None, self._lib.rspl_rcf_stage_times, self._h, STAGES)

    def debug_tile_rows(self, rows):
        """Test hook: 8- or 16-row conv tiles for the calls that follow, 0 for the size-based choice."""
        capi.check(self._lib.rspl_rcf_debug_tile_rows(self._h, int(rows)), "rspl_rcf_debug_tile_rows")

    def close(self):
        if self._h:
            self._lib.rspl_rcf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
