"""The RCF edge network on the device (rspl_rcf_*, rspl_slam_amd.RCF) against the restatement (tests/rcf_ref.py)
under the synthetic weights: all six pre-sigmoid maps and the u8 edge image in both precisions, at the smallest
size, one past a tile edge, odd at every pooling level, whole tiles, and a batch with padded strides and
pitches; determinism, untouched padding, the output selector, the host contract and the chain behind
rectification on one stream.

Tolerances come from the restatement alone.  fp32: 8 x the largest difference between the restatement in
float32 and in float64 on the case (the factor covers the MFMA's other summation order over up to 4608
products).  fp16: 4 x the largest difference between the fp16 restatement accumulated in float32 and in float64.
Each parity test prints a ``RCF_PARITY`` line with what it measured (profiles/rcf_parity.json is collected
from them)."""
import functools
import json

import numpy as np
import pytest

import rcf_ref as RR
from conftest import pkg
from rcf_cases import BATCH, SINGLE, rcf_blob
from rspl_slam_amd import capi

pytestmark = pytest.mark.gpu

FILL = 0xAB
MAX_H, MAX_W, MAX_B = 64, 96, 3
GROUPS = {f"{h}x{w}": [(h, w, s)] for h, w, s in SINGLE}
GROUPS["3x40x56"] = BATCH


@functools.lru_cache(maxsize=None)
def _rcf(precision, output=5):
    return pkg.RCF(rcf_blob(), max_height=MAX_H, max_width=MAX_W, max_batch=MAX_B, precision=precision, output=output)


def _run(rcf, images, pad=False, stream=None):
    """One rspl_rcf_infer_device call on `images` (all of one size).  Returns the edge images and the logits
    [B, 6, H, W]; every byte of the output buffer that is no pixel must keep its fill."""
    B = len(images)
    H, W = images[0].shape
    in_stride, out_stride = (W + 8, W + 4) if pad else (W, W)
    in_pitch, out_pitch = H * in_stride + (24 if pad else 0), H * out_stride + (40 if pad else 0)
    src = np.full((B, in_pitch), 0x5C, np.uint8)  # a read of the input's padding would change the result
    for b, im in enumerate(images):
        src[b, :H * in_stride].reshape(H, in_stride)[:, :W] = im
    d_in, d_out = capi.DeviceBuffer(src.nbytes), capi.DeviceBuffer(B * out_pitch)
    d_in.upload(src)
    d_out.upload(np.full(d_out.nbytes, FILL, np.uint8))
    s = stream or capi.Stream()
    rcf.infer_device(d_in, B, H, W, in_stride, in_pitch, d_out, out_stride, out_pitch, s)
    got = d_out.download((B, out_pitch), np.uint8, stream=s.handle)
    edges = []
    for b in range(B):
        rows = got[b, :H * out_stride].reshape(H, out_stride)
        assert np.all(rows[:, W:] == FILL) and np.all(got[b, H * out_stride:] == FILL), f"padding of image {b}"
        edges.append(rows[:, :W].copy())
    logits = np.stack([np.stack([rcf.debug_logits(b, k, H, W) for k in range(6)]) for b in range(B)])
    return edges, logits


def _images(group):
    return [RR.test_image(h, w, s) for h, w, s in GROUPS[group]]


def _refs(group, dtype, fp16=False):
    return np.stack([RR.reference(h, w, dtype, fp16, s)["logits"] for h, w, s in GROUPS[group]])


@pytest.mark.parametrize("group", list(GROUPS))
def test_fp32_logits_and_edge_image(group):
    ref64, ref32 = _refs(group, "float64"), _refs(group, "float32")
    ref_err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    tol = 8 * ref_err
    edges, logits = _run(_rcf(capi.RSPL_PREC_FP32), _images(group), pad=len(GROUPS[group]) > 1)
    err = np.abs(logits.astype(np.float64) - ref64).reshape(len(edges), 6, -1).max(axis=(0, 2))
    ref_edges = [RR.edge_image(r[5]) for r in ref64]
    diff = [np.abs(e.astype(int) - r.astype(int)) for e, r in zip(edges, ref_edges)]
    worst, frac = max(int(d.max()) for d in diff), max(float((d > 0).mean()) for d in diff)
    print("RCF_PARITY", json.dumps({"case": group, "precision": "fp32", "reference_error": ref_err, "tolerance": tol,
                                    "logit_error": [float(e) for e in err], "edge_max_level_diff": worst,
                                    "edge_fraction_differing": frac}))
    assert ref_err > 0 and err.max() <= tol, (err, tol)
    # truncation at an integer boundary is the only allowed difference: one level, at most 1 % of the pixels
    assert worst <= 1 and frac <= 0.01, (worst, frac)


@pytest.mark.parametrize("group", list(GROUPS))
def test_fp16_logits_and_edge_image(group):
    ref32, ref64 = _refs(group, "float32", True), _refs(group, "float64", True)
    ref_err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    tol = 4 * ref_err
    edges, logits = _run(_rcf(capi.RSPL_PREC_FP16), _images(group), pad=len(GROUPS[group]) > 1)
    err = np.abs(logits.astype(np.float64) - ref32.astype(np.float64)).reshape(len(edges), 6, -1).max(axis=(0, 2))
    ref_edges = [RR.edge_image(r[5]) for r in ref32]
    worst = max(int(np.abs(e.astype(int) - r.astype(int)).max()) for e, r in zip(edges, ref_edges))
    print("RCF_PARITY", json.dumps({"case": group, "precision": "fp16", "reference_error": ref_err, "tolerance": tol,
                                    "logit_error": [float(e) for e in err], "edge_max_level_diff": worst}))
    assert ref_err > 0 and err.max() <= tol, (err, tol)
    assert worst <= 2, worst


@pytest.mark.parametrize("precision", [capi.RSPL_PREC_FP32, capi.RSPL_PREC_FP16])
def test_two_runs_agree_bit_for_bit(precision):
    """The side branches sum in a fixed order (no float atomics): the same call twice, with another size run in
    between so every buffer is dirty, gives identical logits and bytes."""
    rcf = _rcf(precision)
    images = _images("3x40x56")
    e1, l1 = _run(rcf, images, pad=True)
    _run(rcf, _images("37x51"))
    e2, l2 = _run(rcf, images, pad=True)
    assert l1.tobytes() == l2.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(e1, e2))
    # an image's result does not depend on its place in the batch
    e3, l3 = _run(rcf, images[1:2])
    assert l3[0].tobytes() == l1[1].tobytes() and e3[0].tobytes() == e1[1].tobytes()


@pytest.mark.parametrize("precision", [capi.RSPL_PREC_FP32, capi.RSPL_PREC_FP16])
def test_both_conv_tiles_give_the_same_bits(precision):
    """Layers past a size threshold run 16-row tiles, which no quick test image reaches: forced through the
    test hook, the 16-row kernels (stage 5's dilated ones included) give the parity-tested 8-row result bit
    for bit -- at 17 x 33 with a second tile row of one pixel row, odd at every level, and on whole tiles."""
    rcf = _rcf(precision)
    try:
        for group in ("17x33", "37x51", "64x80", "3x40x56"):
            images = _images(group)
            rcf.debug_tile_rows(8)
            e8, l8 = _run(rcf, images)
            rcf.debug_tile_rows(16)
            e16, l16 = _run(rcf, images)
            assert l8.tobytes() == l16.tobytes(), group
            assert all(a.tobytes() == b.tobytes() for a, b in zip(e8, e16)), group
            rcf.debug_tile_rows(0)
            e0, l0 = _run(rcf, images)
            assert l0.tobytes() == l8.tobytes(), group
    finally:
        rcf.debug_tile_rows(0)
    assert capi.load().rspl_rcf_debug_tile_rows(rcf._h, 12) == -1


def test_output_selects_the_matching_map():
    images = _images("37x51")
    ref64 = _refs("37x51", "float64")[0]
    seen = []
    for k in range(6):
        edges, logits = _run(_rcf(capi.RSPL_PREC_FP32, k), images)
        want = RR.edge_image(ref64[k])
        assert np.abs(edges[0].astype(int) - want.astype(int)).max() <= 1, k
        own = RR.edge_image(logits[0, k])  # the handle's own map k through the host's sigmoid
        assert np.abs(edges[0].astype(int) - own.astype(int)).max() <= 1, k
        seen.append(edges[0].tobytes())
    assert len(set(seen)) == 6


def test_host_contract():
    rcf = _rcf(capi.RSPL_PREC_FP32)
    H, W = 37, 51
    im = RR.test_image(H, W)
    dev, _ = _run(rcf, [im])
    assert rcf.infer(im).tobytes() == dev[0].tobytes()
    wide = np.full((H, W + 13), 0x5C, np.uint8)  # rows of a wider buffer: the strided host path
    wide[:, 5:5 + W] = im
    assert rcf.infer(wide[:, 5:5 + W]).tobytes() == dev[0].tobytes()
    with pytest.raises(ValueError):
        rcf.infer(im.astype(np.float32))
    # refusals: RSPL_E_ARG, nothing is launched
    lib, h = capi.load(), rcf._h
    buf = capi.DeviceBuffer(2 * MAX_B * MAX_H * MAX_W)
    out = buf.offset(MAX_B * MAX_H * MAX_W)

    def rc(batch=1, H=H, W=W, stride=None, pitch=None):
        stride = W if stride is None else stride
        pitch = H * stride if pitch is None else pitch
        return lib.rspl_rcf_infer_device(h, buf.ptr, batch, H, W, stride, pitch, out, stride, pitch, None)

    assert rc(H=15) == -1 and rc(W=15) == -1 and rc(H=MAX_H + 1) == -1 and rc(W=MAX_W + 1) == -1
    assert b"sizes are" in lib.rspl_last_error()
    assert rc(stride=W - 1) == -1 and rc(batch=2, pitch=H * W - 1) == -1
    assert rc(batch=MAX_B + 1) == -1 and b"max_batch" in lib.rspl_last_error()
    assert rc(batch=-1) == -1
    assert lib.rspl_rcf_infer_device(h, None, 1, H, W, W, H * W, out, W, H * W, None) == -1
    edges = np.empty((H, W), np.uint8)
    assert lib.rspl_rcf_infer(h, im.ctypes.data, 15, W, W, edges.ctypes.data) == -1
    assert lib.rspl_rcf_debug_logits(h, 1, 5, edges.ctypes.data) == -1  # image 1 of a call of one
    assert lib.rspl_rcf_debug_logits(h, 0, 6, edges.ctypes.data) == -1
    assert rc(batch=0) == 0 and rc(H=16, W=16) == 0 and rc(H=MAX_H, W=MAX_W, batch=MAX_B) == 0
    capi.synchronize()
    again, _ = _run(rcf, [im])
    assert again[0].tobytes() == dev[0].tobytes()


def test_chain_behind_rectification_on_one_stream():
    """rspl_rect_enqueue_device and rspl_rcf_infer_device queued on one stream with nothing between them equal
    the two stages run one after the other with the host in between."""
    from rect_cases import synthetic_pair
    from rspl_slam_amd import camera
    H, W = 48, 80
    cams = synthetic_pair(W, H, 60, 0)
    rect = pkg.Rectifier(H, W, [camera.rect_camera(*c, 0) for c in cams], 0, 2)
    rcf = _rcf(capi.RSPL_PREC_FP32)
    raws = [RR.test_image(H, W, 3), RR.test_image(H, W, 4)]
    s = capi.Stream()
    d_raw, d_rect, d_edge = capi.DeviceBuffer(2 * H * W), capi.DeviceBuffer(2 * H * W), capi.DeviceBuffer(2 * H * W)
    d_raw.upload(np.stack(raws))
    d_rect.zero(s.handle)
    d_edge.zero(s.handle)
    rect.enqueue_device(d_raw, W, H * W, [0, 1], d_rect, W, H * W, s)
    rcf.infer_device(d_rect, 2, H, W, W, H * W, d_edge, W, H * W, s)
    chained = d_edge.download((2, H, W), np.uint8, stream=s.handle)
    left, right = rect.pair(*raws)
    assert left.any() and right.any()
    apart, _ = _run(rcf, [left, right])
    assert chained[0].tobytes() == apart[0].tobytes() and chained[1].tobytes() == apart[1].tobytes()
    assert len(np.unique(chained)) >= 64
