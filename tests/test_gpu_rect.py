"""Stereo rectification on the device (rspl_rect_*, rspl_slam_amd.Camera): the remap kernel against the
restatement (tests/rect_ref.py), bitwise on random u8 images -- crafted maps at every rounding and border
seam, synthetic calibrations of both models whose view crosses the source's border, the sizes around the
kernel's tile and lane widths, both reference calibrations at their own size, the host contract, and the chain
into SuperPoint on one stream."""
import ctypes as C
import pathlib
import re
import tempfile

import numpy as np
import pytest

import rect_ref as RR
from conftest import pkg
from rect_cases import CALIB, SYNTHETIC, crafted_maps, ref_maps, synthetic_pair
from rspl_slam_amd import camera, capi

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
FILL = 0xAB


def _kernel_constant(name):
    hpp = (ROOT / "rspl-slam_amd" / "csrc" / "rect_kernels.hpp").read_text()
    expr = re.search(r"constexpr int %s = ([^;]+);" % name, hpp).group(1)
    for other in re.findall(r"k[A-Z]\w+", expr):
        expr = expr.replace(other, str(_kernel_constant(other)))
    return int(eval(expr, {"__builtins__": {}}))  # products of integers


TILE_W, TILE_H = _kernel_constant("kTileW"), _kernel_constant("kTileH")


def _images(rng, n, H, W):
    return [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(n)]


def _rectifier(W, H, model=0, max_batch=6, f=None):
    f = f if f is not None else 0.6 * max(W, H) + 1
    cams = synthetic_pair(W, H, f, model)
    return pkg.Rectifier(H, W, [camera.rect_camera(*c, model) for c in cams], model, max_batch), cams


def _run(rect, raws, cam_index, maps, in_stride=None, out_stride=None, gap=(0, 0), out_offset=0):
    """Remap `raws` in one launch and compare every image with the restatement, and every byte of the output
    buffer that is not a pixel with the fill it had before."""
    H, W = rect.height, rect.width
    B = len(raws)
    in_stride, out_stride = in_stride or W, out_stride or W
    in_pitch, out_pitch = H * in_stride + gap[0], H * out_stride + gap[1]
    src = np.zeros((B, in_pitch), np.uint8)
    for b, im in enumerate(raws):
        rows = src[b, :H * in_stride].reshape(H, in_stride)
        rows[:, :W] = im
        rows[:, W:] = 0x5C  # never a tap: a read of the input's padding would show
    d_in = capi.DeviceBuffer(src.nbytes)
    d_in.upload(src)
    d_out = capi.DeviceBuffer(out_offset + B * out_pitch)
    d_out.upload(np.full(d_out.nbytes, FILL, np.uint8))
    s = capi.Stream()
    rect.enqueue_device(d_in, in_stride, in_pitch, cam_index, d_out.offset(out_offset), out_stride, out_pitch, s)
    got = d_out.download((d_out.nbytes,), np.uint8, stream=s.handle)
    assert np.all(got[:out_offset] == FILL)
    got = got[out_offset:].reshape(B, out_pitch)
    for b, (im, c) in enumerate(zip(raws, cam_index)):
        rows = got[b, :H * out_stride].reshape(H, out_stride)
        assert rows[:, :W].tobytes() == RR.remap(im, *maps[c]).tobytes(), f"image {b} (camera {c})"
        assert np.all(rows[:, W:] == FILL) and np.all(got[b, H * out_stride:] == FILL), f"padding of image {b}"
    return got


def test_crafted_maps_at_every_seam():
    """Every pairing of the CPU test's crafted coordinates, x with y, placed through rspl_rect_set_maps;
    input stride 80, output stride 88 with its padding left as it was."""
    H, W = 40, 72
    rect, _ = _rectifier(W, H)
    mx, my = crafted_maps(H, W)
    maps = [(mx, my), (np.ascontiguousarray(mx[::-1, ::-1]), np.ascontiguousarray(my[::-1, ::-1]))]
    for c in (0, 1):
        rect.set_maps(c, *maps[c])
        gx, gy = rect.get_maps(c)
        assert gx.tobytes() == maps[c][0].tobytes() and gy.tobytes() == maps[c][1].tobytes()
    counts = np.bincount(RR.classes(mx, my, H, W).ravel(), minlength=3)
    assert counts.min() >= 100, counts
    rng = np.random.default_rng(1)
    _run(rect, _images(rng, 4, H, W), [0, 1, 1, 0], maps, in_stride=80, out_stride=88, gap=(16, 24))


@pytest.mark.parametrize("whf", sorted(SYNTHETIC))
@pytest.mark.parametrize("model", [0, 1])
def test_synthetic_calibrations_cross_the_border(whf, model):
    W, H, f = whf
    rect, cams = _rectifier(W, H, model, max_batch=6, f=f)
    maps = [ref_maps(c, model, H, W) for c in cams]
    for c in (0, 1):  # from the restatement alone: the case does exercise all three classes
        counts = np.bincount(RR.classes(*maps[c], H, W).ravel(), minlength=3)
        assert counts.min() >= 100, (c, counts)
        gx, gy = rect.get_maps(c)  # the handle's maps are the restatement's, bit for bit
        assert gx.tobytes() == maps[c][0].tobytes() and gy.tobytes() == maps[c][1].tobytes()
    rng = np.random.default_rng(W)
    _run(rect, _images(rng, 6, H, W), [0, 1, 0, 1, 0, 1], maps)
    _run(rect, _images(rng, 3, H, W), [1, 1, 0], maps, in_stride=W + 5, out_stride=W + 4)


SEAMS = [(37, 23), (1, 1), (4, 1), (5, 3)] + [(w, h) for w in (TILE_W - 1, TILE_W, TILE_W + 1)
                                              for h in (TILE_H - 1, TILE_H, TILE_H + 1)]


@pytest.mark.parametrize("wh", SEAMS)
def test_sizes_at_the_tile_and_lane_seams(wh):
    """Random coordinates from three pixels outside to three pixels outside, on sizes one below, at and one
    above the workgroup's tile, and below a lane's four pixels; odd input strides; output rows both 4-byte
    aligned (vector stores) and not (byte stores)."""
    W, H = wh
    rect, _ = _rectifier(W, H, max_batch=3)
    rng = np.random.default_rng(1000 * W + H)
    maps = []
    for c in (0, 1):
        mx = rng.uniform(-3, W + 3, (H, W)).astype(np.float32)
        my = rng.uniform(-3, H + 3, (H, W)).astype(np.float32)
        mx.flat[0], my.flat[-1] = np.nan, -np.inf
        rect.set_maps(c, mx, my)
        maps.append((mx, my))
    odd = (W + 2) | 1
    aligned = (W + 3) // 4 * 4 + 4
    _run(rect, _images(rng, 3, H, W), [0, 1, 0], maps, in_stride=odd, out_stride=aligned, gap=(1, 4))
    _run(rect, _images(rng, 2, H, W), [1, 0], maps, in_stride=odd + 2, out_stride=W + 1, gap=(0, 3))
    _run(rect, _images(rng, 1, H, W), [1], maps, out_offset=1)  # an unaligned base with packed rows


@pytest.mark.parametrize("name", ["euroc", "uma_bumblebee"])
def test_golden_calibrations_at_full_size(name):
    cam = pkg.Camera(CALIB / f"{name}.yaml")
    H, W = int(cam.ImageHeight()), int(cam.ImageWidth())
    maps = [RR.build_maps(list(c.K), list(c.D), list(c.R), list(c.P), cam.distortion_type, H, W) for c in cam.cams]
    if name == "euroc":  # the workload's own shape and the plain path: no pixel of the left camera leaves the
        # source, and of the right one only 50 of the last row reach half a pixel below it
        assert np.all(RR.classes(*maps[0], H, W) == 2)
        assert np.bincount(RR.classes(*maps[1], H, W).ravel(), minlength=3).tolist() == [0, 50, H * W - 50]
    rng = np.random.default_rng(7)
    raws = _images(rng, 2, H, W)
    _run(cam.rectifier, raws, [0, 1], maps)
    left, right = cam.UndistortImage(*raws)
    assert left.tobytes() == RR.remap(raws[0], *maps[0]).tobytes()
    assert right.tobytes() == RR.remap(raws[1], *maps[1]).tobytes()


def test_host_contract():
    W, H, f = 96, 64, 60
    cams = synthetic_pair(W, H, f, 0)
    # a Camera over a calibration file written for the case
    text = (CALIB / "euroc.yaml").read_text()
    text = text.replace("image_height: 480", f"image_height: {H}").replace("image_width: 752", f"image_width: {W}")
    for side, (K, D, R, P) in zip(("LEFT", "RIGHT"), cams):
        for key, val in (("K", K), ("D", D), ("R", R), ("P", P)):
            text = re.sub(r"(%s\.%s:.*?data: )\[[^\]]*\]" % (side, key), lambda m: m.group(1) + repr(list(map(float, val))),
                          text, flags=re.S)
    with tempfile.TemporaryDirectory() as d:
        (pathlib.Path(d) / "cam.yaml").write_text(text)
        cam = pkg.Camera(pathlib.Path(d) / "cam.yaml", max_batch=2)
    maps = [ref_maps(c, 0, H, W) for c in cams]
    rng = np.random.default_rng(3)
    raws = _images(rng, 2, H, W)
    dev = _run(cam.rectifier, raws, [0, 1], maps)
    first = cam.UndistortImage(*raws)
    second = cam.UndistortImage(raws[0], raws[1].copy())
    for k in (0, 1):
        assert first[k].tobytes() == dev[k].tobytes() == second[k].tobytes()
    # rows of a wider buffer: the strided host path
    wide = rng.integers(0, 256, (2, H, W + 11), dtype=np.uint8)
    got = cam.UndistortImage(wide[0, :, 3:3 + W], wide[1, :, 3:3 + W])
    assert got[0].tobytes() == RR.remap(wide[0, :, 3:3 + W], *maps[0]).tobytes()
    assert got[1].tobytes() == RR.remap(wide[1, :, 3:3 + W], *maps[1]).tobytes()
    # refusals: nothing is launched
    lib, h = capi.load(), cam.rectifier._h
    buf = capi.DeviceBuffer(8 * H * W)
    idx = (C.c_int * 4)(0, 1, 0, 1)
    px = H * W

    def rc(batch, src, dst, stride=W, pitch=px):
        return lib.rspl_rect_enqueue_device(h, batch, src, stride, pitch, idx, dst, stride, pitch, None)

    assert rc(2, buf.ptr, buf.offset(2 * px)) == 0
    capi.synchronize()
    assert rc(2, buf.ptr, buf.offset(2 * px - 1)) == -1 and b"overlap" in lib.rspl_last_error()
    assert rc(2, buf.offset(px), buf.ptr) == -1 and rc(1, buf.ptr, buf.ptr) == -1
    assert rc(3, buf.ptr, buf.offset(4 * px)) == -1 and b"max_batch" in lib.rspl_last_error()
    assert rc(2, buf.ptr, buf.offset(4 * px), stride=W - 1) == -1
    assert rc(2, buf.ptr, buf.offset(4 * px), pitch=px - 1) == -1
    idx[1] = 2
    assert rc(2, buf.ptr, buf.offset(2 * px)) == -1
    with pytest.raises(ValueError):
        cam.UndistortImage(raws[0], raws[1][:-1])


def test_chain_into_superpoint_on_one_stream(weight_blobs, golden):
    """rspl_rect_enqueue_device and rspl_sp_infer_device queued on one stream with nothing between them: the
    rectified bytes are the restatement's, so SuperPoint's records and counts must be too."""
    H, W, cap = 64, 96, 32
    raw = np.ascontiguousarray(golden("sp_small")["image"], np.uint8)
    assert raw.shape == (H, W)
    raws = [raw, np.ascontiguousarray(np.roll(raw, 5, axis=1))]
    rect, cams = _rectifier(W, H, 0, max_batch=2, f=60)
    maps = [ref_maps(c, 0, H, W) for c in cams]
    sp = pkg.SuperPoint(pkg.SuperPointConfig(max_keypoints=cap, keypoint_threshold=0.004, remove_borders=4,
                                             weights=weight_blobs[0], max_height=H, max_width=W, max_batch=2))
    assert sp.build(), sp.error

    def superpoint(d_images, s):
        d_feat, d_cnt = capi.DeviceBuffer(2 * 259 * cap * 8), capi.DeviceBuffer(8)
        d_feat.zero(s.handle)
        sp.infer_device(d_images.ptr, 2, H, W, W, H * W, d_feat.ptr, cap, d_cnt.ptr, s.handle)
        cnt = d_cnt.download((2,), np.int32, stream=s.handle)
        return d_feat.download((2, cap, 259), np.float64, stream=s.handle), cnt

    s = capi.Stream()
    d_raw, d_rect = capi.DeviceBuffer(2 * H * W), capi.DeviceBuffer(2 * H * W)
    d_raw.upload(np.stack(raws))
    d_rect.zero(s.handle)
    rect.enqueue_device(d_raw, W, H * W, [0, 1], d_rect, W, H * W, s)
    feat, cnt = superpoint(d_rect, s)

    d_ref = capi.DeviceBuffer(2 * H * W)
    d_ref.upload(np.stack([RR.remap(im, *maps[c]) for c, im in enumerate(raws)]))
    ref_feat, ref_cnt = superpoint(d_ref, s)
    assert cnt.tobytes() == ref_cnt.tobytes() and cnt.min() > 0, (cnt, ref_cnt)
    assert feat.tobytes() == ref_feat.tobytes()


def test_create_destroy_cycle():
    """20 rectifiers of a small size created and destroyed (device arena, pinned slot, stream), then one more:
    its host pair equals the first handle's bit for bit."""
    from helpers import assert_same, cycle_handle
    W, H = 16, 8
    left, right = _images(np.random.default_rng(3), 2, H, W)
    first, last = cycle_handle(lambda: _rectifier(W, H, max_batch=1)[0], lambda r: r.pair(left, right))
    assert_same(first, last)
