"""The line detector on the device (rspl_lines_detect_device, csrc/fld_kernels.hip), stage by stage and whole.

Hysteresis against fld_ref.hysteresis (exact), chains against the Python raster walk (exact: seeds, points,
order), the detector against the host path rspl_lines_detect: same count and order, every float within one
float32 ulp of the host's (the device's fp64 atan2 / cos / sin are not glibc's; equality is expected and the
number of unequal floats is printed as ``FLD_DEVICE_PARITY``), then batches, capacities, the asynchronous job
and the chain behind the RCF network on one stream."""
import functools
import json

import numpy as np
import pytest

import fld_parallel_ref as PR
import fld_ref as FR
import lines_ref as LR
from conftest import pkg
from rcf_cases import rcf_blob
from rspl_slam_amd import capi
from rspl_slam_amd import lines as L
from rspl_slam_amd import synthetic as SY

pytestmark = pytest.mark.gpu

FILL = 0x7B
CAP = 1024


@functools.lru_cache(maxsize=None)
def _det(th1=200.0, th2=250.0):
    return L.LineDetector(canny_th1=th1, canny_th2=th2)


@functools.lru_cache(maxsize=None)
def _image(kind, h, w, seed):
    if kind == "edge8":
        return SY.edge_map(h, w, n_lines=8, seed=seed)[0]
    if kind == "edge":
        return SY.edge_map(h, w, seed=seed)[0]
    return SY.textured_image(h, w, seed=seed)


@functools.lru_cache(maxsize=None)
def _host(kind, h, w, seed, th1=200.0, th2=250.0):
    """the host path's segments (rspl_lines_detect), computed once per image"""
    out = _det(th1, th2).detect(_image(kind, h, w, seed))
    out.setflags(write=False)
    return out


def _run_device(det, images, capacity=CAP, pad=False, stream=None):
    """one rspl_lines_detect_device call; returns (counts, [segments written per image]) and checks that every
    byte outside the outputs keeps its fill"""
    B = len(images)
    H, W = images[0].shape
    stride = W + 12 if pad else W
    pitch = H * stride + (40 if pad else 0)
    src = np.full((B, pitch), 0x5C, np.uint8)
    for b, im in enumerate(images):
        src[b, :H * stride].reshape(H, stride)[:, :W] = im
    guard = 64
    d_in = capi.DeviceBuffer(src.nbytes).upload(src)
    d_seg = capi.DeviceBuffer(2 * guard + B * capacity * 16)
    d_cnt = capi.DeviceBuffer(2 * guard + 4 * B)
    d_seg.upload(np.full(d_seg.nbytes, FILL, np.uint8))
    d_cnt.upload(np.full(d_cnt.nbytes, FILL, np.uint8))
    s = stream or capi.Stream()
    det.detect_device(d_in, B, H, W, stride, pitch, d_seg.offset(guard), capacity, d_cnt.offset(guard), s)
    raw_seg = d_seg.download(d_seg.nbytes, np.uint8, stream=s.handle)
    raw_cnt = d_cnt.download(d_cnt.nbytes, np.uint8, stream=s.handle)
    assert np.all(raw_seg[:guard] == FILL) and np.all(raw_seg[-guard:] == FILL), "bytes around the segments"
    assert np.all(raw_cnt[:guard] == FILL) and np.all(raw_cnt[-guard:] == FILL), "bytes around the counts"
    counts = raw_cnt[guard:-guard].view(np.int32).copy()
    body = raw_seg[guard:-guard].reshape(B, capacity * 16)
    segs = []
    for b in range(B):
        n = min(int(counts[b]), capacity)
        assert np.all(body[b, n * 16:] == FILL), f"image {b}: written past its {n} segments"
        segs.append(body[b, :n * 16].view(np.float32).reshape(n, 4).copy())
    return counts, segs


def _assert_within_one_ulp(got, ref, what):
    """count and order equal, each float within one float32 ulp of the reference value"""
    assert got.shape == ref.shape, f"{what}: {len(got)} segments, host path {len(ref)}"
    unequal = int(np.count_nonzero(got != ref))
    print("FLD_DEVICE_PARITY " + json.dumps({"case": what, "segments": len(ref), "unequal_floats": unequal}))
    assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64))


# --- 1. hysteresis ---------------------------------------------------------------------------------------
def _random_classes(h, w, seed):
    rng = np.random.default_rng(seed)
    u = rng.random((h, w))
    return np.where(u < 0.02, 2, np.where(u < 0.32, 0, 1)).astype(np.uint8)


def _hysteresis_cases():
    cases = {f"random{h}x{w}": _random_classes(h, w, 3 * h + w) for h, w in ((33, 65), (35, 69), (64, 64))}
    spiral, path = PR.spiral_classes(64)
    assert len(path) >= 1500
    lit = spiral.copy()
    lit[path[-1]] = 2  # the strong pixel at the inner end: the edge set has to travel the whole path
    cases["spiral"] = lit
    cases["spiral_no_strong"] = spiral
    cases["all_candidate"] = np.zeros((40, 70), np.uint8)
    cases["all_strong"] = np.full((40, 70), 2, np.uint8)
    flood = np.zeros((40, 70), np.uint8)
    flood[20, 33] = 2
    cases["all_candidate_one_strong"] = flood
    wb = np.ones((48, 130), np.uint8)  # candidates across the word boundaries 31|32, 63|64, 95|96 and on all borders
    wb[0, :] = wb[-1, :] = wb[:, 0] = wb[:, -1] = 0
    wb[10, :] = 0
    wb[12:40, 31] = wb[12:40:2, 32] = 0
    for k in range(20):  # a diagonal that crosses 63|64
        wb[14 + k, 54 + k] = 0
    wb[0, 129] = 2
    wb[30, 32] = 2
    cases["word_boundaries_and_borders"] = wb
    return cases


HYST = _hysteresis_cases()


@pytest.mark.parametrize("name", sorted(HYST))
def test_hysteresis_equals_the_restatement(name):
    cls = HYST[name]
    ref = PR.zero_corners(FR.hysteresis(cls).copy())
    if name in ("spiral_no_strong", "all_candidate"):
        assert not ref.any()
    if name == "spiral":
        assert np.count_nonzero(FR.hysteresis(cls)) >= 1500
    np.testing.assert_array_equal(_det().debug_hysteresis(cls), ref)


# --- 2. chains -------------------------------------------------------------------------------------------
def _chain_cases():
    cases = {}
    for h, w in ((33, 65), (64, 64)):
        rng = np.random.default_rng(h)
        cases[f"random{h}x{w}"] = np.where(rng.random((h, w)) < 0.3, 255, 0).astype(np.uint8)
    rng = np.random.default_rng(50)  # above the 8-connected percolation threshold: one junction-heavy component
    cases["dense64x64"] = np.where(rng.random((64, 64)) < 0.5, 255, 0).astype(np.uint8)
    ring = np.zeros((40, 70), np.uint8)
    ring[8, 10:60] = ring[30, 10:60] = ring[8:31, 10] = ring[8:31, 59] = 255
    cases["ring"] = ring
    cases["dots_and_bars"] = PR.dots_and_bars()
    wb = np.zeros((20, 100), np.uint8)  # separate components that meet inside the words around 31|32 and 63|64
    wb[3, 20:32] = wb[5, 32:50] = wb[9, 28:31] = wb[9, 33:36] = 255
    wb[12:18, 63] = wb[12:18, 65] = 255
    cases["word_boundaries"] = wb
    last = np.zeros((24, 45), np.uint8)
    last[-1, :] = last[:, -1] = last[0, 3:40] = last[2:20, 0] = 255
    cases["last_row_and_column"] = last
    cases["empty"] = np.zeros((16, 40), np.uint8)
    return cases


CHAINS = _chain_cases()


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_chains_equal_the_python_walk(name):
    e = CHAINS[name]
    ref = PR.walk_sequential(e)
    got = _det().debug_chains(e)
    if name == "dots_and_bars":
        assert len(PR.components(e)) == 200  # more components than the walk has lanes
    assert [s for s, _ in got] == [s for s, _ in ref]
    for (seed, pts), (_, want) in zip(got, ref):
        assert [tuple(p) for p in pts.tolist()] == want, f"chain seeded at {seed}"
    assert _det().detect_status() == 0


# --- 3. the detector -------------------------------------------------------------------------------------
DETECT = [("edge", 480, 752, 0, 200.0), ("edge", 480, 752, 5, 200.0), ("edge8", 64, 96, 4, 200.0),
          ("edge8", 96, 128, 3, 200.0), ("edge8", 70, 138, 2, 200.0), ("textured", 300, 420, 7, 50.0)]


@pytest.mark.parametrize("kind,h,w,seed,th", DETECT, ids=lambda v: str(v))
def test_detector_equals_the_host_path(kind, h, w, seed, th):
    th2 = 250.0 if th == 200.0 else th
    ref = _host(kind, h, w, seed, th, th2)
    assert len(ref) >= 7
    det = _det(th, th2)
    counts, segs = _run_device(det, [_image(kind, h, w, seed)])
    assert counts[0] == len(ref) and det.detect_status() == 0
    _assert_within_one_ulp(segs[0], ref, f"{kind}-{h}x{w}-{seed}")
    st = det.debug_fld_stats(0)
    assert st["segments"] == len(ref) and st["status"] == 0 and st["edge_pixels"] > 0 and st["components"] > 0


def test_batch_of_two_with_padding_equals_the_single_images():
    a, b = _image("edge8", 96, 128, 3), _image("edge8", 96, 128, 7)
    counts, segs = _run_device(_det(), [a, b], pad=True)
    for im, n, got, what in ((a, counts[0], segs[0], "batch0"), (b, counts[1], segs[1], "batch1")):
        (n1,), (single,) = _run_device(_det(), [im])
        assert n == n1 > 0
        np.testing.assert_array_equal(got, single)
        _assert_within_one_ulp(got, _det().detect(im), what)
    assert not np.array_equal(segs[0], segs[1][:len(segs[0])]) and _det().detect_status() == 0


def test_capacity_four_reports_the_full_count_and_writes_the_first_four():
    ref = _host("edge", 480, 752, 0)
    assert len(ref) == 147
    counts, segs = _run_device(_det(), [_image("edge", 480, 752, 0)], capacity=4)
    assert counts[0] == 147 and len(segs[0]) == 4
    assert _det().detect_status() == L.FLD_ST_SEGMENTS
    _assert_within_one_ulp(segs[0], ref[:4], "capacity4")


def test_blank_image_has_no_segments():
    counts, segs = _run_device(_det(), [np.zeros((64, 64), np.uint8), np.full((64, 64), 255, np.uint8)])
    assert list(counts) == [0, 0] and _det().detect_status() == 0


def test_submit_device_on_two_handles_in_flight():
    """the asynchronous job with a device image: its lines are the reference LineExtractor's of the segments
    detect_device returns for that image; wait and wait_device deliver the same"""
    dets = [L.LineDetector(), L.LineDetector()]
    imgs = [_image("edge", 480, 752, 0), _image("edge", 480, 752, 5)]
    H, W = imgs[0].shape
    st = capi.Stream()
    bufs = [capi.DeviceBuffer(H * W).upload(im, st.handle) for im in imgs]
    want = []
    for im, kind in zip(imgs, (0, 5)):
        counts, segs = _run_device(_det(), [im])
        assert counts[0] == len(_host("edge", 480, 752, kind))
        want.append(LR.line_extractor(segs[0]))
    for d, b in zip(dets, bufs):
        d.submit_device(b, H, W, W, st)
    for d, ref in zip(dets, want):
        got, ms = d.wait()
        assert ms > 0 and len(ref) > 5
        np.testing.assert_array_equal(got, ref)
    out = [capi.DeviceBuffer(512 * 4 * 8) for _ in dets]
    for d, b in zip(dets, bufs):
        d.submit_device(b, H, W, W, st)
    with pytest.raises(capi.RsplError):
        dets[0].submit_device(bufs[0], H, W, W, st)  # one job in flight per handle
    for d, o, ref in zip(dets, out, want):
        n, _ = d.wait_device(o.ptr, 512, st.handle)
        assert n == len(ref)
        np.testing.assert_array_equal(o.download((n, 4), np.float64, st.handle), ref)
    with pytest.raises(capi.RsplError):
        dets[0].wait()


@pytest.mark.parametrize("h,w", [(16, 16), (64, 80)])
def test_chain_behind_the_rcf_network_on_one_stream(h, w):
    """RCF.infer_device and detect_device queued on one stream with no host wait between them equal the host
    detector on the downloaded edge image"""
    rcf = pkg.RCF(rcf_blob(), max_height=64, max_width=96, max_batch=1)
    det = _det(50.0, 50.0)
    img = SY.textured_image(h, w, seed=3)
    s = capi.Stream()
    d_img, d_edge = capi.DeviceBuffer(h * w).upload(img, s.handle), capi.DeviceBuffer(h * w)
    d_seg, d_cnt = capi.DeviceBuffer(CAP * 16), capi.DeviceBuffer(4)
    rcf.infer_device(d_img, 1, h, w, w, h * w, d_edge, w, h * w, s)
    det.detect_device(d_edge, 1, h, w, w, h * w, d_seg, CAP, d_cnt, s)
    n = int(d_cnt.download(1, np.int32, stream=s.handle)[0])
    edges = d_edge.download((h, w), np.uint8, stream=s.handle)
    ref = det.detect(edges)
    assert n == len(ref)
    _assert_within_one_ulp(d_seg.download((n, 4), np.float32, stream=s.handle), ref, f"rcf-{h}x{w}")
