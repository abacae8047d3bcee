"""Line front end after the detector, CPU part.

librspl's LineDetector post-processing (rspl_line_extract, host C++: csrc/line_merge.cpp) against the
oracle's restatement (oracle/lines_ref.py) of LineDetector::LineExtractor / MergeLines /
MergeTwoLines / FilterShortLines (src/line_processor.cc:11-161, 460-665): bit-exact lines on
synthetic FLD-like fragment sets.  The oracle's assignment / matching restatements are checked on
hand-made cases here; the GPU kernels against them in tests/test_gpu_lines.py.
Parity unpinned at the reference C++ (needs OpenCV contrib + Eigen: unbuildable here; its tests
hold no line vectors).
"""
import math

import numpy as np
import pytest

from conftest import pkg
import lines_ref as LR
from rspl_slam_amd import synthetic as SY


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_line_extract_matches_oracle(seed):
    sc = SY.line_scene(n_lines=70, seed=seed)
    for segs in (sc["seg_left"], sc["seg_right"]):
        got = pkg.lines.LineExtractor(segs)
        ref = LR.line_extractor(segs)
        assert got.shape == ref.shape and len(got) > 10
        np.testing.assert_array_equal(got, ref)
        # the merge joins fragments: fewer lines than fragments, all longer than 60 px
        assert len(got) < len(segs)
        assert (np.hypot(got[:, 2] - got[:, 0], got[:, 3] - got[:, 1]) > 60).all()


def test_line_extract_without_merge_and_empty():
    segs = np.array([[10, 10, 50, 12], [100, 100, 100, 160]], np.float32)
    got = pkg.lines.LineExtractor(segs, do_merge=False)
    np.testing.assert_array_equal(got, segs.astype(np.float64) * 2)
    assert pkg.lines.LineExtractor(np.zeros((0, 4), np.float32)).shape == (0, 4)


def test_line_extract_edge_cases():
    # vertical (dx == 0), horizontal, near +-pi/2 pairs that wrap the angle difference, and
    # collinear fragments with gaps below / above the endpoint thresholds
    segs = np.array([[100, 20, 100, 80], [100.5, 82, 100.3, 150],          # vertical, merges
                     [20, 200, 90, 200], [96, 200.4, 160, 200.2],           # horizontal, 6 px gap (< 15)
                     [300, 200, 360, 200], [400, 200, 460, 200],            # 40 px gap: kept apart in pass 1
                     [200, 10, 200.8, 70], [201.1, 72, 200.2, 140],        # angles near +pi/2 and -pi/2
                     [50, 300, 52, 300]], np.float32)                        # too short: filtered
    got = pkg.lines.LineExtractor(segs)
    ref = LR.line_extractor(segs)
    np.testing.assert_array_equal(got, ref)
    # with capacity too small the call reports the count
    lib = pkg.lines._declare(pkg.capi.load())
    import ctypes as C
    n = C.c_int()
    rc = lib.rspl_line_extract(segs.ctypes.data_as(C.POINTER(C.c_float)), len(segs), 1, None, 0, C.byref(n))
    assert rc == -4 and n.value == len(ref)


def test_merge_two_lines_known_answer():
    # two collinear horizontal pieces merge into their hull
    m = LR.merge_two_lines(np.array([0, 0, 10, 0], np.float32), np.array([12, 0, 30, 0], np.float32))
    np.testing.assert_allclose(m, [0, 0, 30, 0], atol=1e-5)


def test_oracle_assignment_and_matching_known_answers():
    lines = np.array([[0.0, 0.0, 100.0, 0.0], [50.0, -50.0, 50.0, 50.0]])
    xy = np.array([[10, 1], [50, 0], [120, 0], [101, 2], [50, 40], [70, 10], [-2.5, 0.5]], np.float64)
    rel = LR.assign_points_to_lines(lines, xy)
    # point 2 is beyond the box (x > 103); point 3 is within 3 px of the endpoint; point 6 too
    assert sorted(rel[0]) == [0, 1, 3, 6]
    assert sorted(rel[1]) == [1, 4]
    assert rel[0][0] == pytest.approx(1.0) and rel[1][4] == 0.0
    # matching: line 0 of image 0 shares 3 matched points with line 1 of image 1
    rel1 = [{5: 0.0}, {0: 0.0, 1: 0.0, 3: 0.0}]
    m = np.array([[0, 0], [1, 1], [3, 3], [4, 5]])
    out = LR.match_lines(rel, rel1, m, len(xy), 6)
    # v = 3 shared points, score 9 / min(4, 3) = 3 >= 0.8; line 1 (points 1, 4) shares 1: unmatched
    assert out == [1, -1]
    assert LR.match_lines(rel, rel1, m, 0, 6) == [-1, -1]


def test_oracle_stereo_quirk():
    # frame.cc:190 tests line_matches[i] > 0: a match to right line 0 is invalid
    lr, valid = LR.right_lines(np.arange(8.0).reshape(2, 4), [0, 1, -1], 3)
    assert valid.tolist() == [False, True, False]
    np.testing.assert_array_equal(lr[1], [4, 5, 6, 7])


def test_line_scene_is_reproducible():
    a, b = SY.line_scene(seed=5), SY.line_scene(seed=5)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert a["feat_left"].shape[1] == 259 and math.isfinite(a["seg_left"].sum())


# --- the detector restatement (oracle/fld_ref.py: cv::resize + cv::Canny + FastLineDetector) ---
import fld_ref as FR  # noqa: E402


def test_fld_resize_and_sobel_known_answers():
    img = np.arange(16, dtype=np.uint8).reshape(4, 4) * 9
    half = FR.resize_half(img)
    a = img.astype(int)
    ref = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) // 4
    np.testing.assert_array_equal(half, ref)
    ramp = np.tile(np.arange(8, dtype=np.uint8) * 10, (6, 1))  # horizontal ramp: dx = 4 * 10 * 2, dy = 0
    dx, dy = FR.sobel3(ramp)
    assert (dx[:, 1:-1] == 80).all() and (dy == 0).all()
    assert (dx[:, 0] == 40).all() and (dx[:, -1] == 40).all()  # replicated border: one-sided difference 10, x4


def test_fld_canny_step_edge():
    img = np.zeros((40, 40), np.uint8)
    img[:, 20:] = 200                        # vertical step edge between columns 19 and 20
    e = FR.canny(img, 200, 250)
    cols = np.nonzero(e.any(0))[0]
    assert set(cols) <= {19, 20} and e[5:35].any(1).all()  # one thin edge column, every row


def test_fld_oracle_finds_the_ridges():
    """The restated detector + LineExtractor merges recover the synthetic RCF-like ridges: every
    ridge longer than 100 px has a merged line within 3 degrees and 3 px of it (the restatement is
    unpinned; this checks it is a line detector)."""
    img, gt = SY.edge_map(seed=4)
    lines = LR.line_extractor(FR.line_detect(img))
    assert len(lines) > 10
    hit = 0
    long_gt = [g for g in gt if math.hypot(g[2] - g[0], g[3] - g[1]) > 100]
    for g in long_gt:
        ga = math.atan2(g[3] - g[1], g[2] - g[0]) % math.pi
        mid = ((g[0] + g[2]) / 2, (g[1] + g[3]) / 2)
        for l in lines:
            la = math.atan2(l[3] - l[1], l[2] - l[0]) % math.pi
            d = abs(ga - la)
            d = min(d, math.pi - d)
            n = np.array([-(l[3] - l[1]), l[2] - l[0]]) / math.hypot(l[2] - l[0], l[3] - l[1])
            if d < math.radians(3) and abs(n @ (np.array(mid) - l[:2])) < 3:
                hit += 1
                break
    assert hit >= 0.8 * len(long_gt), (hit, len(long_gt))


@pytest.mark.parametrize("seed", [0, 1, 2, 6])
def test_line_extract_on_detector_segments(seed):
    """The merge passes on real detector output (restated FLD on RCF-like edge maps): the two edges
    of a ridge give equal-angle segments, i.e. sort ties -- kept stable on both sides"""
    img, _ = SY.edge_map(seed=seed)
    segs = FR.line_detect(img)
    np.testing.assert_array_equal(pkg.lines.LineExtractor(segs), LR.line_extractor(segs))
