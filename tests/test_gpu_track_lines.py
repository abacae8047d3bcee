"""The tracking step's line side and keyframe decision on the device (rspl_track_enqueue_ext: the line half of
MapBuilder::TrackFrame, src/map_builder.cc:450-455 / 490-501, and MapBuilder::AddKeyframe, :616-636) against
oracle/lines_ref.py's AssignPointsToLines / MatchLines and tests/track_lines_ref.py's id copy and decision.
Index work and the distances (the reference's doubles through a float) are compared exactly; the decision's
two doubles within 1e-12 of the restatement on the device's own fetched pose.  Parity of the line row is
unpinned at the reference C++ (Eigen / OpenCV absent)."""
import numpy as np
import pytest

import track_lines_cases as TC
import track_lines_ref as TLR
import track_ref as TR
from conftest import pkg
from rspl_slam_amd import capi
from rspl_slam_amd import lines as LN

pytestmark = pytest.mark.gpu

K, ML, CAP = 512, 64, 4096


@pytest.fixture(scope="module")
def tr():
    t = pkg.Tracker(max_batch=3, max_keypoints=K)
    t.enable_lines(max_lines=ML, max_pairs=CAP)
    return t


@pytest.fixture(scope="module")
def plain():
    return pkg.Tracker(max_batch=3, max_keypoints=K)


def _dev(a):
    a = np.ascontiguousarray(a)
    b = capi.DeviceBuffer(max(a.nbytes, 8))
    if a.nbytes:
        b.upload(a)
    return b


def _frames(t, cases, lines=True, set_lines=True, **kw):
    """keyframe b in slot b; returns the frame dicts (they hold the device buffers until the fetch)"""
    frames = []
    for b, c in enumerate(cases):
        t.set_keyframe(b, c["points"], c["state"], c["track_id"])
        d = dict(slot=b, d_features=_dev(c["features"]), d_n1=_dev(np.array([len(c["idx1"])], np.int32)),
                 d_idx0=_dev(c["idx0"]), d_idx1=_dev(c["idx1"]), cam=c["cam"], last_Twc=c["last_Twc"])
        if lines:
            if set_lines:
                kf = (_dev(c["kf_lines"]), _dev(c["kf_features"]), _dev(np.array([len(c["idx0"])], np.int32)))
                t.set_keyframe_lines(b, len(c["kf_lines"]), *kf, c["kf_line_track_id"], c["kf_line_slot"])
                d["_kf"] = kf
            d.update(d_lines=_dev(c["lines"]), n_lines=len(c["lines"]), frame_id=c["frame_id"],
                     keyframe=dict(Twc=c["kf_Twc"], frame_id=c["kf_frame_id"]))
        d.update(kw)
        frames.append(d)
    return frames


def _run(t, cases, **kw):
    frames = _frames(t, cases, **kw)
    t.enqueue(frames)
    res = t.fetch()
    return res, [t.debug_lines(b) for b in range(len(cases))]


def _ref(c, max_pairs=CAP):
    n0, n1 = len(c["idx0"]), len(c["idx1"])
    return TLR.track_lines(c["kf_lines"], c["kf_features"][:, 1:3], c["lines"], c["features"][:, 1:3],
                           TR.matches(c["idx0"], c["idx1"], n0), n0, n1, c["kf_line_track_id"], c["kf_line_slot"],
                           max_pairs=max_pairs)


def _csr_equal(got, rel):
    off, idx, dist = LN.relation_to_csr(rel)
    np.testing.assert_array_equal(got[0], off)
    np.testing.assert_array_equal(got[1], idx)
    np.testing.assert_array_equal(got[2], dist)  # bit for bit


def _check_lines(r, d, ref, csr=True):
    for k in ("line_match_kf", "line_track_id", "line_slot"):
        np.testing.assert_array_equal(r[k], ref[k], err_msg=k)
    assert (r["n_lines"], r["n_line_matches"], r["n_line_tracks"], r["overflow"]) == \
        (len(ref["line_match_kf"]), ref["n_line_matches"], ref["n_line_tracks"], ref["overflow"])
    if csr:
        _csr_equal(d["frame"], ref["rel"])
        _csr_equal(d["keyframe"], ref["rel_kf"])


def _check_decision(c, r, **kw):
    ref = TLR.decision_q(r["pose_q"], r["pose_p"], r["n_inliers"], c["kf_Twc"], c["kf_frame_id"], c["frame_id"], **kw)
    assert (r["tracked_well"], r["add_keyframe"], r["passed_frames"]) == \
        (ref["tracked_well"], ref["add_keyframe"], ref["passed_frames"])
    assert abs(r["delta_angle"] - ref["delta_angle"]) < 1e-12
    assert abs(r["delta_distance"] - ref["delta_distance"]) < 1e-12
    return ref


# the seams of the wave-per-line loop (16 waves) and of the 64-keypoints-per-ballot loop
@pytest.mark.parametrize("n_pts", [0, 1, 63, 64, 65])
def test_seams(tr, n_pts):
    cases = [TC.line_case(nl, n_pts) for nl in (0, 1, 15, 16, 17)]
    for i in range(0, len(cases), 3):
        part = cases[i:i + 3]
        res, dbg = _run(tr, part)
        for c, r, d in zip(part, res, dbg):
            ref = _ref(c)
            _check_lines(r, d, ref)
            _check_decision(c, r)
            if len(c["lines"]) and n_pts >= 63:  # both sides non-empty: an all -1 output cannot pass
                assert ref["n_line_matches"] > 0


def test_typical_frame(tr):
    c = TC.line_case(60, 400)
    (r,), (d,) = _run(tr, [c])
    ref = _ref(c)
    assert ref["n_line_matches"] > 40 and 0 < ref["n_line_tracks"] < ref["n_line_matches"]
    assert (ref["line_track_id"] == 0).any()  # id 0 is propagated, unlike the points' `> 0`
    assert ((ref["line_track_id"] >= 0) & (ref["line_slot"] == -1)).any()  # a slot of -1 is copied
    _check_lines(r, d, ref)
    assert r["pose_set"] and r["tracked_well"]
    _check_decision(c, r)


def test_max_lines_handle():
    t = pkg.Tracker(max_batch=1, max_keypoints=K)
    t.enable_lines(max_lines=32, max_pairs=CAP)
    c = TC.line_case(32, 300)
    (r,), (d,) = _run(t, [c])
    ref = _ref(c)
    assert ref["n_line_matches"] > 10
    _check_lines(r, d, ref)
    with pytest.raises(capi.RsplError):
        t.enqueue(_frames(t, [c], n_lines=33))  # checked before the first launch
    t.enqueue(_frames(t, [c]))                  # ... so the handle is still usable
    _check_lines(t.fetch()[0], None, ref, csr=False)


def test_hand_built_matrices(tr):
    c = TC.hand_case()
    (r,), (d,) = _run(tr, [c])
    for k, v in c["expect"].items():
        assert list(r[k]) == v, k
    _check_lines(r, d, _ref(c))
    assert (r["n_line_matches"], r["n_line_tracks"]) == (3, 2)


def test_batch_of_three(tr):
    """different slots, keyframes and line counts (one of them 0): the per-frame strides"""
    cases = [TC.line_case(40, 300, seed=3), TC.line_case(0, 120, seed=4, n_kf_lines=9), TC.line_case(23, 210, seed=5)]
    res, dbg = _run(tr, cases)
    for c, r, d in zip(cases, res, dbg):
        ref = _ref(c)
        _check_lines(r, d, ref)
        _check_decision(c, r)
    assert res[0]["n_line_matches"] > 0 and res[2]["n_line_matches"] > 0 and res[1]["n_lines"] == 0
    # the device arrays a device consumer reads
    for b, r in enumerate(res):
        p = tr.frame_lines(b)
        for k in ("line_track_id", "line_slot"):
            got = np.zeros(ML, np.int32)
            capi.check(capi.load().rspl_memcpy_d2h(got.ctypes.data, p[k], got.nbytes, None), "rspl_memcpy_d2h")
            np.testing.assert_array_equal(got[:r["n_lines"]], r[k])


def test_unchanged_point_results(tr, plain):
    cases = [TC.line_case(40, 300, seed=3), TC.line_case(12, 90, seed=6)]
    ext, _ = _run(tr, cases)
    tr.enqueue(_frames(tr, cases, lines=False))  # the plain path on the handle with lines enabled
    same = tr.fetch()
    plain.enqueue(_frames(plain, cases, lines=False))
    base = plain.fetch()
    for e, s, b in zip(ext, same, base):
        assert "n_lines" in e and "n_lines" not in s and "n_lines" not in b
        for k, v in b.items():
            np.testing.assert_array_equal(e[k], v, err_msg=k)
            np.testing.assert_array_equal(s[k], v, err_msg=k)


@pytest.mark.parametrize("side", ["keyframe", "frame"])
def test_overflow(tr, side):
    c = TC.line_case(60, 400)
    full = _ref(c)
    assert min(full["pairs"]) > 128 and max(full["pairs"]) <= CAP
    if side == "keyframe":  # only the keyframe's assignment does not fit: fewer lines in the frame
        c = dict(c, lines=c["lines"][:12])
        assert _ref(c)["pairs"][1] <= 128
    else:
        c = dict(c, kf_lines=c["kf_lines"][:12], kf_line_track_id=c["kf_line_track_id"][:12],
                 kf_line_slot=c["kf_line_slot"][:12])
        assert _ref(c)["pairs"][0] <= 128
    (ok,), _ = _run(tr, [c])
    assert ok["n_line_matches"] > 0 and not ok["overflow"]
    small = pkg.Tracker(max_batch=1, max_keypoints=K)
    small.enable_lines(max_lines=ML, max_pairs=128)
    (r,), _ = _run(small, [c])
    ref = _ref(c, max_pairs=128)
    assert ref["overflow"] and r["overflow"] and r["n_line_matches"] == 0 and r["n_lines"] == len(c["lines"])
    _check_lines(r, None, ref, csr=False)
    assert (r["line_match_kf"] == -1).all() and (r["line_track_id"] == -1).all() and (r["line_slot"] == -1).all()
    for k in ("pose_q", "pose_p", "pose_set", "n_inliers", "match_kf", "track_id", "kept", "chi2", "add_keyframe",
              "delta_angle", "delta_distance"):
        np.testing.assert_array_equal(r[k], ok[k], err_msg=k)  # the point results and the decision are unaffected


def test_decision_bits_from_the_inputs(tr):
    c = TC.line_case(20, 300)
    (r0,), _ = _run(tr, [c])
    assert r0["pose_set"] and r0["n_inliers"] > 10
    n, ang, dist = r0["n_inliers"], r0["delta_angle"], r0["delta_distance"]
    assert ang > 1e-3 and dist > 1e-3
    none = dict(max_num_match=n, max_angle=ang + 1e-6, max_distance=dist + 1e-6, max_num_passed_frame=7)
    runs = [(none, 0),
            (dict(none, max_num_match=n + 1), TLR.KF_NOT_ENOUGH_MATCH),
            (dict(none, max_angle=ang - 1e-6), TLR.KF_LARGE_DELTA_ANGLE),
            (dict(none, max_distance=dist - 1e-6), TLR.KF_LARGE_DISTANCE),
            (dict(none, max_num_passed_frame=6), TLR.KF_ENOUGH_PASSED_FRAME),
            (dict(max_num_match=n + 1, max_angle=ang - 1e-6, max_distance=dist - 1e-6, max_num_passed_frame=6), 15)]
    for kw, bits in runs:
        (r,), _ = _run(tr, [c], **kw)
        assert r["add_keyframe"] == bits, kw
        assert (r["n_inliers"], r["passed_frames"]) == (n, 7)
        _check_decision(c, r, **kw)
    # tracked_well: n_inliers >= min_num_match (:240), while pose_set is n_inliers > min_num_match (:586)
    (r,), _ = _run(tr, [c], min_num_match=n)
    assert r["n_inliers"] == n and r["tracked_well"] and not r["pose_set"]
    (r,), _ = _run(tr, [c], min_num_match=n + 1)
    assert not r["tracked_well"]


def test_decision_on_the_last_pose(tr):
    """pose_set == 0: the frame keeps the last pose (:217), and the decision is made on it"""
    c = TC.line_case(20, 300)
    (r,), _ = _run(tr, [c], min_num_match=1000)
    assert not r["pose_set"] and not r["tracked_well"]
    last = c["last_Twc"]
    ref = TLR.decision(last[:3, :3], last[:3, 3], r["n_inliers"], c["kf_Twc"], c["kf_frame_id"], c["frame_id"],
                       min_num_match=1000)
    assert r["add_keyframe"] == ref["add_keyframe"]
    np.testing.assert_array_equal(r["pose_p"], last[:3, 3])
    assert abs(r["delta_angle"] - ref["delta_angle"]) < 1e-12
    assert abs(r["delta_distance"] - ref["delta_distance"]) < 1e-12
    _check_decision(c, r, min_num_match=1000)


def test_slot_without_lines():
    """a slot whose lines were set to none, and one whose lines were never set: empty line results, the
    decision still made"""
    t = pkg.Tracker(max_batch=2, max_keypoints=K)
    t.enable_lines(max_lines=ML, max_pairs=CAP)
    c = TC.line_case(20, 300)
    zero = dict(c, kf_lines=c["kf_lines"][:0], kf_line_track_id=c["kf_line_track_id"][:0],
                kf_line_slot=c["kf_line_slot"][:0])
    frames = _frames(t, [zero, c], set_lines=False)
    t.set_keyframe_lines(0, 0, None, None, None, [], [])  # slot 0: no lines; slot 1: never set
    t.enqueue(frames)
    res = t.fetch()
    for r in res:
        assert (r["n_lines"], r["n_line_matches"], r["n_line_tracks"], r["overflow"]) == (20, 0, 0, False)
        assert (r["line_match_kf"] == -1).all() and (r["line_track_id"] == -1).all() and (r["line_slot"] == -1).all()
        _check_decision(c, r)
    _csr_equal(t.debug_lines(1)["frame"], _ref(c)["rel"])  # the frame's own assignment is still made
    assert list(t.debug_lines(1)["keyframe"][0]) == [0]


def test_argument_checks(tr, plain):
    c = TC.line_case(5, 64)
    with pytest.raises(capi.RsplError):
        plain.enqueue(_frames(plain, [c], set_lines=False))       # lines not enabled
    with pytest.raises(capi.RsplError):
        tr.enqueue(_frames(tr, [c], d_lines=None))                # NULL d_lines with n_lines > 0
    with pytest.raises(capi.RsplError):
        tr.enable_lines(max_lines=ML, max_pairs=CAP)              # once per handle
    big = pkg.Tracker(max_batch=1, max_keypoints=4097)
    with pytest.raises(capi.RsplError):
        big.enable_lines(max_lines=ML, max_pairs=CAP)             # more keypoints than a line workgroup holds
    (r,), (d,) = _run(tr, [c])                                    # the refusals left the handle usable
    _check_lines(r, d, _ref(c))


def test_create_destroy_cycle():
    """20 handles of the smallest capacities with the line side enabled, created and destroyed (both device
    arenas, both pinned arenas, both stagings, stream, events), then one more: its enqueue_ext + fetch and debug
    read-back equal the first handle's bit for bit."""
    from helpers import assert_same, cycle_handle
    c = TC.line_case(4, 8)

    def make():
        t = pkg.Tracker(max_batch=1, max_keypoints=8)
        t.enable_lines(max_lines=8, max_pairs=64)
        return t

    first, last = cycle_handle(make, lambda t: _run(t, [c]))
    assert first[0][0]["n_lines"] == 4
    assert_same(first, last)
