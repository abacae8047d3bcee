"""CPU-side checks of the tracking step's line side and keyframe decision (rspl_track_enqueue_ext): the
boundary is declared and bound without touching ABI 2, rspl_track_enable_lines judges its configuration
before a device is touched, and the numpy restatement (tests/track_lines_ref.py) does what
map_builder.cc:490-501 and :616-636 do on hand-made cases."""
import ctypes as C
import math
import pathlib
import re

import numpy as np
import pytest

import track_lines_ref as TLR

ROOT = pathlib.Path(__file__).resolve().parents[1]
FUNCS = ("rspl_track_enable_lines", "rspl_track_set_keyframe_lines", "rspl_track_enqueue_ext", "rspl_track_fetch_ext",
         "rspl_track_debug_lines", "rspl_track_frame_lines")


def test_header_declares_track_lines_api():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    for n in FUNCS:
        assert n in names
    for s in ("rspl_track_lines_config", "rspl_track_frame_ext", "rspl_track_ext_result", "rspl_track_debug_lines_out"):
        assert re.search(r"}\s*%s;" % s, hdr), s
    for bit, v in (("NOT_ENOUGH_MATCH", 1), ("LARGE_DELTA_ANGLE", 2), ("LARGE_DISTANCE", 4), ("ENOUGH_PASSED_FRAME", 8)):
        assert re.search(r"#define RSPL_TRACK_KF_%s %d\b" % (bit, v), hdr), bit
    assert "#define RSPL_ABI_VERSION 2" in hdr  # every addition is a new declaration
    assert "stays with rspl_lines_match" not in hdr


def test_capi_binds_track_lines_api():
    from rspl_slam_amd import api, capi
    lib = capi.load()
    for n in FUNCS:
        assert n in capi.EXPORTS and hasattr(lib, n)
    assert len(lib.rspl_track_enqueue_ext.argtypes) == 5 and len(lib.rspl_track_set_keyframe_lines.argtypes) == 9
    assert [f[0] for f in capi.TrackLinesConfig._fields_] == ["max_lines", "max_pairs"]
    assert [f[0] for f in capi.TrackFrameExt._fields_] == ["d_lines", "n_lines", "kf_Twc", "kf_frame_id", "frame_id",
                                                            "max_num_match", "max_angle", "max_distance",
                                                            "max_num_passed_frame"]
    # the C layouts (LP64): pointer, int, 16 doubles, 3 ints (+ pad), 2 doubles, int (+ pad)
    assert C.sizeof(capi.TrackFrameExt) == 8 + 8 + 128 + 16 + 16 + 8
    assert C.sizeof(capi.TrackExtResult) == 24 + 16 + 8 + 24
    assert (api.TRACK_KF_NOT_ENOUGH_MATCH, api.TRACK_KF_LARGE_DELTA_ANGLE, api.TRACK_KF_LARGE_DISTANCE,
            api.TRACK_KF_ENOUGH_PASSED_FRAME) == (1, 2, 4, 8)
    for k in ("enable_lines", "set_keyframe_lines", "frame_lines", "debug_lines"):
        assert callable(getattr(api.Tracker, k))


@pytest.mark.parametrize("ml,mp,what", [(0, 1024, "max_lines"), (1025, 1024, "max_lines"), (64, 0, "max_pairs")])
def test_enable_lines_rejects_bad_config_before_the_device(ml, mp, what):
    """The configuration is judged first, whatever the handle: no tracker (and so no device) is needed."""
    from rspl_slam_amd import capi
    lib = capi.load()
    cfg = capi.TrackLinesConfig(ml, mp)
    assert lib.rspl_track_enable_lines(None, C.byref(cfg)) == -1  # RSPL_E_ARG, not a device error
    assert what in lib.rspl_last_error().decode()
    ok = capi.TrackLinesConfig(1024, 1)  # the bounds themselves pass: the complaint is the missing handle
    assert lib.rspl_track_enable_lines(None, C.byref(ok)) == -1
    assert "handle" in lib.rspl_last_error().decode()


def test_id_copy_hand_case():
    # keyframe line  line_matches  track id  map line
    #      0              2           0        -1      matched, id 0: propagated (>= 0), the slot -1 copied
    #      1              0          -1        31      matched, no track: nothing propagated
    #      2             -1           5        32      unmatched
    #      3              3           6        33      matched
    mk, tid, slot = TLR.id_copy([2, 0, -1, 3], [0, -1, 5, 6], [-1, 31, 32, 33], 5)
    assert list(mk) == [1, -1, 0, 3, -1]
    assert list(tid) == [-1, -1, 0, 6, -1]
    assert list(slot) == [-1, -1, -1, 33, -1]
    assert [list(a) for a in TLR.id_copy([], [], [], 2)] == [[-1, -1]] * 3


def _rot(axis, a):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx


def _kf(R=np.eye(3), t=(0, 0, 0)):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def test_decision_bits_one_at_a_time():
    Rk, tk = _rot([1, 2, 3], 0.3), np.array([1.0, -2.0, 0.5])
    base = dict(R=Rk @ _rot([0, 1, 0], 0.1), t=tk + [0.1, 0, 0], n_inliers=100, kf_Twc=_kf(Rk, tk), kf_frame_id=10,
                frame_id=20)
    d = TLR.decision(**base)
    assert d["add_keyframe"] == 0 and d["tracked_well"] and d["passed_frames"] == 10
    assert abs(d["delta_angle"] - 0.1) < 1e-12 and abs(d["delta_distance"] - 0.1) < 1e-12
    assert TLR.decision(**dict(base, n_inliers=79))["add_keyframe"] == TLR.KF_NOT_ENOUGH_MATCH
    assert TLR.decision(**dict(base, R=Rk @ _rot([0, 1, 0], 0.6)))["add_keyframe"] == TLR.KF_LARGE_DELTA_ANGLE
    assert TLR.decision(**dict(base, t=tk + [0.3, 0.4, 0.1]))["add_keyframe"] == TLR.KF_LARGE_DISTANCE
    assert TLR.decision(**dict(base, frame_id=311))["add_keyframe"] == TLR.KF_ENOUGH_PASSED_FRAME
    assert TLR.decision(**dict(base, n_inliers=5, frame_id=400))["add_keyframe"] == \
        TLR.KF_NOT_ENOUGH_MATCH | TLR.KF_ENOUGH_PASSED_FRAME
    assert not TLR.decision(**dict(base, n_inliers=9))["tracked_well"]         # num_match >= min_num_match (:240)
    assert TLR.decision(**dict(base, n_inliers=10))["tracked_well"]


def test_decision_comparisons_at_equality():
    base = dict(R=np.eye(3), t=np.zeros(3), kf_Twc=_kf(), kf_frame_id=0)
    assert TLR.decision(n_inliers=80, frame_id=300, **base)["add_keyframe"] == 0    # `<` and `>` (:631, :634)
    assert TLR.decision(n_inliers=79, frame_id=300, **base)["add_keyframe"] == TLR.KF_NOT_ENOUGH_MATCH
    assert TLR.decision(n_inliers=80, frame_id=301, **base)["add_keyframe"] == TLR.KF_ENOUGH_PASSED_FRAME
    for eps, bit in ((-1e-6, 0), (1e-6, TLR.KF_LARGE_DELTA_ANGLE)):
        d = TLR.decision(n_inliers=80, frame_id=1, **dict(base, R=_rot([0, 0, 1], 0.52 + eps)))
        assert d["add_keyframe"] == bit
    for eps, bit in ((-1e-6, 0), (1e-6, TLR.KF_LARGE_DISTANCE)):
        d = TLR.decision(n_inliers=80, frame_id=1, **dict(base, t=[0.0, 0.5 + eps, 0.0]))
        assert d["add_keyframe"] == bit


def test_decision_angle_extremes():
    assert TLR.delta_angle(np.eye(3), np.eye(3)) == 0.0
    Rk = _rot([1, 0, 1], 0.7)
    assert TLR.delta_angle(Rk, Rk) < 1e-15
    for ax in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0]):
        assert abs(TLR.delta_angle(np.eye(3), _rot(ax, math.pi)) - math.pi) < 1e-7   # trace = -1: the branch of R_to_q
    assert abs(TLR.delta_angle(np.eye(3), _rot([0, 0, 1], -3.0)) - 3.0) < 1e-12      # in [0, pi] whatever the sign


def test_angle_agrees_with_arccos_of_the_trace():
    rng = np.random.default_rng(0)
    for _ in range(200):
        a = rng.uniform(0.05, math.pi - 0.05)
        Rk = _rot(rng.normal(size=3), rng.uniform(-3, 3))
        R = Rk @ _rot(rng.normal(size=3), a)
        ref = math.acos((np.trace(Rk.T @ R) - 1) / 2)
        assert abs(TLR.delta_angle(Rk, R) - ref) < 1e-9
        assert abs(ref - a) < 1e-9


def test_q_to_R_round_trip():
    from rspl_slam_amd import synthetic as SY
    R = _rot([1, -2, 0.5], 1.1)
    q = SY.R_to_quat_xyzw(R)
    assert np.abs(TLR.q_to_R(q) - R).max() < 1e-14
    w = TLR.R_to_q(R)
    s = 1.0 if w[0] * q[3] > 0 else -1.0
    assert np.abs(w / np.linalg.norm(w) - s * np.array([q[3], q[0], q[1], q[2]])).max() < 1e-14


def test_line_case_is_not_trivial():
    """the validity of the GPU test's scenes, checked here: their lines do match"""
    import track_lines_cases as TC
    import track_ref as TR
    for nl, npt, want in ((17, 65, None), (60, 400, None), (1, 64, None)):
        c = TC.line_case(nl, npt)
        mk = TR.matches(c["idx0"], c["idx1"], npt)
        r = TLR.track_lines(c["kf_lines"], c["kf_features"][:, 1:3], c["lines"], c["features"][:, 1:3], mk, npt, npt,
                            c["kf_line_track_id"], c["kf_line_slot"])
        assert len(c["lines"]) == nl and r["n_line_matches"] > 0, (nl, npt)
    h = TC.hand_case()
    mk = TR.matches(h["idx0"], h["idx1"], len(h["kf_features"]))
    r = TLR.track_lines(h["kf_lines"], h["kf_features"][:, 1:3], h["lines"], h["features"][:, 1:3], mk,
                        len(h["kf_features"]), len(h["features"]), h["kf_line_track_id"], h["kf_line_slot"])
    for k, v in h["expect"].items():
        assert list(r[k]) == v, k
    assert [len(x) for x in r["rel_kf"]] == [5, 5, 5, 5, 4] and [len(x) for x in r["rel"]] == [5, 5, 6, 5, 4, 4]
