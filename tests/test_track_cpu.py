"""CPU-side checks of the tracking step (rspl_track_*): the boundary is declared and bound, the
Python class rejects bad capacities before a device is touched, and the numpy restatement
(tests/track_ref.py) does what map_builder.cc:448-611 does on a hand-made case."""
import pathlib
import re

import numpy as np
import pytest

import track_ref as TR

ROOT = pathlib.Path(__file__).resolve().parents[1]
FUNCS = ("rspl_track_create", "rspl_track_destroy", "rspl_track_set_keyframe", "rspl_track_enqueue",
         "rspl_track_fetch", "rspl_track_debug_stage")


def test_header_declares_track_api():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    for n in FUNCS:
        assert n in names
    for s in ("rspl_track_config", "rspl_track_frame", "rspl_track_result", "rspl_track_debug"):
        assert re.search(r"}\s*%s;" % s, hdr), s
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct changed


def test_capi_binds_track_api():
    from rspl_slam_amd import capi
    lib = capi.load()
    for n in FUNCS:
        assert n in capi.EXPORTS and hasattr(lib, n)
    assert lib.rspl_track_enqueue.argtypes is not None and len(lib.rspl_track_enqueue.argtypes) == 4
    assert [f[0] for f in capi.TrackConfig._fields_] == ["max_batch", "max_keypoints", "device"]


@pytest.mark.parametrize("kw", [dict(max_batch=0), dict(max_keypoints=0), dict(max_batch=-1, max_keypoints=16)])
def test_tracker_rejects_bad_capacities(kw):
    import rspl_loader
    pkg = rspl_loader.load()
    with pytest.raises(ValueError):
        pkg.Tracker(**kw)


def test_create_rejects_bad_capacities_before_the_device():
    import ctypes as C
    from rspl_slam_amd import capi
    lib = capi.load()
    for mb, mk in ((0, 64), (4, 0)):
        h = C.c_void_p()
        cfg = capi.TrackConfig(mb, mk, 0)
        assert lib.rspl_track_create(C.byref(cfg), C.byref(h)) == -1  # RSPL_E_ARG, not a device error
        assert not h.value


def _hand_case():
    # 6 current keypoints, 5 keyframe keypoints
    #  i  idx1  partner's idx0   state  track id
    #  0   2        0              1       7      match, edge (stereo)
    #  1   0        1              1       0      match, edge; track id 0: dropped by `> 0`
    #  2   1        5              -       -      idx0[1] = 5 != 2: not mutual
    #  3   4        3              2       9      match, map point not Good: never an edge, kept
    #  4  -1                                      unmatched
    #  5   1        5              0       4      match, no map point: never an edge, kept
    feats = np.zeros((6, 259))
    feats[:, 1] = [10.5, 20.25, 30, 40, 50, 60.125]
    feats[:, 2] = [1, 2, 3, 4, 5, 6]
    return dict(points=np.arange(15, dtype=np.float64).reshape(5, 3) + 0.1, state=np.array([1, 0, 1, 1, 2], np.uint8),
                track_id=np.array([0, 4, 7, 3, 9], np.int32), idx0=np.array([1, 5, 0, -1, 3], np.int32),
                idx1=np.array([2, 0, 1, 4, -1, 1], np.int32), features=feats,
                u_right=np.array([5.0, -1, 3, 3, 3, 3]), cam=(400.0, 401.0, 300.0, 200.0, 40.0), last_Twc=np.eye(4))


def test_track_ref_hand_case():
    p = _hand_case()
    g = TR.gather(p)
    assert list(g["match_kf"]) == [2, 0, -1, 4, -1, 1]          # i = 2 is not mutual
    assert list(g["inl"]) == [7, 0, -1, 9, -1, 4]
    assert list(g["corr_kp"]) == [0, 1]                         # ascending i, state 1 only
    assert list(g["edge_kp"]) == [1, 0] and (g["n_mono"], g["n_stereo"]) == (1, 1)  # mono before stereo
    assert g["n_matches"] == 4
    np.testing.assert_array_equal(g["pnp_points"][0], np.float32(p["points"][2]).astype(np.float64))
    assert g["pnp_points"][0, 0] != p["points"][2, 0]           # 6.1 is not a float
    np.testing.assert_array_equal(g["edges"][0], [0.1, 1.1, 2.1, 20.25, 2, 0, 400, 401, 300, 200, 40, 0])
    np.testing.assert_array_equal(g["edges"][1], [6.1, 7.1, 8.1, 10.5, 1, 5, 400, 401, 300, 200, 40, 1])
    # pose set: every edge an inlier -> track id 0 (i = 1) dropped, the edge-less matches kept
    ps, tid, kept = TR.write_back(g, [1, 1], n_inliers=2, min_num_match=1)
    assert ps and list(tid) == [7, -1, -1, 9, -1, 4] and list(kept) == [True, False, False, True, False, True]
    # the stereo edge (slot 1, i = 0) flagged as an outlier
    ps, tid, kept = TR.write_back(g, [1, 0], n_inliers=2, min_num_match=1)
    assert list(tid) == [-1, -1, -1, 9, -1, 4] and list(kept) == [False, False, False, True, False, True]
    # n_inliers == min_num_match is not `>`: nothing assigned, nothing removed
    ps, tid, kept = TR.write_back(g, [1, 0], n_inliers=2, min_num_match=2)
    assert not ps and list(tid) == [-1] * 6 and list(kept) == [True, True, False, True, False, True]


def test_track_ref_seed_gate():
    last = np.eye(4)
    R = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    used, q, p = TR.seed(20, R, [0.1, 0.2, 0.3], last)
    assert used and np.allclose(q, [0, 0, np.sqrt(0.5), np.sqrt(0.5)]) and list(p) == [0.1, 0.2, 0.3]
    for n, t in ((0, [0, 0, 0]), (9, [0.1, 0, 0]), (20, [0.4, 0.4, 0.0])):  # no model; too few; jump > 0.5 m
        used, q, p = TR.seed(n, R, t, last)
        assert not used and np.allclose(q, [0, 0, 0, 1]) and list(p) == [0, 0, 0]


def test_track_problem_shapes():
    from rspl_slam_amd import synthetic as SY
    p = SY.track_problem(n0=120, n1=100, n_common=70, seed=3, stereo_frac=0.5)
    assert set(np.unique(p["state"])) == {0, 1, 2}
    assert (p["track_id"] == 0).any() and (p["track_id"] == -1).any()
    mk = TR.matches(p["idx0"], p["idx1"], 120)
    assert (mk >= 0).sum() >= 70 and ((p["idx1"] >= 0) & (mk < 0)).any() and (p["idx1"] >= 120).any()
    assert p["features"].shape == (100, 259) and (p["u_right"] > 0).any() and (p["u_right"] < 0).any()
