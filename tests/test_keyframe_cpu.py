"""CPU-side checks of keyframe insertion (rspl_kf_*, rspl_map_insert_keyframe): the boundary is declared and
bound, bad capacities are refused before a device is touched, the restatement (tests/kf_ref.py) does what
frame.cc:150-177 / map_builder.cc:390-403, :660-665 / map.cc:40-55 do on a hand-made stereo case, the host
instantiation of the triangulation routine (csrc/kf_triangulate.hpp) against the restatement, and the native
map insertion without a device (kfh = NULL, ba = NULL) against the restatement on oracle/map_ref's structures."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import kf_ref as KR
import map_ref
from kf_cases import CAM, check_triangulation, compare_maps, ref_stage, tri_cases

ROOT = pathlib.Path(__file__).resolve().parents[1]
FUNCS = ("rspl_kf_create", "rspl_kf_destroy", "rspl_kf_enqueue", "rspl_kf_fetch", "rspl_kf_triangulate",
         "rspl_track_keyframe_table", "rspl_map_insert_keyframe", "rspl_map_get_mapline_observers")


def test_header_declares_keyframe_api():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    for n in FUNCS:
        assert n in names
    for s in ("rspl_kf_config", "rspl_kf_frame", "rspl_kf_result", "rspl_map_tracks", "rspl_map_insert_report"):
        assert re.search(r"}\s*%s;" % s, hdr), s
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct changed


def test_capi_binds_keyframe_api():
    from rspl_slam_amd import capi, mapping
    lib = mapping._declare(capi.load())
    for n in FUNCS:
        assert n in capi.EXPORTS and hasattr(lib, n)
    assert len(lib.rspl_kf_enqueue.argtypes) == 4 and len(lib.rspl_kf_triangulate.argtypes) == 10
    assert len(lib.rspl_map_insert_keyframe.argtypes) == 6
    assert [f[0] for f in capi.KfConfig._fields_] == ["max_batch", "max_keypoints", "max_tri_points",
                                                      "max_tri_observations", "device"]


@pytest.mark.parametrize("kw", [dict(max_batch=0), dict(max_keypoints=0), dict(max_batch=-1, max_keypoints=16),
                                dict(max_tri_points=-1), dict(max_tri_observations=-5)])
def test_builder_rejects_bad_capacities(kw):
    import rspl_loader
    pkg = rspl_loader.load()
    with pytest.raises(ValueError):
        pkg.KeyframeBuilder(**kw)


def test_create_rejects_bad_capacities_before_the_device():
    from rspl_slam_amd import capi
    lib = capi.load()
    for cfg in ((0, 64, 8, 8), (4, 0, 8, 8), (4, 64, -1, 8), (4, 64, 8, -1), (1 << 20, 1 << 20, 8, 8)):
        h = C.c_void_p()
        c = capi.KfConfig(*cfg, 0)
        assert lib.rspl_kf_create(C.byref(c), C.byref(h)) == -1  # RSPL_E_ARG, not a device error
        assert not h.value


# ---------------------------------------------------------------------------------------------------------
# the stereo stage, by hand
# ---------------------------------------------------------------------------------------------------------
def _hand_case():
    mn, mx, my = 4.0, 100.0, 2.0
    #  i  xl     partner  xr      dy    track id  slot   what
    #  0  200    r2       180     0.5     -1       -1    mutual, in the window
    #  1  300    r0 (r0 -> 4)             11       -1    not mutual
    #  2  250    r1       246     0        -1       -1    dx == min_x_diff exactly: rejected (strict)
    #  3  400    r3       350     2.0      12       -1    dy == max_y_diff: kept
    #  4  100    r4       130     0        -1       -1    right of left: u_right > 0, depth < 0, UnTriangulated
    #  5  500    r5       460     1.0      13       13    holds map point 13
    #  6  600    -                          -1       -1    unmatched
    FL, FR = np.zeros((7, 259)), np.zeros((6, 259))
    FL[:, 1] = [200, 300, 250, 400, 100, 500, 600]
    FL[:, 2] = [50, 60, 70, 80, 90, 100, 110]
    FR[:, 1] = [290, 246, 180, 350, 130, 460]
    FR[:, 2] = [60, 70, 50.5, 82.0, 90, 101.0]
    idx0 = np.array([2, 0, 1, 3, 4, 5, -1], np.int32)
    idx1 = np.array([4, 2, 0, 3, 4, 5], np.int32)   # r0 -> 4: left 1 is not mutual (and left 4's partner is r4)
    T = np.eye(4)
    T[:3, 3] = [1.0, 2.0, 3.0]
    pts = np.zeros((7, 3))
    pts[5] = [7.0, 8.0, 9.0]
    return dict(feat_left=FL, feat_right=FR, idx0=idx0, idx1=idx1, track_id=np.array([-1, 11, -1, 12, -1, 13, -1], np.int32),
                point_slot=np.array([-1, -1, -1, -1, -1, 13, -1], np.int32), points=pts,
                state=np.array([0, 0, 0, 0, 0, 1, 0], np.uint8), cam=(400.0, 400.0, 300.0, 200.0, 40.0),
                window=(mn, mx, my), Twc=T, next_track_id=100)


def test_kf_ref_hand_case():
    p = _hand_case()
    r = KR.stereo(p)
    assert (r["n_matches"], r["n_stereo_matches"]) == (5, 4)          # 1 and 6 have no partner; 2 is rejected
    assert list(r["u_right"]) == [180, -1, -1, 350, 130, 460, -1]
    assert list(r["depth"]) == [40 / 20, -1, -1, 40 / 50, 40 / -30, 40 / 40, -1]
    assert r["u_right"][4] > 0 and r["depth"][4] < 0                   # a partner to the right (frame.cc:176)
    # ids: every keypoint without one, ascending (map_builder.cc:660-665)
    assert list(r["track_id"]) == [100, 11, 101, 12, 102, 13, 103] and r["next_track_id"] == 104
    # new points: Good with a depth, UnTriangulated without (the negative depth fails BackProjectPoint), none held
    assert list(r["new_point"]) == [1, 2, 2, 1, 2, 0, 2]
    d = 40.0 / 20
    np.testing.assert_array_equal(r["new_position"][0], [(200 - 300) / 400 * d + 1, (50 - 200) / 400 * d + 2, d + 3])
    assert not r["new_position"][4].any()
    tp, ts, tt = r["table"]
    assert list(ts) == [1, 2, 2, 1, 2, 1, 2] and list(tp[5]) == [7, 8, 9] and list(tt) == list(r["track_id"])
    # init (MapBuilder::Init :390-403 then :660-665): the keypoints with a depth first, the ids passed in ignored,
    # no map point without a depth
    q = KR.stereo(dict(p, point_slot=None), init=True)
    assert list(q["track_id"]) == [100, 103, 104, 101, 105, 102, 106] and q["next_track_id"] == 107
    assert list(q["new_point"]) == [1, 0, 0, 1, 0, 1, 0]
    assert list(q["table"][1]) == [1, 0, 0, 1, 0, 1, 0]


def test_keyframe_problem_covers_every_kind():
    from rspl_slam_amd import synthetic as SY
    p = SY.keyframe_problem(n_left=200, n_right=180, n_common=120, seed=2)
    r = KR.stereo(p)
    assert set(np.unique(p["kind"])) == {0, 1, 2, 3, 4, 5}
    assert 0 < r["n_stereo_matches"] < r["n_matches"] < 200
    assert ((r["u_right"] > 0) & (r["depth"] < 0)).sum() >= 10          # right-of-left partners
    assert (p["idx0"] >= 180).any() and (p["idx1"] >= 200).any()       # out of range
    assert set(np.unique(r["new_point"])) == {0, 1, 2} and (p["point_slot"] >= 0).any()
    assert r["n_new_ids"] == int((p["track_id"] < 0).sum())


# ---------------------------------------------------------------------------------------------------------
# Map::TriangulateMappoint: the host instantiation of csrc/kf_triangulate.hpp against the restatement
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tri():
    c = tri_cases()
    return c, KR.triangulate(c[0], CAM, c[1], c[2], c[3]), KR.triangulate(c[0], CAM, c[1], c[2], c[3], reverse=True)


def test_triangulate_host_vs_ref(tri):
    import rspl_loader
    pkg = rspl_loader.load()
    case, ref, ref_rev = tri
    poses, off, op, xy, names = case
    pos, st = pkg.triangulate_points(poses, CAM, off, op, xy)
    by = dict(zip(names, ref[1]))
    assert by["one valid observer"] == by["no observer"] == KR.TRI_FEW
    assert by["identical bearings"] == KR.TRI_RANK
    assert by["ratio 5e-06"] == KR.TRI_RANK and by["ratio 2e-05"] == KR.TRI_OK
    r = dict(zip(names, ref[2]))
    assert abs(r["ratio 5e-06"] / 0.5e-5 - 1) < 1e-3 and abs(r["ratio 2e-05"] / 2e-5 - 1) < 1e-3
    assert (ref[1][:300] == KR.TRI_OK).sum() > 250
    check_triangulation(case, ref, ref_rev, pos, st)


def test_triangulate_rejects_bad_arguments():
    from rspl_slam_amd import capi
    lib = capi.load()
    T, cam = np.eye(4).reshape(1, 16).copy(), np.array(CAM[:4])
    pos, st = np.zeros(3), np.zeros(1, np.uint8)
    xy = np.zeros((2, 2))
    for off, op in (([0, 2], [0, 1]), ([1, 2], [0, 0]), ([0, 2, 1], [0, 0])):   # a pose past n_poses; offsets
        off, op = np.array(off, np.int32), np.array(op, np.int32)
        rc = lib.rspl_kf_triangulate(None, 1, T.ctypes.data, cam.ctypes.data, len(off) - 1, off.ctypes.data,
                                     op.ctypes.data, xy.ctypes.data, np.zeros(6).ctypes.data, np.zeros(2, np.uint8).ctypes.data)
        assert rc == -1


# ---------------------------------------------------------------------------------------------------------
# rspl_map_insert_keyframe without a device against the restatement
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw6():
    from rspl_slam_amd import synthetic as SY
    return SY.raw_sequence(SY.map_sequence(n_keyframes=6, n_points=300, n_lines=10, seed=3))


def test_map_insert_keyframe_vs_ref(raw6):
    from rspl_slam_amd.mapping import Map
    seq = raw6
    m, mr = Map(seq["camera"]), map_ref.Map(seq["camera"])
    next_tid = next_line = next_line_ref = 0
    bounds, totals = {}, dict(cand=0, ok=0, rank=0, lines=0, new_untri=0)
    for k, f in enumerate(seq["keyframes"]):
        s = ref_stage(seq, f, k, mr, next_tid)
        next_tid = s["next_track_id"]
        rep_ref, next_line_ref = KR.insert_keyframe(mr, f, s, next_line_ref)
        kp = np.column_stack([f["feat_left"][:, 1:3], s["u_right"]])
        tracks = dict(track_id=s["track_id"], point_slot=f["point_slot"], new_point=s["new_point"],
                      new_position=s["new_position"], line_track_id=f["line_track_id"], line_slot=f["line_slot"],
                      next_line_track_id=next_line)
        rep = m.InsertKeyframeFull(f["id"], f["timestamp"], f["Twc"], kp, tracks, f["lines_left"], f["lines_right"],
                                   f["lines_right_valid"], f["points_on_lines"], f["parent_id"])
        next_line = rep["next_line_track_id"]
        assert next_line == next_line_ref and rep["optimization"] is None
        for key in ("n_new_points", "n_new_lines", "n_tri_candidates", "n_tri_ok", "n_tri_rank_failures",
                    "n_lines_triangulated"):
            assert rep[key] == rep_ref[key], (k, key)
        if rep_ref["ratios"]:
            assert np.abs(np.array(rep_ref["ratios"]) / KR.RANK_TOL - 1.0).min() > 1e-8
        for pid, st, p, A, nv in rep_ref["tri"]:
            if st == KR.TRI_OK:
                bounds[pid] = KR.position_bound(A, nv, p)
        compare_maps(m, mr, seq["keyframes"][:k + 1], bounds)
        totals["cand"] += rep["n_tri_candidates"]
        totals["ok"] += rep["n_tri_ok"]
        totals["rank"] += rep["n_tri_rank_failures"]
        totals["lines"] += rep["n_lines_triangulated"]
        totals["new_untri"] += int((s["new_point"] == 2).sum())
        if k == 0:   # MapBuilder::Init: ids for the keypoints with a depth first, map points only for them
            assert rep["n_new_points"] == int((s["depth"] > 0).sum()) and rep["n_tri_candidates"] == 0
    # the sequence exercises every path: mono points triangulated from three observers, lines from map points
    assert totals["new_untri"] > 0 and totals["cand"] > 0 and totals["ok"] > 0 and totals["lines"] > 0, totals
    # the ids the sequence predicted are the ones insertion handed out
    assert next_tid == len(seq["point_ids"]) and next_line == len(seq["line_ids"])


def test_duplicate_landmark_id_is_refused(raw6):
    from rspl_slam_amd import capi
    from rspl_slam_amd.mapping import Map
    seq = raw6
    m, mr = Map(seq["camera"]), map_ref.Map(seq["camera"])
    f = seq["keyframes"][0]
    s = ref_stage(seq, f, 0, mr, 0)
    kp = np.column_stack([f["feat_left"][:, 1:3], s["u_right"]])
    args = (f["timestamp"], f["Twc"], kp)
    tracks = dict(track_id=s["track_id"], point_slot=f["point_slot"], new_point=s["new_point"],
                  new_position=s["new_position"], next_line_track_id=0)
    m.InsertKeyframeFull(f["id"], *args, tracks)
    with pytest.raises(capi.RsplError, match=r"rc=-1.*already in the map"):   # the same new ids again
        m.InsertKeyframeFull(f["id"] + 1, *args, tracks)
    with pytest.raises(capi.RsplError):                                       # refused before the map changed
        m.GetPose(f["id"] + 1)
    dup = dict(tracks, track_id=np.full(len(kp), 999999, np.int32), new_point=np.ones(len(kp), np.uint8))
    with pytest.raises(capi.RsplError, match=r"rc=-1.*already in the map"):   # twice in one call
        m.InsertKeyframeFull(f["id"] + 2, *args, dup)
    held = dict(tracks, point_slot=np.full(len(kp), 555555, np.int32))
    with pytest.raises(capi.RsplError, match=r"rc=-1.*not in the map"):       # a held point the map lacks
        m.InsertKeyframeFull(f["id"] + 3, *args, held)
