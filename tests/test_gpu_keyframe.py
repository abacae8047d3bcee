"""Keyframe insertion on the device (rspl_kf_*, rspl_track_keyframe_table, rspl_map_insert_keyframe with a
device): the stereo stage against the restatement (tests/kf_ref.py) at the scan's seams, the hand-off of a
keyframe table to the tracker in stream order, the batched Map::TriangulateMappoint against the host
instantiation (bit for bit) and the restatement (the CPU test's bound), and an 8-keyframe raw sequence end to
end against the restatement + oracle/map_ref.py's LocalMapOptimization with the oracle BA."""
import numpy as np
import pytest

import kf_ref as KR
import map_ref
import oracle
from conftest import pkg
from kf_cases import CAM, check_triangulation, ref_stage, tri_cases
from rspl_slam_amd import capi, sequence as SQ, synthetic as SY

pytestmark = pytest.mark.gpu

K = 1024
COUNTS = ("n_keypoints", "n_matches", "n_stereo_matches", "n_new_ids", "n_new_points", "n_new_good", "next_track_id")


@pytest.fixture(scope="module")
def kf():
    return pkg.KeyframeBuilder(max_batch=3, max_keypoints=K, max_tri_points=512, max_tri_observations=4096)


def _dev(a):
    a = np.ascontiguousarray(a)
    b = capi.DeviceBuffer(max(a.nbytes, 8))
    if a.nbytes:
        b.upload(a)
    return b


def _frame(p, init=False, table=None):
    d = dict(d_features_left=_dev(p["feat_left"]), d_features_right=_dev(p["feat_right"]),
             d_n_left=_dev(np.array([len(p["feat_left"])], np.int32)),
             d_n_right=_dev(np.array([len(p["feat_right"])], np.int32)), d_idx0=_dev(p["idx0"]), d_idx1=_dev(p["idx1"]),
             cam=p["cam"], window=p["window"], Twc=p["Twc"], next_track_id=p["next_track_id"], init=init,
             track_id=p["track_id"], point_slot=p["point_slot"], points=p["points"], state=p["state"])
    if table is not None:
        d["table"] = table
    return d


def _run(kf, probs, init=False):
    frames = [_frame(p, init) for p in probs]  # (holds the device buffers until the fetch)
    kf.enqueue(frames)
    return kf.fetch()


def _check_stage(r, g):
    for k in COUNTS:
        assert r[k] == g[k], k
    for k in ("track_id", "new_point"):
        np.testing.assert_array_equal(r[k], g[k], err_msg=k)
    for k in ("u_right", "depth", "new_position"):   # a handful of IEEE operations, contraction off: bitwise
        assert r[k].tobytes() == g[k].tobytes(), k


def _problem(n, need, seed):
    return SY.keyframe_problem(n_left=n, n_right=n + 5 if n else 0, n_common=(3 * n) // 4, seed=seed, need_id=need)


# the scan's seams: empty, one lane, a wave -1 / exact / +1, a chunk -1 / exact / +1, several chunks, the cap
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513, K])
def test_stereo_stage_matches_ref(kf, n):
    probs = [_problem(min(n, K - 5) if n == K else n, need, 10 * n + k) for k, need in enumerate(("all", "none", "third"))]
    if n == K:   # the cap on the left side (the right side then has K - 5 + 5 keypoints)
        probs[0] = SY.keyframe_problem(n_left=K, n_right=K, n_common=700, seed=3, need_id="all")
    for init in (False, True):
        res = _run(kf, probs, init)
        for p, r, need in zip(probs, res, ("all", "none", "third")):
            g = KR.stereo(p, init=init)
            nl = len(p["feat_left"])
            assert r["n_keypoints"] == nl
            if not init:
                assert g["n_new_ids"] == {"all": nl, "none": 0, "third": (nl + 2) // 3}[need]
            else:
                assert g["n_new_ids"] == nl
            _check_stage(r, g)


def test_batch_frames_are_independent(kf):
    """three frames of different sizes in one enqueue = each of them alone"""
    probs = [_problem(257, "third", 1), _problem(64, "all", 2), _problem(513, "none", 3)]
    together = _run(kf, probs)
    for p, r in zip(probs, together):
        (alone,) = _run(kf, [p])
        _check_stage(r, KR.stereo(p))
        for k in COUNTS:
            assert r[k] == alone[k]
        for k in ("u_right", "depth", "track_id", "new_point", "new_position"):
            assert r[k].tobytes() == alone[k].tobytes(), k
    assert 0 < together[0]["n_stereo_matches"] < together[0]["n_matches"]
    assert ((together[0]["u_right"] > 0) & (together[0]["depth"] < 0)).any()   # right-of-left partners survive


def test_enqueue_rejects_bad_frames(kf):
    p = _problem(64, "third", 5)
    f = _frame(p)
    for bad in (dict(d_idx1=None), dict(next_track_id=-1), dict(cam=(0.0, 1.0, 1.0, 1.0, 1.0)),
                dict(table=dict(points=1 << 20, state=None, track_id=None, capacity=8))):
        with pytest.raises(capi.RsplError):
            kf.enqueue([dict(f, **bad)])
    with pytest.raises(capi.RsplError):
        kf.enqueue([f] * 4)   # max_batch = 3
    assert _run(kf, [p])[0]["n_keypoints"] == 64   # the handle is still usable


def test_tracker_hand_off(kf):
    """A tracker slot filled by the chain = the table rspl_track_set_keyframe uploads from the fetched result,
    byte for byte; tracking against either slot gives the same result."""
    tp = SY.track_problem(n0=400, n1=380, n_common=300, seed=9, stereo_frac=0.3)
    n0 = 400
    p = SY.keyframe_problem(n_left=n0, n_right=390, n_common=300, seed=4)
    # the keyframe holds the tracking problem's map points (states 0 / 1 / 2 pass through), a few ids are new
    p.update(track_id=tp["track_id"], point_slot=np.arange(n0, dtype=np.int32), points=tp["points"], state=tp["state"])
    p["point_slot"][::50] = -1   # and a few keypoints get a new map point from the stereo stage
    tr = pkg.Tracker(max_batch=2, max_keypoints=K)
    kf.enqueue([_frame(p, table=tr.keyframe_table(0, n0))])
    (r,) = kf.fetch()
    g = KR.stereo(p)
    _check_stage(r, g)
    held = p["point_slot"] >= 0
    pts = np.where(held[:, None], p["points"], r["new_position"])
    state = np.where(held, p["state"], r["new_point"]).astype(np.uint8)   # RSPL_KF_NEW_* = RSPL_TRACK_* for new points
    tr.set_keyframe(1, pts, state, r["track_id"])
    a, b = tr.debug_keyframe_table(0, n0), tr.debug_keyframe_table(1, n0)
    for x, y, z in zip(a, b, g["table"]):
        assert x.tobytes() == y.tobytes() == z.astype(x.dtype).tobytes()
    assert set(np.unique(a[1])) == {0, 1, 2} and (a[2] >= p["next_track_id"]).any()
    # one frame tracked against both slots in one enqueue
    fr = dict(d_features=_dev(tp["features"]), d_n1=_dev(np.array([len(tp["idx1"])], np.int32)), d_idx0=_dev(tp["idx0"]),
              d_idx1=_dev(tp["idx1"]), d_u_right=_dev(tp["u_right"]), cam=tp["cam"], last_Twc=tp["last_Twc"])
    tr.enqueue([dict(fr, slot=0), dict(fr, slot=1)])
    r0, r1 = tr.fetch()
    assert r0["pose_set"] and r0["n_inliers"] > 50
    for k, v in r0.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == r1[k].tobytes(), k
        else:
            assert v == r1[k], k


@pytest.fixture(scope="module")
def tri():
    c = tri_cases()
    return c, KR.triangulate(c[0], CAM, c[1], c[2], c[3]), KR.triangulate(c[0], CAM, c[1], c[2], c[3], reverse=True)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300, None])
def test_triangulate_device(kf, tri, n):
    """the device against the host instantiation (the same routine: bit for bit) and the restatement"""
    case, ref, ref_rev = tri
    poses, off, op, xy, names = case
    n = len(names) if n is None else n   # None: the random points and the special cases
    m = off[n]
    sub = (poses, off[:n + 1], op[:m], xy[:m], names[:n])
    pos, st = kf.triangulate(poses, CAM, sub[1], sub[2], sub[3])
    hpos, hst = kf.triangulate(poses, CAM, sub[1], sub[2], sub[3], host=True)
    assert pos.shape == (n, 3) and pos.tobytes() == hpos.tobytes()
    np.testing.assert_array_equal(st, hst)
    cut = lambda r: (r[0][:n], r[1][:n], r[2][:n], r[3][:n], r[4][:n])  # noqa: E731
    check_triangulation(sub, cut(ref), cut(ref_rev), pos, st)


def test_triangulate_capacity(kf):
    off = np.arange(0, 2 * 600 + 1, 2, dtype=np.int32)   # 600 points > max_tri_points = 512
    with pytest.raises(capi.RsplError, match="rc=-4"):
        kf.triangulate(np.eye(4)[None], CAM, off, np.zeros(1200, np.int32), np.zeros((1200, 2)))




# The sequence of the end-to-end test.  Two BA runs that sum in different orders agree to test_gpu_map.py's
# bounds only where the problem is well conditioned, which is decided on the CPU path alone (asserted below:
# a one-ulp change of the triangulated points moves the oracle path's poses and points by less than a hundredth
# of the bounds).  That holds with the analytic limit of g2o's numeric line Jacobian on both sides
# (tests/test_gpu_map.py's trajectory test gives the reason), 1 m between keyframes (parallax for the mono
# points) and no gross outliers among the observations: with map_sequence's defaults the oracle path moves by
# 3e-7 (poses) and 2e-4 (points) under the same one-ulp change, more than the bounds themselves, because a
# point triangulated from a 30-80 px outlier leaves the BA far from converged at its iteration cap.
E2E = dict(n_keyframes=8, n_points=600, n_lines=10, seed=1, step=1.0, outlier_frac=0.0)
POSE_ATOL, POINT_ATOL = 1e-7, 1e-6   # tests/test_gpu_map.py


def _cpu_path(seq, perturb=False):
    """The restatement + oracle map + oracle BA over the sequence.  Per keyframe a snapshot: poses, points
    (position, type, observers), frame slots, lines (type, observers); the insertion reports; the pivot ratios."""
    mr = map_ref.Map(seq["camera"])
    next_tid = next_line = 0
    hist, reps, ratios = [], [], []
    for k, f in enumerate(seq["keyframes"]):
        s = ref_stage(seq, f, k, mr, next_tid)
        next_tid = s["next_track_id"]
        rep, next_line = KR.insert_keyframe(mr, f, s, next_line)
        ratios += rep["ratios"]
        reps.append(rep)
        if perturb:
            for pid, st, p, A, nv in rep["tri"]:
                if st == KR.TRI_OK:
                    mr.mappoints[pid].p = mr.mappoints[pid].p * (1 + 2.0 ** -52)
        if k >= 1:
            map_ref.local_map_optimization(mr, f["id"], oracle.ba_local)
        hist.append(dict(
            poses={g["id"]: mr.keyframes[g["id"]].pose.copy() for g in seq["keyframes"][:k + 1]},
            points={i: (q.p.copy(), q.type, dict(q.obs)) for i, q in mr.mappoints.items()},
            slots={g["id"]: ([-1 if q is None else q.id for q in mr.keyframes[g["id"]].mappoints],
                             [-1 if l is None else l.id for l in mr.keyframes[g["id"]].maplines])
                   for g in seq["keyframes"][:k + 1]},
            lines={i: (l.type, dict(l.obs)) for i, l in mr.maplines.items()}))
    return hist, reps, np.array(ratios), next_tid


def test_end_to_end_raw_sequence(kf):
    """sequence.run_raw (rspl_kf + rspl_ba) against the restatement + the oracle map and BA, keyframe by keyframe"""
    seq = SY.raw_sequence(SY.map_sequence(**E2E))
    ba = pkg.LocalBA(max_poses=16, max_points=2000, max_lines=64, max_edges=20000)
    ba.set_line_jacobian(True)
    oracle.ba_set_line_jacobian(True)
    try:
        hist, reps, ratios, next_tid = _cpu_path(seq)
        hist2, _, _, _ = _cpu_path(seq, perturb=True)
        # the CPU path's own conditioning: a one-ulp change of its triangulated points, after every keyframe
        for h, h2 in zip(hist, hist2):
            assert max(np.abs(h["poses"][i] - h2["poses"][i]).max() for i in h["poses"]) < POSE_ATOL / 100
            assert max(np.abs(h["points"][i][0] - h2["points"][i][0]).max() for i in h["points"]) < POINT_ATOL / 100
            assert all(h["points"][i][1:] == h2["points"][i][1:] for i in h["points"])
        # no rank decision of the CPU path lies within a relative 1e-3 of the threshold (poses agree to 1e-7 and
        # the parallax is >= 3e-3, so a ratio moves by about 1e-4 between the two sides): none may be excused
        assert len(ratios) > 50 and np.abs(ratios / KR.RANK_TOL - 1.0).min() > 1e-3

        def check(k, m):   # the GPU side inserted and optimised keyframe k
            h = hist[k]
            for fid, T in h["poses"].items():
                np.testing.assert_allclose(m.GetPose(fid), T, rtol=0, atol=POSE_ATOL, err_msg=f"keyframe {k}: pose {fid}")
                a, b = m.FrameSlots(fid)
                assert (list(a), list(b)) == h["slots"][fid], (k, fid)
            for pid, (rp, rt, robs) in h["points"].items():
                p, t, obs = m.GetMappoint(pid)
                assert t == rt and obs == robs, (k, pid)
                np.testing.assert_allclose(p, rp, rtol=0, atol=POINT_ATOL, err_msg=f"keyframe {k}: point {pid}")
            for lid, (lt, lobs) in h["lines"].items():
                t = m.GetMapline(lid)[1]
                assert t == lt and {f: i for f, i, _ in m.GetMaplineObservers(lid)} == lobs, (k, lid)

        m, reports, stages = SQ.run_raw(seq, ba, kf, on_keyframe=check)
    finally:
        ba.set_line_jacobian(False)
        oracle.ba_set_line_jacobian(False)
    for rep, ref in zip(reports, reps):   # rank decisions equal
        for key in ("n_new_points", "n_new_lines", "n_tri_candidates", "n_tri_ok", "n_tri_rank_failures",
                    "n_lines_triangulated"):
            assert rep[key] == ref[key], key
    assert sum(r["n_tri_ok"] for r in reports) > 0 and sum(r["n_tri_rank_failures"] for r in reports) > 0
    assert sum(r["n_lines_triangulated"] for r in reports) > 0
    assert all(r["optimization"] is not None for r in reports[1:]) and reports[0]["optimization"] is None
    assert next_tid == stages[-1]["next_track_id"] == len(seq["point_ids"])


def test_create_destroy_cycle():
    """20 handles of the smallest capacities created and destroyed (pinned arena, stream, event), then one more:
    its stereo stage and its triangulation equal the first handle's bit for bit."""
    from helpers import assert_same, cycle_handle
    p = SY.keyframe_problem(n_left=8, n_right=8, n_common=6, seed=1)
    poses, off, op, xy, _ = tri_cases()
    off = off[:9]  # 8 points
    m = int(off[-1])

    def run(h):
        return _run(h, [p]), h.triangulate(poses, CAM, off, op[:m], xy[:m])

    first, last = cycle_handle(lambda: pkg.KeyframeBuilder(max_batch=1, max_keypoints=8, max_tri_points=8,
                                                           max_tri_observations=max(m, len(poses))), run)
    assert first[0][0]["n_matches"] > 0
    assert_same(first, last)
