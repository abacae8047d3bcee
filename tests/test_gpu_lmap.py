"""Local map tracking on the device (rspl_lmap_*): the search equals the numpy restatement (tests/lmap_ref.py) bit
for bit per local point and exactly in its lists -- the kernel and the restatement share the arithmetic's text
(csrc/lmap_match.hpp, whose host instantiation tests/test_lmap_cpu.py pins to the restatement) and the summation
order -- and the chain into the tracking step equals the existing Tracker handed the restatement's merged table.
The cases are tests/lmap_cases.py's: each asserts on the CPU that the restatement reaches the decision it is named
after, with margins above 1e-9 unless it is built on a boundary from exactly representable values.

Parity is with this project's restatement: the reference never calls this code, and it cannot be built here."""
import numpy as np
import pytest

import lmap_cases as LC
import lmap_ref as LR
from conftest import pkg
from rspl_slam_amd import capi

pytestmark = pytest.mark.gpu

K, L, B = 256, 256, 3


@pytest.fixture(scope="module")
def lm_handle():
    return pkg.LocalMap(max_bank_points=1024, max_local_points=L, max_keypoints=K, max_batch=B)


def _dev(a):
    a = np.ascontiguousarray(a)
    b = capi.DeviceBuffer(max(a.nbytes, 8))
    if a.nbytes:
        b.upload(a)
    return b


def _frame(fr):
    """the device side of one lmap_ref frame (the buffers live as long as the dict)"""
    n1 = len(fr["features"])
    d = dict(d_features=_dev(fr["features"]), d_n1=_dev(np.array([n1], np.int32)), d_point_id=_dev(fr["point_id"]),
             d_point_xyz=_dev(fr["point_xyz"]), Twc=fr["Twc"], cam=fr["cam"], width=fr["width"], height=fr["height"])
    if fr["u_right"] is not None:
        d["d_u_right"] = _dev(fr["u_right"])
    if fr.get("point_good") is not None:
        d["d_point_good"] = _dev(np.asarray(fr["point_good"], np.uint8))
    return d


def _load_local(h, lm):
    h.store_host(lm["ids"], lm["desc"])
    h.set_local(lm["ids"], lm["pos"])


def _check(h, frames, lm):
    """one enqueue of `frames` against `lm`: per point bitwise, the lists and the merged table exactly"""
    _load_local(h, lm)
    dev = [_frame(fr) for fr in frames]
    h.enqueue(dev)
    res = h.fetch()
    assert len(res) == len(frames)
    for b, (fr, r) in enumerate(zip(frames, res)):
        want = LR.search(fr, lm)
        LC.same_bits(h.debug_points(b), want)
        kp, pt = LR.good_list(want)
        assoc, _ = LR.merge(fr, lm, kp, pt)
        st = want["status"]
        assert r["n_keypoints"] == len(fr["features"])
        assert (r["n_selected"], r["n_projected"], r["n_with_candidates"], r["n_good"]) == \
            (int((st != LR.NOT_SELECTED).sum()), int((st >= LR.NO_CANDIDATE).sum()), int((st >= LR.FAILED).sum()), len(pt))
        np.testing.assert_array_equal(r["good_kp"], kp)
        np.testing.assert_array_equal(r["good_point"], pt)     # ascending: the list is in local order
        np.testing.assert_array_equal(r["assoc_id"], assoc)
    return res


@pytest.mark.parametrize("name", list(LC.DESIGNED))
def test_designed_cases(lm_handle, name):
    fr, lm = LC.DESIGNED[name]()
    _check(lm_handle, [fr], lm)


# keypoint counts 0, 1, 63, 64, 65, 130 (the chunk of 64 and its ballot), local points 0, 1, 4, 5, 65 (the last
# block of four waves partly empty), with and without a u_right array
@pytest.mark.parametrize("nk,nl", LC.SIZES)
@pytest.mark.parametrize("stereo", [False, True])
def test_size_boundaries(lm_handle, nk, nl, stereo):
    fr, lm = LC.random_scene(nk, nl, seed=100 * nk + nl, stereo=stereo)
    _check(lm_handle, [fr], lm)


def test_many_local_points():
    """600 local points: every wave of the merge walks several chunks of its quarter, the last quarter partly empty;
    more good projections than a chunk holds, several of them claiming one keypoint"""
    fr, lm = LC.random_scene(130, 600, seed=13600)
    h = pkg.LocalMap(max_bank_points=640, max_local_points=640, max_keypoints=K, max_batch=1)
    (r,) = _check(h, [fr], lm)
    assert r["n_good"] > 100 and len(set(r["good_kp"])) < r["n_good"]


def test_batch_of_three(lm_handle):
    """different poses, keypoint counts (130, 63, 1) and u_right arrays per frame; then a batch of one leaks nothing"""
    frames, lm = LC.batch_scenes()
    res = _check(lm_handle, frames, lm)
    assert [r["n_keypoints"] for r in res] == [130, 63, 1] and res[0]["n_good"] > 8 and res[1]["n_good"] > 4
    one = _check(lm_handle, frames[1:2], lm)
    fresh = pkg.LocalMap(max_bank_points=128, max_local_points=L, max_keypoints=K, max_batch=1)
    two = _check(fresh, frames[1:2], lm)
    for k in one[0]:
        np.testing.assert_array_equal(one[0][k], two[0][k], err_msg=k)


def test_store_from_device_records(lm_handle):
    """rspl_lmap_store copies rows 3..258 of the named records: a search against descriptors stored that way equals
    the one against the same descriptors stored from the host, bit for bit; an id stored again is overwritten"""
    fr, lm = LC.random_scene(65, 65, seed=6565)
    rec = np.zeros((80, 259))
    rows = np.random.default_rng(0).permutation(80)[:65]
    rec[rows, 3:] = lm["desc"]
    rec[:, :3] = 9.0  # (score, x, y are not part of a descriptor)
    d_rec = _dev(rec)
    h = pkg.LocalMap(max_bank_points=80, max_local_points=L, max_keypoints=K, max_batch=1)
    h.store_host(lm["ids"][:10], lm["desc"][10:20])  # wrong on purpose: the device store below overwrites them
    h.store(lm["ids"], rows, d_rec)
    assert h.bank_size() == 65
    h.set_local(lm["ids"], lm["pos"])
    h.enqueue([_frame(fr)])
    h.fetch()
    LC.same_bits(h.debug_points(0), LR.search(fr, lm))


def _run_chain(fr, lm, last, Kt=K):
    """track_enqueue into a tracker of capacity Kt, and the existing Tracker (same capacity) handed the restatement's
    merged table, identity indices and clamped keypoint count directly: the same kernels on the same inputs.
    The restatement sees the frame as the handle does: its first K keypoints."""
    n1 = min(len(fr["features"]), K)
    cut = dict(fr, features=fr["features"][:n1], point_id=fr["point_id"][:n1], point_xyz=fr["point_xyz"][:n1],
               u_right=None if fr["u_right"] is None else fr["u_right"][:n1],
               point_good=None if fr.get("point_good") is None else fr["point_good"][:n1])
    want = LR.search(cut, lm)
    kp, pt = LR.good_list(want)
    assoc, winner = LR.merge(cut, lm, kp, pt)
    pts, state, tid, idx = LR.track_table(cut, lm, winner, K)
    h = pkg.LocalMap(max_bank_points=512, max_local_points=L, max_keypoints=K, max_batch=1)
    _load_local(h, lm)
    t = pkg.Tracker(max_batch=1, max_keypoints=Kt)
    d = _frame(fr)
    tf = dict(slot=0, d_features=d["d_features"], d_n1=d["d_n1"], cam=fr["cam"], last_Twc=last)
    h.track_enqueue(t, [d], [tf])
    got, s = t.fetch()[0], h.fetch()[0]
    points = h.debug_points(0)
    table = t.debug_keyframe_table(0, K)
    t2 = pkg.Tracker(max_batch=1, max_keypoints=Kt)
    t2.set_keyframe(0, pts, state, tid)
    t2.enqueue([dict(tf, d_n1=_dev(np.array([n1], np.int32)), d_idx0=_dev(idx), d_idx1=_dev(idx))])
    ref = t2.fetch()[0]
    return dict(fr=cut, lm=lm, want=want, assoc=assoc, table=(pts, state, tid), got=got, s=s, ref=ref, points=points,
                dev_table=table, n_good=len(pt))


def _same_results(got, ref):
    assert set(got) == set(ref)
    for k in got:  # pose, inliers, track ids, kept, and every count
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(ref[k]), err_msg=k)


@pytest.fixture(scope="module")
def chain():
    fr, lm, gt, last = LC.chain_scene()
    return dict(_run_chain(fr, lm, last), gt=gt, last=last)


def test_keypoint_count_above_the_handles_capacity():
    """*d_n1 = 300 > max_keypoints = 256: the search, the merge and -- in a tracker of capacity 512 -- the tracking
    step all work on the first 256 keypoints; both fetches report 256"""
    fr, lm = LC.random_scene(300, 65, seed=30065)
    cut = dict(fr, features=fr["features"][:K], point_id=fr["point_id"][:K], point_xyz=fr["point_xyz"][:K])
    assert LR.margins(cut, lm) > LC.MARGIN and (fr["point_id"][K:] >= 0).any()
    h = pkg.LocalMap(max_bank_points=128, max_local_points=L, max_keypoints=K, max_batch=1)
    _load_local(h, lm)
    h.enqueue([_frame(fr)])          # the device arrays hold all 300 keypoints
    (r,) = h.fetch()
    want = LR.search(cut, lm)
    LC.same_bits(h.debug_points(0), want)
    kp, pt = LR.good_list(want)
    assert r["n_keypoints"] == K and len(pt) > 10
    np.testing.assert_array_equal(r["good_kp"], kp)
    np.testing.assert_array_equal(r["assoc_id"], LR.merge(cut, lm, kp, pt)[0])
    c = _run_chain(fr, lm, fr["Twc"], Kt=512)
    LC.same_bits(c["points"], want)
    assert c["got"]["n_keypoints"] == c["s"]["n_keypoints"] == K and len(c["got"]["track_id"]) == K
    for a, b in zip(c["dev_table"], c["table"]):
        np.testing.assert_array_equal(a, b)
    _same_results(c["got"], c["ref"])


def test_chain_with_points_that_are_not_good():
    """d_point_good: two of the frame's six own points are held but not Good (untriangulated): they keep their slot
    against the search (state RSPL_TRACK_NOT_GOOD) and are never an edge of the pose optimisation"""
    fr, lm, gt, last = LC.chain_scene()
    own = np.flatnonzero(fr["point_id"] >= 0)
    good = np.ones(len(fr["features"]), np.uint8)
    good[own[:2]] = 0
    c = _run_chain(dict(fr, point_good=good), lm, last)
    assert list(c["table"][1][own]) == [2, 2, 1, 1, 1, 1]
    for a, b in zip(c["dev_table"], c["table"]):
        np.testing.assert_array_equal(a, b)
    _same_results(c["got"], c["ref"])
    assert c["got"]["n_mono"] == 4 + c["n_good"] and c["got"]["pose_set"]
    np.testing.assert_array_equal(c["s"]["assoc_id"], c["assoc"])  # the held points stay in the merged table


def test_chain_merged_table(chain):
    for a, b in zip(chain["dev_table"], chain["table"]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(chain["s"]["assoc_id"], chain["assoc"])
    assert chain["s"]["n_good"] == chain["n_good"] >= 190
    assert int((chain["fr"]["point_id"] >= 0).sum()) == 6  # too few points of its own for the tracking step


def test_chain_equals_tracker_bitwise(chain):
    got, ref = chain["got"], chain["ref"]
    _same_results(got, ref)
    assert got["pose_set"] and got["n_mono"] == 6 + chain["n_good"] and got["n_inliers"] > 190


def test_chain_recovers_ground_truth(chain):
    """The scene is noise-free (every keypoint is the exact projection of its point), so the pose is held to the
    1e-9 that tests/test_gpu_track.py holds the chain to against its oracle, here against the ground truth."""
    from rspl_slam_amd import synthetic as SY
    got, gt = chain["got"], chain["gt"]
    assert np.abs(got["pose_p"] - gt[:3, 3]).max() < 1e-9
    assert np.abs(SY.quat_xyzw_to_R(got["pose_q"]) - gt[:3, :3]).max() < 1e-9
    # track ids: every merged keypoint keeps its point's id (id 0 would be dropped by `> 0`; none here)
    np.testing.assert_array_equal(got["track_id"], chain["assoc"])


def test_track_local_map_gates(chain):
    fr, lm = chain["fr"], chain["lm"]
    h = pkg.LocalMap(max_bank_points=512, max_local_points=L, max_keypoints=K, max_batch=1)
    _load_local(h, lm)
    t = pkg.Tracker(max_batch=1, max_keypoints=K)
    d = _frame(fr)
    n, out = pkg.TrackLocalMap(None, h, t, d)
    assert n == chain["got"]["n_inliers"] > 10
    np.testing.assert_array_equal(out["pose_p"], chain["got"]["pose_p"])
    np.testing.assert_array_equal(out["track_id"], chain["assoc"])
    assert pkg.TrackLocalMap(None, h, t, d, min_num_match=n)[0] == -1           # n_inliers <= min_num_match
    assert pkg.TrackLocalMap(None, h, t, d, min_num_match=n - 1)[0] == n
    assert pkg.TrackLocalMap(None, h, t, d, num_inlier_thr=n)[0] == -1          # n_inliers <= num_inlier_thr
    assert pkg.TrackLocalMap(None, h, t, d, num_inlier_thr=n - 1)[0] == n
    h.set_local(lm["ids"][:2], lm["pos"][:2])                                   # fewer than 3 good projections
    n2, out2 = pkg.TrackLocalMap(None, h, t, d)
    assert n2 == -1 and out2["n_good"] == 2 and "pose_q" not in out2


def test_chain_from_the_map(chain):
    """TrackLocalMap with a reference keyframe: the local map comes from the native map's neighbours"""
    fr, lm = chain["fr"], chain["lm"]
    m = pkg.mapping.Map(fr["cam"])
    n = len(lm["ids"])
    for f in (1, 2):
        m.InsertKeyframe(f, float(f), np.eye(4), np.zeros((n, 3)))
    m.InsertMappoints(lm["ids"], lm["pos"])
    m.AddPointObservations(1, lm["ids"][:30], np.arange(30))
    m.AddPointObservations(2, lm["ids"], np.arange(n)[::-1].copy())  # frame 2 holds the local map, reversed
    m.UpdateFrameConnection(1)
    assert m.GetOrderedConnections(1) == [(30, 2)]
    h = pkg.LocalMap(max_bank_points=512, max_local_points=L, max_keypoints=K, max_batch=1)
    h.store_host(lm["ids"], lm["desc"])
    t = pkg.Tracker(max_batch=1, max_keypoints=K)
    ninl, out = pkg.TrackLocalMap(m, h, t, _frame(fr), ref_keyframe=1)
    assert h.n_local == n and ninl == chain["got"]["n_inliers"]
    rev = dict(ids=lm["ids"][::-1], pos=lm["pos"][::-1], desc=lm["desc"][::-1])
    kp, pt = LR.good_list(LR.search(fr, rev))
    np.testing.assert_array_equal(out["good_kp"], kp)
    np.testing.assert_array_equal(out["good_point"], pt)


def test_enqueue_contract(lm_handle):
    fr, lm = LC.random_scene(5, 1, seed=1)
    _load_local(lm_handle, lm)
    d = _frame(fr)
    with pytest.raises(capi.RsplError, match="exceeds max_batch"):
        lm_handle.enqueue([d] * (B + 1))
    with pytest.raises(capi.RsplError, match="NULL device pointer"):
        lm_handle.enqueue([dict(d, d_point_id=None)])
    lm_handle.enqueue([d])
    with pytest.raises(capi.RsplError, match="has not been fetched"):
        lm_handle.enqueue([d])
    with pytest.raises(capi.RsplError, match="in flight"):
        lm_handle.set_local(lm["ids"], lm["pos"])
    lm_handle.fetch()
    small = pkg.Tracker(max_batch=1, max_keypoints=K // 2)  # the tracker's slots cannot hold the merged table
    with pytest.raises(capi.RsplError, match="exceeds max_keypoints"):
        lm_handle.track_enqueue(small, [d], [dict(slot=0, d_features=d["d_features"], d_n1=d["d_n1"], cam=fr["cam"],
                                                  last_Twc=np.eye(4))])
    lm_handle.enqueue([])
    assert lm_handle.fetch() == []
