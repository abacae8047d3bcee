"""The device-resident tracking step (rspl_track_*: MapBuilder::TrackFrame + FramePoseOptimization,
src/map_builder.cc:448-611) checked stage by stage through rspl_track_debug_stage against the numpy
restatement of the host steps (tests/track_ref.py) and the fp64 oracles of the two solvers
(oracle.pnp, oracle.pnp_subsets, oracle.frame_opt), then end to end against the fully CPU chain.
Inputs are synthetic arrays uploaded to device memory; no SuperPoint / SuperGlue run is needed."""
import numpy as np
import pytest

import oracle
import track_ref as TR
from conftest import pkg
from rspl_slam_amd import capi, synthetic as SY

pytestmark = pytest.mark.gpu

K = 1024


@pytest.fixture(scope="module")
def tr():
    return pkg.Tracker(max_batch=4, max_keypoints=K)


@pytest.fixture(scope="module")
def tr512():  # the launch bound min(n0, max_keypoints) <= 512: FrameOptimization's LDS path
    return pkg.Tracker(max_batch=2, max_keypoints=512)


def _dev(a):
    a = np.ascontiguousarray(a)
    b = capi.DeviceBuffer(max(a.nbytes, 8))
    if a.nbytes:
        b.upload(a)
    return b


def _run(t, probs, **kw):
    """One enqueue of `probs` (keyframe b in slot b) -> (fetch results, debug stages)."""
    frames = []  # (holds the device buffers until the fetch)
    for b, p in enumerate(probs):
        t.set_keyframe(b, p["points"], p["state"], p["track_id"])
        d = dict(slot=b, d_features=_dev(p["features"]), d_n1=_dev(np.array([len(p["idx1"])], np.int32)),
                 d_idx0=_dev(p["idx0"]), d_idx1=_dev(p["idx1"]), cam=p["cam"], last_Twc=p["last_Twc"])
        if p["u_right"] is not None:
            d["d_u_right"] = _dev(p["u_right"])
        d.update(kw)
        frames.append(d)
    t.enqueue(frames)
    res = t.fetch()
    return res, [t.debug_stage(b) for b in range(len(probs))]


def _problem(n, state="all", **kw):
    """n keypoints on both sides, all of them mutually matched; state: which partners carry a Good map point"""
    p = SY.track_problem(n0=n, n1=n, n_common=n, frac_no_mappoint=0.0, frac_not_good=0.0, n_non_mutual=0, **kw)
    if state == "none":
        p["state"][:] = np.where(np.arange(n) % 2, 0, 2)
    elif state == "third":  # only every third current keypoint has a valid partner
        p["state"][:] = 2
        i = np.arange(0, n, 3)
        p["state"][p["idx1"][i]] = 1
    return p


def _check_gather(r, d, g):
    np.testing.assert_array_equal(r["match_kf"], g["match_kf"])
    assert (r["n_matches"], r["n_mono"], r["n_stereo"]) == (g["n_matches"], g["n_mono"], g["n_stereo"])
    assert (d["n_corr"], d["n_mono"], d["n_stereo"]) == (len(g["corr_kp"]), g["n_mono"], g["n_stereo"])
    np.testing.assert_array_equal(d["corr_kp"], g["corr_kp"])
    np.testing.assert_array_equal(d["edge_kp"], g["edge_kp"])          # mono before stereo, ascending
    np.testing.assert_array_equal(d["pnp_points"], g["pnp_points"])    # float rounding of the PnP copy
    np.testing.assert_array_equal(d["pnp_keypoints"], g["pnp_keypoints"])
    np.testing.assert_array_equal(d["edges"], g["edges"])              # full doubles


# the scan's seams: empty, one lane, a wave -1 / exact / +1, a chunk -1 / exact / +1, several chunks, the cap
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513, K])
def test_gather_matches_ref(tr, n):
    probs = [_problem(n, s, seed=n + k, stereo_frac=0.4) for k, s in enumerate(("all", "none", "third"))]
    res, dbg = _run(tr, probs)
    for p, r, d, s in zip(probs, res, dbg, ("all", "none", "third")):
        g = TR.gather(p)
        assert r["n_keypoints"] == n
        assert len(g["corr_kp"]) == {"all": n, "none": 0, "third": (n + 2) // 3}[s]
        _check_gather(r, d, g)


def test_gather_mixed_scene(tr):
    """unmatched, non-mutual and out-of-range indices, states 0 / 1 / 2, n0 != n1"""
    p = SY.track_problem(n0=700, n1=600, n_common=450, seed=11, stereo_frac=0.3, n_non_mutual=20)
    (r,), (d,) = _run(tr, [p])
    g = TR.gather(p)
    assert 0 < len(g["corr_kp"]) < g["n_matches"] < 600 and g["n_stereo"] > 0
    _check_gather(r, d, g)


@pytest.mark.parametrize("count", [8, 9, 64, 300])
def test_subsets_match_oracle(tr, count):
    (r,), (d,) = _run(tr, [_problem(count, seed=count)])
    assert d["n_corr"] == count
    np.testing.assert_array_equal(d["subsets"], oracle.pnp_subsets(count, 100))


def test_fewer_than_8_correspondences(tr):
    p = _problem(7, seed=3)
    (r,), (d,) = _run(tr, [p])
    assert d["n_corr"] == 7 and len(d["subsets"]) == 0
    assert (d["pnp_n_inliers"], r["n_pnp_inliers"], r["pnp_used"]) == (0, 0, False)  # SolvePnPWithCV returns 0 (:433)
    _, q, t = TR.seed(0, None, None, p["last_Twc"])
    assert np.abs(d["seed_q"] - q).max() < 1e-12 and np.abs(d["seed_p"] - t).max() < 1e-12


@pytest.mark.parametrize("n,outl,seed", [(300, 0.2, 0), (60, 0.3, 5), (900, 0.3, 3)])
def test_pnp_matches_oracle_and_handle(tr, n, outl, seed):
    p = _problem(n, seed=seed, outlier_frac=outl, pixel_sigma=0.8)
    (r,), (d,) = _run(tr, [p])
    K4 = np.array(p["cam"][:4])
    rn, rR, rt, rinl, rused = oracle.pnp(K4, d["pnp_points"], d["pnp_keypoints"])
    assert rn > 0 and (d["pnp_n_inliers"], d["pnp_hypotheses"]) == (rn, rused)
    np.testing.assert_array_equal(d["pnp_inlier"], rinl)
    assert np.abs(d["pnp_Rwc"] - rR).max() < 1e-9 and np.abs(d["pnp_twc"] - rt).max() < 1e-8
    # rspl_pnp_solve on the same correspondences: the same kernels on the same inputs, bit for bit
    hn, hR, ht, hinl, hused = pkg.PnP(max_batch=1, max_points=K).solve([(K4, d["pnp_points"], d["pnp_keypoints"])])[0]
    assert (hn, hused) == (rn, rused)
    np.testing.assert_array_equal(d["pnp_inlier"], hinl)
    np.testing.assert_array_equal(d["pnp_Rwc"], hR)
    np.testing.assert_array_equal(d["pnp_twc"], ht)


def _check_seed(p, r, d, min_num_match=10):
    used, q, t = TR.seed(d["pnp_n_inliers"], d["pnp_Rwc"], d["pnp_twc"], p["last_Twc"], min_num_match)
    assert (d["pnp_used"], r["pnp_used"]) == (used, used)
    assert np.abs(d["seed_q"] - q).max() < 1e-12 and np.abs(d["seed_p"] - t).max() < 1e-12
    return used


def test_seed_gate_branches(tr):
    p = _problem(200, seed=21)
    (r,), (d,) = _run(tr, [p])
    assert _check_seed(p, r, d)                                   # PnP accepted
    far = dict(p, last_Twc=p["last_Twc"].copy())
    far["last_Twc"][:3, 3] += [0.4, 0.4, 0.0]                     # |twc - t_last| > 0.5 m
    (r,), (d,) = _run(tr, [far])
    assert d["pnp_n_inliers"] >= 10 and not _check_seed(far, r, d)
    (r,), (d,) = _run(tr, [p], min_num_match=1000)                # PnP inliers < min_num_match
    assert 0 < d["pnp_n_inliers"] < 1000 and not _check_seed(p, r, d, 1000)
    few = _problem(7, seed=22)                                    # PnP returned 0
    (r,), (d,) = _run(tr, [few])
    assert d["pnp_n_inliers"] == 0 and not _check_seed(few, r, d)


def _check_frame(r, d, min_num_match):
    """FrameOptimization from the device's own seed pose vs the oracle (tests/test_gpu_frame.py's bounds)"""
    ref = oracle.frame_opt(TR.frame_problem(d, d["seed_q"], d["seed_p"]))
    assert (r["rounds"], r["n_inliers"]) == (ref.rounds, ref.n_inliers)
    assert [i > 0 for i in r["iterations"]] == [i > 0 for i in ref.iterations]
    np.testing.assert_allclose(r["chi2"], ref.chi2, rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(d["edge_inlier"], np.concatenate([ref.inlier["mono"], ref.inlier["stereo"]]))
    assert r["pose_set"] == (ref.n_inliers > min_num_match)
    if r["pose_set"]:
        assert np.abs(r["pose_p"] - ref.pose_p).max() < 1e-9
        s = 1.0 if np.dot(r["pose_q"], ref.pose_q) > 0 else -1.0
        assert np.abs(r["pose_q"] - s * ref.pose_q).max() < 1e-9
    return ref


@pytest.mark.parametrize("n,stereo", [(9, 0.0), (10, 0.0), (300, 0.0), (300, 0.5)])
def test_frame_opt_lds_path(tr512, n, stereo):
    p = _problem(n, seed=30 + n, stereo_frac=stereo, outlier_frac=0.1 if n > 10 else 0.0)
    (r,), (d,) = _run(tr512, [p], min_num_match=3)
    assert d["n_corr"] == n and (d["n_stereo"] > 0) == (stereo > 0)
    ref = _check_frame(r, d, 3)
    assert ref.rounds == (1 if n < 10 else 4) and r["pose_set"]  # optimizer.edges().size() < 10 (:383)


def test_frame_opt_global_path(tr):
    p = _problem(K, "all", seed=40, stereo_frac=0.3, outlier_frac=0.1)
    p["state"][p["idx1"][::3]] = 2  # 682 valid of the 1024 bound
    (r,), (d,) = _run(tr, [p])
    assert d["n_corr"] == K - len(range(0, K, 3)) > 512 and d["n_stereo"] > 0
    _check_frame(r, d, 10)
    assert r["pose_set"]


def _check_write_back(p, r, d, min_num_match):
    g = TR.gather(p)
    pose_set, tid, kept = TR.write_back(g, d["edge_inlier"], r["n_inliers"], min_num_match)
    assert r["pose_set"] == pose_set and r["n_kept"] == int(kept.sum())
    np.testing.assert_array_equal(r["track_id"], tid)
    np.testing.assert_array_equal(r["kept"], kept)
    if not pose_set:  # the pose is the last pose, nothing assigned, nothing removed
        _, q, t = TR.seed(0, None, None, p["last_Twc"])
        assert np.abs(r["pose_q"] - q).max() < 1e-12 and np.abs(r["pose_p"] - t).max() < 1e-12
        assert (r["track_id"] == -1).all() and r["n_kept"] == r["n_matches"]
    return g


def test_write_back(tr):
    p = SY.track_problem(n0=500, n1=450, n_common=350, seed=50, outlier_frac=0.15, stereo_frac=0.3)
    (r,), (d,) = _run(tr, [p])
    g = _check_write_back(p, r, d, 10)
    assert r["pose_set"] and not d["edge_inlier"].all()
    mk = g["match_kf"]
    zero = (mk >= 0) & (p["track_id"][np.maximum(mk, 0)] == 0)
    assert zero.any() and not r["kept"][zero].any()             # track id 0 is dropped (`> 0`, :476)
    edgeless = (mk >= 0) & (p["state"][np.maximum(mk, 0)] != 1) & (p["track_id"][np.maximum(mk, 0)] > 0)
    assert edgeless.any() and r["kept"][edgeless].all()         # never an edge: kept with a positive track id
    # n_inliers == min_num_match is not strictly greater
    n = r["n_inliers"]
    (r2,), (d2,) = _run(tr, [p], min_num_match=n)
    assert r2["n_inliers"] == n and not r2["pose_set"]
    _check_write_back(p, r2, d2, n)


def _check_chain(p, r, min_num_match=10):
    c = TR.chain(p, oracle, min_num_match)
    # the scene is well conditioned: the oracle chain's flags do not move when its seed pose does by 1e-9
    c2 = TR.chain(p, oracle, min_num_match, seed_eps=1e-9)
    np.testing.assert_array_equal(c["flags"], c2["flags"])
    assert c["n_inliers"] == c2["n_inliers"]
    g = c["gather"]
    assert (r["n_keypoints"], r["n_matches"], r["n_mono"], r["n_stereo"]) == \
        (len(p["idx1"]), g["n_matches"], g["n_mono"], g["n_stereo"])
    assert (r["n_pnp_inliers"], r["pnp_used"], r["n_inliers"], r["pose_set"]) == \
        (c["n_pnp_inliers"], c["pnp_used"], c["n_inliers"], c["pose_set"])
    assert r["rounds"] == c["frame"].rounds and r["n_kept"] == int(c["kept"].sum())
    np.testing.assert_array_equal(r["match_kf"], g["match_kf"])
    np.testing.assert_array_equal(r["track_id"], c["track_id"])
    np.testing.assert_array_equal(r["kept"], c["kept"])
    assert np.abs(r["pose_p"] - c["pose_p"]).max() < 1e-9
    s = 1.0 if np.dot(r["pose_q"], c["pose_q"]) > 0 else -1.0
    assert np.abs(r["pose_q"] - s * c["pose_q"]).max() < 1e-9
    return c


E2E = [dict(n0=400, n1=400, n_common=300, seed=60), dict(n0=130, n1=100, n_common=90, seed=61, stereo_frac=0.4),
       dict(n0=900, n1=1000, n_common=800, seed=62, outlier_frac=0.2)]


def test_end_to_end_batch(tr):
    probs = [SY.track_problem(**kw) for kw in E2E]
    res, _ = _run(tr, probs)
    for p, r in zip(probs, res):
        c = _check_chain(p, r)
        assert c["pose_set"] and c["pnp_used"]


def test_track_frame_convenience():
    """MapBuilder::TrackFrame's shape: pose and track ids set in place, the matches filtered"""
    p = SY.track_problem(n0=300, n1=320, n_common=220, seed=70)
    c = TR.chain(p, oracle)
    mk = c["gather"]["match_kf"]
    matches = [(int(j), int(i)) for i, j in enumerate(mk) if j >= 0]
    frame0 = dict(points=p["points"], state=p["state"], track_id=p["track_id"])
    frame1 = dict(features=p["features"].T.copy(), track_id=np.full(320, -1, np.int32), pose=np.eye(4))
    n = pkg.TrackFrame(frame0, frame1, matches, p["cam"], p["last_Twc"])
    assert n == c["n_inliers"] > 10
    np.testing.assert_array_equal(frame1["track_id"], c["track_id"])
    assert matches == [(int(mk[i]), int(i)) for i in np.flatnonzero(c["kept"])]
    assert np.abs(frame1["pose"][:3, 3] - c["pose_p"]).max() < 1e-9
    assert np.abs(frame1["pose"][:3, :3] - SY.quat_xyzw_to_R(c["pose_q"])).max() < 1e-9


def test_re_enqueue_leaks_no_state(tr):
    big = SY.track_problem(n0=900, n1=1000, n_common=800, seed=80, stereo_frac=0.3)
    small = SY.track_problem(n0=90, n1=70, n_common=50, seed=81)
    (rb,), _ = _run(tr, [big])
    (rs,), (ds,) = _run(tr, [small])  # the same slot and buffers, a smaller frame
    _check_chain(big, rb)
    _check_chain(small, rs)
    _check_gather(rs, ds, TR.gather(small))
    fresh = pkg.Tracker(max_batch=1, max_keypoints=K)
    (rf,), _ = _run(fresh, [small])
    for k in ("pose_q", "pose_p", "track_id", "kept", "match_kf", "chi2"):
        np.testing.assert_array_equal(rs[k], rf[k], err_msg=k)


def test_create_destroy_cycle():
    """20 handles of the smallest capacities created and destroyed (device arena, pinned arena, staging, stream,
    events), then one more: its enqueue + fetch and debug stages equal the first handle's bit for bit."""
    from helpers import assert_same, cycle_handle
    p = _problem(8)
    first, last = cycle_handle(lambda: pkg.Tracker(max_batch=1, max_keypoints=8), lambda t: _run(t, [p]))
    assert len(first[1][0]["subsets"]) == 100  # 8 correspondences: PnP ran
    assert_same(first, last)
