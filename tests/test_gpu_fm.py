"""The F-matrix RANSAC on the device (rspl_fm_*: cv::findFundamentalMat(FM_RANSAC, 3, 0.99) as
PointMatching::MatchingPoints calls it, src/point_matching.cc:34-45) against the numpy restatement
(tests/fm_ref.py) on scenes whose decisions are checked to sit away from rounding level (tests/fm_cases.py):
the host-fed solve, the per-iteration models and counts, rspl_pm_match's outlier rejection, and the
device-resident chain from SuperGlue's indices to filtered indices, fed on into rspl_track_enqueue."""
import numpy as np
import pytest

import fm_cases as FC
import fm_ref
from conftest import pkg
from rspl_slam_amd import capi, synthetic as SY

pytestmark = pytest.mark.gpu

K = 512


@pytest.fixture(scope="module")
def fm():
    return pkg.FundamentalRansac(max_batch=3, max_matches=K)


def _dev(a):
    a = np.ascontiguousarray(a)
    b = capi.DeviceBuffer(max(a.nbytes, 8))
    if a.nbytes:
        b.upload(a)
    return b


def _same_model(F, Fr):
    return np.abs(fm_ref.normalized(F) - fm_ref.normalized(Fr)).max() <= 1e-9


def _check(got, ref):
    assert (got["n_inliers"], got["hypotheses"]) == (ref["n_inliers"], ref["hypotheses"])
    np.testing.assert_array_equal(got["inlier"], ref["mask"])
    if ref["F"] is None:
        assert np.all(got["F"] == 0)
    else:
        assert _same_model(got["F"], ref["F"])


# 6 ------------------------------------------------------------------------------------------------------------
# n: 7 the direct path; 8, 9 the smallest RANSAC; 63, 64, 65, 257 the ballot and wave seams; 400
# (seeds for which fm_cases.checked_scene's precondition holds)
CASES = [(7, 0.0, 0.0, 1), (8, 0.0, 0.0, 2), (9, 0.0, 0.3, 5), (63, 0.3, 0.0, 1), (64, 0.0, 0.3, 5), (64, 0.6, 0.0, 18),
         (65, 0.3, 0.3, 1), (257, 0.6, 0.3, 1), (257, 0.0, 0.0, 9), (400, 0.3, 0.3, 10), (400, 0.6, 0.0, 77),
         (400, 0.0, 0.3, 12)]
TRUTH = {(63, 1), (64, 18), (257, 9), (400, 77)}  # noise-free scenes on which RANSAC finds exactly the ground truth


@pytest.mark.parametrize("n,outliers,noise,seed", CASES)
def test_solve_equals_fm_ref(fm, n, outliers, noise, seed):
    p0, p1, inl, ref = FC.checked_scene(n, outliers, noise, seed)
    (got,) = fm.solve([(p0, p1)])
    print(f"n={n}: inliers {got['n_inliers']} (fm_ref {ref['n_inliers']}), iterations {got['hypotheses']} "
          f"(fm_ref {ref['hypotheses']})")
    _check(got, ref)
    if n == 7:
        assert np.all(got["inlier"] == 1) and got["hypotheses"] == 1
    elif (n, seed) in TRUTH:
        np.testing.assert_array_equal(got["inlier"].astype(bool), inl)  # and that is the ground truth


@pytest.mark.parametrize("n", [0, 3, 6])
def test_fewer_than_seven_matches_reject_nothing(fm, n):
    p0, p1, _, _ = FC.scene(7, 0.0, 0.0, seed=13)
    (got,) = fm.solve([(p0[:n], p1[:n])])
    assert got["n_inliers"] == -1 and len(got["inlier"]) == n and np.all(got["inlier"] == 1)
    assert np.all(got["F"] == 0)


def test_pure_outliers_run_every_iteration(fm):
    p0, p1 = FC.pure_outliers(32, seed=10)
    ref = fm_ref.find_fundamental(p0, p1, trace=True)
    em, dm = FC.precondition(ref)
    assert em > FC.MARGIN and dm > FC.MARGIN and not ref["order_dependent"]
    assert ref["hypotheses"] == 1000
    (got,) = fm.solve([(p0, p1)])
    _check(got, ref)


# 7 ------------------------------------------------------------------------------------------------------------
def test_batch_equals_single_calls_bit_for_bit(fm):
    probs = [FC.checked_scene(400, 0.3, 0.3, 10)[:2], FC.scene(5, 0.0, 0.0, 15)[:2], FC.checked_scene(65, 0.3, 0.3, 1)[:2]]
    a = fm.solve(probs)
    b = fm.solve(probs)
    singles = [fm.solve([p])[0] for p in probs]
    for x, y, z in zip(a, b, singles):
        for k in ("n_inliers", "hypotheses"):
            assert x[k] == y[k] == z[k]
        for k in ("F", "inlier"):
            assert x[k].tobytes() == y[k].tobytes() == z[k].tobytes()
    assert a[1]["n_inliers"] == -1 and a[0]["n_inliers"] > 0 and a[2]["n_inliers"] > 0


# 8 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,outliers,noise,seed", [(400, 0.3, 0.3, 10), (65, 0.3, 0.3, 1), (9, 0.0, 0.3, 5)])
def test_debug_hypotheses_equal_fm_ref_per_iteration(fm, n, outliers, noise, seed):
    p0, p1, _, _ = FC.scene(n, outliers, noise, seed)
    fm.solve([(p0, p1)])
    nm, cnt, F = fm.debug_hypotheses(0, 1000)
    sub, _, _ = fm_ref.subsets(n, 200, p0, p1)
    assert len(nm) == 1000
    thr = np.float32(9.0)
    skipped, worst = 0, 0.0
    for h, idx in enumerate(sub):
        want, rel = fm_ref.seven_point(p0[idx], p1[idx])
        e_ref = [fm_ref.errors_f64(w, p0, p1) for w in want]
        margin = min([np.abs(e - 9.0).min() / 9.0 for e in e_ref] + [np.inf])
        if (rel is not None and rel <= FC.MARGIN) or margin <= FC.MARGIN:
            skipped += 1
            continue
        assert nm[h] == len(want)
        left = list(range(nm[h]))
        for w, e in zip(want, e_ref):  # the order of an iteration's models follows the null-space basis
            d = [np.abs(fm_ref.normalized(F[h, k]) - fm_ref.normalized(w)).max() for k in left]
            k = left.pop(int(np.argmin(d)))
            assert min(d) <= 1e-9
            assert cnt[h, k] == int(np.count_nonzero(e.astype(np.float32) <= thr))
            ed = fm_ref.errors_f64(F[h, k], p0, p1)
            near = (e > 0.09) & (e < 900.0)  # within a factor 100 of the threshold: where a difference can decide
            if near.any():
                worst = max(worst, float((np.abs(ed[near] - e[near]) / e[near]).max()))
    print(f"n={n}: largest relative error difference device vs fm_ref {worst:.3g} (margin {FC.MARGIN:.3g}), "
          f"skipped {skipped} of {len(sub)}")
    assert skipped <= 2  # at most 1 %
    assert worst <= FC.MEASURED_REL_ERR  # the measurement fm_cases.MARGIN is 100 x of: it must stay an upper bound


# 9 ------------------------------------------------------------------------------------------------------------
def _expected_filtered(fm, F0, F1, matches):
    p0 = np.array([F0[1:3, q] for q, _, _ in matches]).reshape(-1, 2)
    p1 = np.array([F1[1:3, t] for _, t, _ in matches]).reshape(-1, 2)
    (r,) = fm.solve([(p0, p1)])
    return [m for m, keep in zip(matches, r["inlier"]) if keep], r


@pytest.mark.parametrize("name", ["sg_small", "sg_c1"])
def test_pm_match_outlier_rejection(fm, golden, weight_blobs, sg_c1_blob, name):
    g = golden(name)
    F0, F1 = g["F0"].astype(np.float64), g["F1"].astype(np.float64)
    blob = sg_c1_blob if name == "sg_c1" else weight_blobs[1]
    pm = pkg.PointMatching(pkg.SuperGlueConfig(image_width=752, image_height=480, weights=blob, max_keypoints=400,
                                               max_batch=1, precision=pkg.capi.RSPL_PREC_FP32))
    n, plain = pm.MatchingPoints(F0, F1, False)
    assert n == len(g["matches"])
    np.testing.assert_array_equal(np.array([(q, t) for q, t, _ in plain]), g["matches"])
    want, r = _expected_filtered(fm, F0, F1, plain)
    nf, filtered = pm.MatchingPoints(F0, F1, True)
    print(f"{name}: {n} matches, {nf} after the outlier rejection ({r['hypotheses']} iterations)")
    assert nf == len(want) == (r["n_inliers"] if r["n_inliers"] >= 0 else n)
    assert filtered == want
    n2, again = pm.MatchingPoints(F0, F1, False)  # and the plain path is untouched by the handle created meanwhile
    assert again == plain


# 10 -----------------------------------------------------------------------------------------------------------
def _chain_case(nk, outliers, seed):
    """nk keypoints in both images: the matches of a scene scattered over them and, from 16 keypoints on, six
    keypoints that are unmatched, not mutual or point past n1.  Returns the SuperPoint records, idx0 / idx1 and
    the matches in DMatch order."""
    rng = np.random.default_rng(1000 + seed)
    pad = 6 if nk >= 16 else 0
    n = nk - pad
    p0, p1, _, _ = FC.scene(max(n, 1), outliers, 0.3, seed)
    n0, n1 = nk, nk
    perm0, perm1 = rng.permutation(n0), rng.permutation(n1)
    idx0, idx1 = np.full(n0, -1, np.int32), np.full(n1, -1, np.int32)
    pts0 = rng.uniform(10, 400, (n0, 2))
    pts1 = rng.uniform(10, 400, (n1, 2))
    for m in range(n):
        i, j = perm0[m], perm1[m]
        idx0[i], idx1[j] = j, i
        pts0[i], pts1[j] = p0[m], p1[m]
    if pad >= 6:
        a, b, c = perm0[n:n + 3]
        x, y, z = perm1[n:n + 3]
        idx0[a], idx1[x] = x, b      # not mutual: x points at another keypoint
        idx0[b] = n1 + 5             # past n1
        idx1[y] = perm0[0]           # a second claim on a matched keypoint: not mutual from y's side
    order = [i for i in range(n0) if idx0[i] >= 0 and idx0[i] < n1 and idx1[idx0[i]] == i]
    assert len(order) == n
    mp0 = pts0[order]
    mp1 = pts1[[idx0[i] for i in order]]
    return dict(rec0=FC.superpoint_records(pts0, n0, rng), rec1=FC.superpoint_records(pts1, n1, rng), idx0=idx0,
                idx1=idx1, n0=n0, n1=n1, order=order, mp0=mp0, mp1=mp1)


def _enqueue(fm, cases):
    frames, keep = [], []
    for c in cases:
        o0, o1 = _dev(np.full(c["n0"], 77, np.int32)), _dev(np.full(c["n1"], 77, np.int32))
        d = dict(d_features0=_dev(c["rec0"]), d_n0=_dev(np.array([c["n0"]], np.int32)), d_features1=_dev(c["rec1"]),
                 d_n1=_dev(np.array([c["n1"]], np.int32)), d_idx0=_dev(c["idx0"]), d_idx1=_dev(c["idx1"]),
                 d_idx0_out=o0, d_idx1_out=o1)
        frames.append(d)
        keep.append((o0, o1))
    fm.enqueue(frames)
    res = fm.fetch()
    outs = [(o0.download((c["n0"],), np.int32), o1.download((c["n1"],), np.int32)) for (o0, o1), c in zip(keep, cases)]
    return res, outs, frames


def _check_chain(fm, c, got, out):
    (want,) = fm.solve([(c["mp0"], c["mp1"])])
    assert (got["n_inliers"], got["hypotheses"]) == (want["n_inliers"], want["hypotheses"])
    np.testing.assert_array_equal(got["inlier"], want["inlier"])
    assert got["F"].tobytes() == want["F"].tobytes()
    e0, e1 = c["idx0"].copy(), c["idx1"].copy()
    for keep, i in zip(want["inlier"], c["order"]):
        if not keep:
            e1[e0[i]] = -1
            e0[i] = -1
    np.testing.assert_array_equal(out[0], e0)
    np.testing.assert_array_equal(out[1], e1)
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 400, K])
def test_device_chain_equals_solve(fm, n):
    c = _chain_case(n, 0.3 if n >= 63 else 0.0, seed=n)
    (got,), (out,), _ = _enqueue(fm, [c])
    want = _check_chain(fm, c, got, out)
    if n >= 63:
        assert 0 < want["n_inliers"] < n - 6  # something is rejected
    else:
        assert want["n_inliers"] == -1
        np.testing.assert_array_equal(out[0], c["idx0"])  # fewer than 7 matches: plain copies
        np.testing.assert_array_equal(out[1], c["idx1"])


def test_device_chain_batch_and_seven(fm):
    cases = [_chain_case(263, 0.6, seed=31), _chain_case(6, 0.0, seed=32), _chain_case(7, 0.0, seed=33)]
    res, outs, _ = _enqueue(fm, cases)
    for c, got, out in zip(cases, res, outs):
        _check_chain(fm, c, got, out)
    assert res[1]["n_inliers"] == -1 and res[2]["n_inliers"] == 7 and np.all(res[2]["inlier"] == 1)


def test_filtered_indices_feed_the_tracker(fm):
    n = 300
    p = SY.track_problem(n0=n, n1=n, n_common=n, frac_no_mappoint=0.0, frac_not_good=0.0, n_non_mutual=0, seed=41)
    q0, q1, _, _ = FC.scene(n, 0.3, 0.3, seed=41)
    rng = np.random.default_rng(41)
    feat1 = np.array(p["features"], np.float64).reshape(-1, 259).copy()
    pts0 = np.zeros((n, 2))
    order = [i for i in range(n) if p["idx0"][i] >= 0 and p["idx1"][p["idx0"][i]] == i]
    assert len(order) == n
    for m, i in enumerate(order):  # keyframe keypoint i <-> current keypoint idx0[i] carry scene pair m
        pts0[i] = q0[m]
        feat1[p["idx0"][i], 1:3] = q1[m]
    feat0 = FC.superpoint_records(pts0, n, rng)
    o0, o1 = _dev(np.zeros(n, np.int32)), _dev(np.zeros(n, np.int32))
    d_feat1, d_n1 = _dev(feat1), _dev(np.array([n], np.int32))
    frame = dict(d_features0=_dev(feat0), d_n0=_dev(np.array([n], np.int32)), d_features1=d_feat1, d_n1=d_n1,
                 d_idx0=_dev(np.asarray(p["idx0"], np.int32)), d_idx1=_dev(np.asarray(p["idx1"], np.int32)),
                 d_idx0_out=o0, d_idx1_out=o1)
    fm.enqueue([frame])
    (r,) = fm.fetch()
    assert 0 < r["n_inliers"] < n
    tr = pkg.Tracker(max_batch=1, max_keypoints=K)
    tr.set_keyframe(0, p["points"], p["state"], p["track_id"])
    tr.enqueue([dict(slot=0, d_features=d_feat1, d_n1=d_n1, d_idx0=o0, d_idx1=o1, cam=p["cam"],
                     last_Twc=p["last_Twc"])])
    (t,) = tr.fetch()
    assert t["n_matches"] == r["n_inliers"]


def test_create_destroy_cycle():
    """20 handles of the smallest capacities created and destroyed (device arena, pinned arena, stream, event),
    then one more: its host-fed solve and its device-resident chain equal the first handle's bit for bit."""
    from helpers import assert_same, cycle_handle
    p0, p1, _, _ = FC.checked_scene(8, 0.0, 0.0, 2)
    c = _chain_case(8, 0.0, seed=8)

    def run(h):
        solved = h.solve([(p0, p1)])
        res, outs, _ = _enqueue(h, [c])
        return solved, res, outs

    first, last = cycle_handle(lambda: pkg.FundamentalRansac(max_batch=1, max_matches=8), run)
    assert first[0][0]["n_inliers"] > 0 and first[1][0]["n_inliers"] > 0
    assert_same(first, last)
