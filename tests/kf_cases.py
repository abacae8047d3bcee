"""Shared cases and checks of the keyframe-insertion tests (tests/test_keyframe_cpu.py on the host
instantiation and the native map without a device, tests/test_gpu_keyframe.py on the device): the
triangulation batch with its special cases, the position bound, the map comparison.  The reference is
tests/kf_ref.py."""
import numpy as np

import kf_ref as KR
import map_ref

CAM = (435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297, 47.90639384423901)


def _rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _project(T, X):
    Xc = T[:3, :3].T @ (X - T[:3, 3])
    return np.array([CAM[0] * Xc[0] / Xc[2] + CAM[2], CAM[1] * Xc[1] / Xc[2] + CAM[3]])


def _two_view(baseline, depth=8.0):
    """one point seen from two parallel cameras `baseline` apart"""
    poses = [_pose(np.eye(3), [0, 0, 0]), _pose(np.eye(3), [baseline, 0, 0])]
    X = np.array([0.3, -0.2, depth])
    return poses, [0, 1], [_project(T, X) for T in poses]


def _baseline_for_ratio(target):
    """the baseline at which the restatement's pivot ratio is `target` (the ratio grows with the baseline)"""
    lo, hi = 1e-6, 10.0
    for _ in range(200):
        mid = np.sqrt(lo * hi)
        poses, op, xy = _two_view(mid)
        if KR.triangulate_point(poses, op, xy, CAM)[2] < target:
            lo = mid
        else:
            hi = mid
    return hi


def tri_cases():
    """(poses, CSR) of 300 random points with 2-12 observers -- a few observers skipped -- and the special
    cases; built once"""
    rng = np.random.default_rng(5)
    poses = [_pose(_rot(rng.normal(0, 0.05, 3)), np.array([0.3 * k, 0.0, 0.1 * k]) + rng.normal(0, 0.1, 3)) for k in range(16)]
    off, op, xy, names = [0], [], [], []

    def add(name, obs):
        for f, px in obs:
            op.append(f)
            xy.append(px)
        off.append(len(op))
        names.append(name)

    for i in range(300):
        n = int(rng.integers(2, 13))
        X = np.array([rng.uniform(-4, 4), rng.uniform(-2, 2), rng.uniform(3, 25)])
        fs = np.sort(rng.choice(16, n, replace=False))
        obs = [(int(f), _project(poses[f], X) + rng.normal(0, 0.5, 2)) for f in fs]
        if i % 7 == 0 and n > 3:      # an observer whose frame is not in the map
            obs[1] = (-1, obs[1][1])
        add("random", obs)
    X = np.array([0.5, 0.2, 9.0])
    add("one valid observer", [(-1, _project(poses[0], X)), (3, _project(poses[3], X)), (-1, _project(poses[5], X))])
    add("no observer", [])
    # identical bearings from distinct centres: rank 2
    base = len(poses)
    poses += [_pose(np.eye(3), [0, 0, 0]), _pose(np.eye(3), [1.0, 0.5, 0]), _pose(np.eye(3), [-0.7, 0.2, 0.1])]
    add("identical bearings", [(base + k, np.array([400.0, 260.0])) for k in range(3)])
    # the pivot ratio just below and just above the threshold, by scaling the baseline
    for target in (0.5e-5, 2e-5):
        ps, _, px = _two_view(_baseline_for_ratio(target))
        b = len(poses)
        poses += ps
        add(f"ratio {target:g}", [(b, px[0]), (b + 1, px[1])])
    return (np.array(poses), np.array(off, np.int32), np.array(op, np.int32), np.array(xy).reshape(-1, 2), names)


def check_triangulation(case, ref, ref_rev, pos, st):
    """rank decisions equal on every case, none of them near the threshold; positions within the bound"""
    poses, off, op, xy, names = case
    rp, rs, ratio, As, nv = ref
    assert len(st) == len(names) == len(rs)
    # no case may be excused: none is near the threshold
    assert (np.abs(ratio / KR.RANK_TOL - 1.0) > 1e-8).all()
    np.testing.assert_array_equal(st, rs)
    for i in range(len(names)):
        if rs[i] != KR.TRI_OK:
            assert not pos[i].any()
            continue
        bound = KR.position_bound(As[i], nv[i], rp[i])
        # the restatement's own spread between ascending and descending observer order: the bound is not too tight
        spread = np.linalg.norm(ref_rev[0][i] - rp[i])
        assert ref_rev[1][i] == KR.TRI_OK and spread <= bound / 4, (i, names[i], spread, bound)
        err = np.linalg.norm(pos[i] - rp[i])
        assert err <= bound, (i, names[i], err, bound)


def compare_maps(m, mr, seq_keyframes, tri_bounds, exact_lines=True):
    """landmark ids, types, observers and frame slots identical; triangulated positions within their bound,
    everything else exact; lines: ids, types, observers with their endpoint status, fit and endpoints"""
    for pid, q in mr.mappoints.items():
        p, t, obs = m.GetMappoint(pid)
        assert t == q.type and obs == q.obs, pid
        if pid in tri_bounds:
            assert np.linalg.norm(p - q.p) <= tri_bounds[pid], pid
        else:
            np.testing.assert_array_equal(p, q.p)
    for lid, l in mr.maplines.items():
        L, t, n, ep, valid = m.GetMapline(lid)
        assert (t, n, valid) == (l.type, len(l.obs), l.endpoints_valid), lid
        assert m.GetMaplineObservers(lid) == [(f, l.obs[f], l.incl.get(f, -1)) for f in sorted(l.obs)], lid
        if exact_lines:
            np.testing.assert_array_equal(L, l.L)
            np.testing.assert_array_equal(ep, l.endpoints)
    for f in seq_keyframes:
        a, b = m.FrameSlots(f["id"])
        fr = mr.keyframes[f["id"]]
        assert list(a) == [-1 if q is None else q.id for q in fr.mappoints]
        assert list(b) == [-1 if l is None else l.id for l in fr.maplines]


def ref_stage(seq, f, k, mr, next_tid):
    """the stereo stage of raw keyframe f by the restatement, with the held points' positions from the oracle map"""
    n = len(f["feat_left"])
    pts, state = np.zeros((n, 3)), np.zeros(n, np.uint8)
    for i in np.flatnonzero(f["point_slot"] >= 0):
        q = mr.mappoints[int(f["point_slot"][i])]
        pts[i], state[i] = q.p, 1 if q.type == map_ref.GOOD else 2
    p = dict(f, points=pts, state=state, cam=seq["camera"], window=seq["window"], next_track_id=next_tid)
    return KR.stereo(p, init=k == 0)
