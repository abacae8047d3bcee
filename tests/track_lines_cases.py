"""Seeded inputs of the tracking step's line side (tests/test_gpu_track_lines.py, tools/bench_track_lines.py):
synthetic.line_scene's stereo frame read as keyframe (left) and current frame (right), with a
synthetic.track_problem-style keyframe table behind it so that the pose chain has something to solve."""
import numpy as np

from rspl_slam_amd import synthetic as SY


def _exact_lines(n_lines, n_pts, seed):
    """a line_scene with at least n_lines lines (it drops segments the image clips short)"""
    want = max(n_lines, 1)
    while True:
        sc = SY.line_scene(n_lines=want, n_points=max(n_pts, 1), seed=seed)
        if len(sc["lines_left"]) >= n_lines:
            return sc
        want += 1


def line_case(n_lines, n_pts, seed=3, n_kf_lines=None):
    """One frame: the keyframe's lines / keypoints (left image), the frame's (right image), SuperGlue-style
    indices from the scene's stereo matches (a few wrong: not all mutual), a keyframe table whose world
    points project onto their partners from a ground-truth pose, and per keyframe line a track id (0 and -1
    among them) and a map-line id (-1 among them)."""
    sc = _exact_lines(max(n_lines, n_kf_lines or 0), n_pts, seed)
    rng = np.random.default_rng(1000 + seed)
    nk = n_lines if n_kf_lines is None else n_kf_lines
    L0, L1 = sc["lines_left"][:nk].copy(), sc["lines_right"][:n_lines].copy()
    F0, F1, m = sc["feat_left"][:n_pts].copy(), sc["feat_right"][:n_pts].copy(), sc["stereo_matches"]
    m = m[(m[:, 0] < n_pts) & (m[:, 1] < n_pts)]
    idx0, idx1 = np.full(n_pts, -1, np.int32), np.full(n_pts, -1, np.int32)
    idx0[m[:, 0]] = m[:, 1]
    idx1[m[:, 1]] = m[:, 0]  # a right keypoint two left ones claim keeps the last: the other is not mutual
    fx, fy, cx, cy, bf = cam = (SY.EUROC_FX, SY.EUROC_FY, SY.EUROC_CX, SY.EUROC_CY, SY.EUROC_BF)
    Rwc, twc = SY._rotvec_to_R(rng.normal(0, 0.1, 3)), rng.normal(0, 1.0, 3)
    z = rng.uniform(1.5, 20.0, n_pts)
    uv = F0[:, 1:3].copy()
    has = idx0 >= 0
    uv[has] = F1[idx0[has], 1:3] + rng.normal(0, 0.3, (int(has.sum()), 2))
    X = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1) @ Rwc.T + twc
    last = SY._Twc(SY._rotvec_to_R(rng.normal(0, 0.01, 3)) @ Rwc, twc + rng.normal(0, 0.05, 3))
    k = np.arange(nk)
    return dict(kf_lines=L0, lines=L1, kf_features=F0, features=F1, idx0=idx0, idx1=idx1,
                points=X.reshape(-1, 3), state=np.ones(n_pts, np.uint8), track_id=np.arange(1, n_pts + 1, dtype=np.int32),
                u_right=None, cam=tuple(float(c) for c in cam), last_Twc=last,
                kf_line_track_id=np.where(k % 5 == 3, -1, k).astype(np.int32),
                kf_line_slot=np.where(k % 4 == 1, -1, 100 + k).astype(np.int32),
                kf_Twc=SY._Twc(Rwc @ SY._rotvec_to_R(np.array([0.03, -0.04, 0.02])), twc + [0.2, 0.0, 0.1]),
                kf_frame_id=40, frame_id=47)


def hand_case():
    """Hand-built count matrices: horizontal lines 60 px apart, keypoints on them 20 px apart, keyframe
    keypoint i matched to frame keypoint i wherever `matched` says so.
      keyframe lines  A (5 points, all matched)  A again        C (5 points, 2 matched)  D (5 points, 1 matched)  E
      frame lines     A  A again                 C (6 points)   D                        E E again
    A: the duplicated keyframe line ties two rows (the first wins), the duplicated frame line two columns.
    C: v = 2, min(5, 6) = 5: the score is exactly 0.8f, accepted.  D: v = 1, rejected.
    E: the keyframe's line sees 4 matched points and both copies of the frame's line tie for its row."""
    def line(y, x0=100.0, x1=300.0):
        return [x0, y, x1, y]

    def pts(y, n, x0=100.0):
        return [[x0 + 20.0 * i, y] for i in range(n)]

    kf_xy = pts(60, 5) + pts(120, 5) + pts(180, 5) + pts(240, 4)
    xy = pts(60, 5) + pts(120, 5) + pts(180, 5) + pts(240, 4) + [[290.0, 120.0]]  # a 6th point on the frame's C
    matched = [1] * 5 + [1, 1, 0, 0, 0] + [1, 0, 0, 0, 0] + [1] * 4
    n0, n1 = len(kf_xy), len(xy)
    idx0, idx1 = np.full(n0, -1, np.int32), np.full(n1, -1, np.int32)
    for i, on in enumerate(matched):
        if on:
            idx0[i] = idx1[i] = i
    F0, F1 = np.zeros((n0, 259)), np.zeros((n1, 259))
    F0[:, 1:3], F1[:, 1:3] = kf_xy, xy
    kf_lines = np.array([line(60), line(60), line(120), line(180), line(240)])
    lines = np.array([line(60), line(60), line(120), line(180), line(240), line(240)])
    rng = np.random.default_rng(5)
    return dict(kf_lines=kf_lines, lines=lines, kf_features=F0, features=F1, idx0=idx0, idx1=idx1,
                points=rng.normal(0, 1, (n0, 3)) + [0, 0, 5], state=np.ones(n0, np.uint8),
                track_id=np.arange(1, n0 + 1, dtype=np.int32), u_right=None,
                cam=(SY.EUROC_FX, SY.EUROC_FY, SY.EUROC_CX, SY.EUROC_CY, SY.EUROC_BF), last_Twc=np.eye(4),
                kf_line_track_id=np.array([0, 7, 8, 9, -1], np.int32), kf_line_slot=np.array([-1, 21, 22, 23, 24], np.int32),
                kf_Twc=np.eye(4), kf_frame_id=3, frame_id=4,
                expect=dict(line_match_kf=[0, -1, 2, -1, 4, -1], line_track_id=[0, -1, 8, -1, -1, -1],
                            line_slot=[-1, -1, 22, -1, -1, -1]))
