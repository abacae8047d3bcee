"""Numpy restatement of what the tracking step does for lines and for the keyframe decision
(rspl_track_enqueue_ext): the line half of MapBuilder::TrackFrame (src/map_builder.cc:450-455, 490-501)
and MapBuilder::AddKeyframe (:616-636) with the _last_frame_track_well flag (:240).  Test infrastructure
only.  AssignPointsToLines and MatchLines themselves are oracle/lines_ref.py's, imported, not restated."""
import math

import numpy as np

import lines_ref as LR

KF_NOT_ENOUGH_MATCH, KF_LARGE_DELTA_ANGLE, KF_LARGE_DISTANCE, KF_ENOUGH_PASSED_FRAME = 1, 2, 4, 8


def point_matches(match_kf):
    """TrackFrame's `matches` before the removal of :472-488: (queryIdx, trainIdx) = (match_kf[i], i)"""
    mk = np.asarray(match_kf)
    i = np.flatnonzero(mk >= 0)
    return np.column_stack([mk[i], i]).astype(np.int64).reshape(-1, 2)


def id_copy(line_matches, kf_track_id, kf_slot, n_lines):
    """:490-501 -- for every keyframe line i with j = line_matches[i] >= 0 and GetLineTrackId(i) >= 0:
    SetLineTrackId(j, id), InsertMapline(j, maplines[i]).  Returns per line of the frame (the keyframe line
    or -1, the track id or -1, the map line or -1)."""
    match_kf = np.full(n_lines, -1, np.int32)
    tid = np.full(n_lines, -1, np.int32)
    slot = np.full(n_lines, -1, np.int32)
    for i, j in enumerate(line_matches):
        if j < 0:
            continue
        match_kf[j] = i
        if kf_track_id[i] >= 0:
            tid[j] = kf_track_id[i]
            slot[j] = kf_slot[i]
    return match_kf, tid, slot


def track_lines(kf_lines, kf_xy, lines, xy, match_kf, n0, n1, kf_track_id, kf_slot, max_pairs=None):
    """The line side for one frame.  kf_xy [n0, 2] / xy [n1, 2]: the keypoints.  Returns the two relations
    (lists of {point: distance}), line_matches per keyframe line, the per-line results and the counts."""
    kf_lines, lines = np.asarray(kf_lines, np.float64).reshape(-1, 4), np.asarray(lines, np.float64).reshape(-1, 4)
    r0 = LR.assign_points_to_lines(kf_lines, np.asarray(kf_xy, np.float64).reshape(-1, 2)[:n0])
    r1 = LR.assign_points_to_lines(lines, np.asarray(xy, np.float64).reshape(-1, 2)[:n1])
    pairs = (sum(len(r) for r in r0), sum(len(r) for r in r1))
    overflow = max_pairs is not None and len(lines) > 0 and (pairs[1] > max_pairs or pairs[0] > max_pairs)
    if overflow or len(lines) == 0:  # no line work, or an assignment that did not fit: every line unmatched
        lm = [-1] * len(kf_lines)
    else:
        lm = LR.match_lines(r0, r1, point_matches(match_kf), n0, n1)
    mk, tid, slot = id_copy(lm, kf_track_id, kf_slot, len(lines))
    return dict(rel_kf=r0, rel=r1, pairs=pairs, line_matches=lm, line_match_kf=mk, line_track_id=tid, line_slot=slot,
                n_line_matches=int((mk >= 0).sum()), n_line_tracks=int((tid >= 0).sum()), overflow=bool(overflow))


def q_to_R(q_xyzw):
    """Eigen's Quaterniond::toRotationMatrix"""
    x, y, z, w = (float(v) for v in q_xyzw)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def R_to_q(m):
    """Eigen's Quaterniond(Matrix3d) (quaternionbase_assign_impl<Other, 3, 3>): (w, x, y, z), not normalised"""
    m = np.asarray(m, np.float64)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = [0.0] * 4
    if t > 0:
        s = math.sqrt(t + 1.0)
        q[0] = 0.5 * s
        s = 0.5 / s
        q[1] = (m[2, 1] - m[1, 2]) * s
        q[2] = (m[0, 2] - m[2, 0]) * s
        q[3] = (m[1, 0] - m[0, 1]) * s
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[1 + i] = 0.5 * s
        s = 0.5 / s
        q[0] = (m[k, j] - m[j, k]) * s
        q[1 + j] = (m[j, i] + m[i, j]) * s
        q[1 + k] = (m[k, i] + m[i, k]) * s
    return np.array(q)


def delta_angle(R_kf, R):
    """Eigen::AngleAxisd(R_kf^T R).angle(): matrix -> quaternion, then 2 atan2(|vec|, |w|), in [0, pi]"""
    q = R_to_q(np.asarray(R_kf, np.float64).T @ np.asarray(R, np.float64))
    n = math.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return 2.0 * math.atan2(n, abs(q[0])) if n != 0 else 0.0


def decision(R, t, n_inliers, kf_Twc, kf_frame_id, frame_id, min_num_match=10, max_num_match=80, max_angle=0.52,
             max_distance=0.5, max_num_passed_frame=300):
    """AddKeyframe (:616-636) for the frame pose (R, t) = T_wc and num_match = n_inliers"""
    kf = np.asarray(kf_Twc, np.float64).reshape(4, 4)
    ang = delta_angle(kf[:3, :3], R)
    d = np.asarray(t, np.float64) - kf[:3, 3]
    dist = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    passed = int(frame_id) - int(kf_frame_id)
    bits = ((KF_NOT_ENOUGH_MATCH if n_inliers < max_num_match else 0) | (KF_LARGE_DELTA_ANGLE if ang > max_angle else 0) |
            (KF_LARGE_DISTANCE if dist > max_distance else 0) | (KF_ENOUGH_PASSED_FRAME if passed > max_num_passed_frame else 0))
    return dict(tracked_well=n_inliers >= min_num_match, add_keyframe=bits, delta_angle=ang, delta_distance=dist,
                passed_frames=passed)


def decision_q(pose_q, pose_p, n_inliers, kf_Twc, kf_frame_id, frame_id, **kw):
    """the same on the pose as rspl_track_result reports it: quaternion (x, y, z, w) and position"""
    return decision(q_to_R(pose_q), pose_p, n_inliers, kf_Twc, kf_frame_id, frame_id, **kw)
