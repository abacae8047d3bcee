"""numpy restatement of the reference's local map tracking -- code it keeps but never calls:
Map::SearchByProjection (src/map.cc:952-1005), Camera::StereoProject (include/camera.h:59-70), Frame::FindGrid /
FindNeighborKeypoints (src/frame.cc:70-78, :324-349), DescriptorDistance (src/utils.cc:14-16),
MapBuilder::UpdateReferenceFrame / UpdateLocalKeyframes / UpdateLocalMappoints / TrackLocalMap
(src/map_builder.cc:684-785).  Scalar Python floats throughout (IEEE doubles, no fused operations), written in
the operation order csrc/lmap_match.hpp fixes, so the library's host and device instantiations can be compared
with it bit for bit.

A frame is a dict: features [n1, 259] (score, x, y, descriptor), u_right [n1] or None (None: a frame without a
right image -- the dxr term is skipped), point_id [n1] (the non-bad map point a keypoint holds, or -1),
point_xyz [n1, 3], Twc [4, 4], cam (fx, fy, cx, cy, bf), width, height.  A local map is a dict: ids [n], pos [n, 3],
desc [n, 256]."""
import math

import numpy as np

NOT_SELECTED, BEHIND, OFF_IMAGE, NO_CANDIDATE, FAILED, GOOD = range(6)
COLS, ROWS = 64, 48
RADIUS, MAX_DISTANCE, MAX_RATIO = 15.0, 0.35, 0.6


# ---- DescriptorDistance with the summation order fixed ---------------------------------------------------------
def distance(a, b):
    """2 (1 - a . b): lane l of 64 owns entries 4l..4l+3, ((a0 b0 + a1 b1) + a2 b2) + a3 b3, the 64 partials by
    the xor butterfly 32, 16, 8, 4, 2, 1.  b may be [m, 256]: one distance per row."""
    a4 = np.asarray(a, np.float64).reshape(64, 4)
    b4 = np.asarray(b, np.float64).reshape(-1, 64, 4)
    p = ((a4[:, 0] * b4[:, :, 0] + a4[:, 1] * b4[:, :, 1]) + a4[:, 2] * b4[:, :, 2]) + a4[:, 3] * b4[:, :, 3]
    o = 32
    while o >= 1:
        p = p[:, :o] + p[:, o:2 * o]
        o //= 2
    d = 2.0 * (1.0 - p[:, 0])
    return d if np.ndim(b) == 2 else float(d[0])


# ---- projection ---------------------------------------------------------------------------------------------
def project(Twc, cam, pw):
    """-> (status, u, v, xr, z): BEHIND / GOOD (the image bounds are the caller's)"""
    T = np.asarray(Twc, np.float64)
    fx, fy, cx, cy, bf = (float(c) for c in cam)
    d0, d1, d2 = (float(pw[k]) - float(T[k, 3]) for k in range(3))
    x = (float(T[0, 0]) * d0 + float(T[1, 0]) * d1) + float(T[2, 0]) * d2
    y = (float(T[0, 1]) * d0 + float(T[1, 1]) * d1) + float(T[2, 1]) * d2
    z = (float(T[0, 2]) * d0 + float(T[1, 2]) * d1) + float(T[2, 2]) * d2
    if not z > 0:
        return BEHIND, 0.0, 0.0, 0.0, z
    z_inv = 1.0 / z
    u = x * z_inv * fx + cx
    v = y * z_inv * fy + cy
    return GOOD, u, v, u - bf * z_inv, z


def in_image(u, v, W, H):
    return 0 < u < W and 0 < v < H


# ---- the grid ---------------------------------------------------------------------------------------------
def c_round(t):
    """std::round: half away from zero"""
    r = math.trunc(t)
    if abs(t - r) >= 0.5:
        r += 1 if t > 0 else -1
    return r


def cell(kx, ky, W, H):
    """Frame::FindGrid"""
    gx = c_round(float(kx) * (COLS / float(W)))
    gy = c_round(float(ky) * (ROWS / float(H)))
    return min(max(0, gx), COLS - 1), min(max(0, gy), ROWS - 1)


def build_grid(fr):
    """Frame::AddLeftFeatures: every keypoint into its cell, in index order"""
    g = {}
    for i, (x, y) in enumerate(fr["features"][:, 1:3]):
        g.setdefault(cell(x, y, fr["width"], fr["height"]), []).append(i)
    return g


def _box(fr, i, u, v, xr, r):
    """the test of FindNeighborKeypoints for keypoint i (cv::KeyPoint holds floats)"""
    if fr["point_id"][i] >= 0:  # filter: _mappoints[idx] && !IsBad()
        return False
    dx = float(np.float32(fr["features"][i, 1])) - u
    dy = float(np.float32(fr["features"][i, 2])) - v
    dxr = float(fr["u_right"][i]) - xr if (fr["u_right"] is not None and xr > 0) else 0.0
    return abs(dx) < r and abs(dy) < r and abs(dxr) < r


def neighbors_walk(fr, grid, u, v, xr, r=RADIUS):
    """Frame::FindNeighborKeypoints(p2D, r, filter = true), literally: the candidates in visiting order"""
    iw, ih = COLS / float(fr["width"]), ROWS / float(fr["height"])
    x0, x1 = max(0, math.floor((u - r) * iw)), min(COLS - 1, math.ceil((u + r) * iw))
    y0, y1 = max(0, math.floor((v - r) * ih)), min(ROWS - 1, math.ceil((v + r) * ih))
    if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
        return []
    out = []
    for gx in range(x0, x1 + 1):
        for gy in range(y0, y1 + 1):
            for i in grid.get((gx, gy), ()):
                if _box(fr, i, u, v, xr, r):
                    out.append(i)
    return out


def neighbors_brute(fr, u, v, xr, r=RADIUS):
    """the same set without the grid, in index order"""
    return [i for i in range(len(fr["features"])) if _box(fr, i, u, v, xr, r)]


# ---- Map::SearchByProjection ---------------------------------------------------------------------------------
def _result(n):
    return dict(status=np.zeros(n, np.int32), best_idx=np.full(n, -1, np.int32), best=np.full(n, 4.0),
                second=np.full(n, 4.0))


def search(fr, lm, r=RADIUS, max_distance=MAX_DISTANCE, max_ratio=MAX_RATIO, tie_rule=False):
    """Per local point: status, best_idx, best, second.  tie_rule False: the reference's loop over the grid walk
    with its strict `<`; True: the candidates in index order with argmin over (dist, gx, gy, idx) -- what the
    library implements."""
    n = len(lm["ids"])
    out = _result(n)
    grid = build_grid(fr)
    held = set(int(i) for i in fr["point_id"] if i >= 0)
    W, H = fr["width"], fr["height"]
    for p in range(n):
        if int(lm["ids"][p]) in held:  # SearchLocalPoints: last_frame_seen == current frame
            out["status"][p] = NOT_SELECTED
            continue
        st, u, v, xr, _ = project(fr["Twc"], fr["cam"], lm["pos"][p])
        if st == GOOD and not in_image(u, v, W, H):
            st = OFF_IMAGE
        if st != GOOD:
            out["status"][p] = st
            continue
        cand = neighbors_walk(fr, grid, u, v, xr, r) if not tie_rule else neighbors_brute(fr, u, v, xr, r)
        if not cand:
            out["status"][p] = NO_CANDIDATE
            continue
        dist = distance(lm["desc"][p], fr["features"][cand, 3:])
        best, second, bi, bkey = 4.0, 4.0, -1, None
        for i, d in zip(cand, dist):
            d = float(d)
            key = cell(fr["features"][i, 1], fr["features"][i, 2], W, H)
            if d < best or (tie_rule and bi >= 0 and d == best and key < bkey):
                second, best, bi, bkey = best, d, i, key
            elif d < second:
                second = d
        out["best_idx"][p], out["best"][p], out["second"][p] = bi, best, second
        out["status"][p] = GOOD if (bi >= 0 and best < max_distance and best < max_ratio * second) else FAILED
    return out


def margins(fr, lm, r=RADIUS, max_distance=MAX_DISTANCE, max_ratio=MAX_RATIO):
    """The smallest distance of any decision of `search` from its threshold: depth, image bounds, the box sides of
    every free keypoint, best against max_distance and max_ratio * second."""
    m = math.inf
    res = search(fr, lm, r, max_distance, max_ratio)
    W, H = fr["width"], fr["height"]
    for p in range(len(lm["ids"])):
        if res["status"][p] == NOT_SELECTED:
            continue
        st, u, v, xr, z = project(fr["Twc"], fr["cam"], lm["pos"][p])
        m = min(m, abs(z))
        if st != GOOD:
            continue
        m = min(m, abs(u), abs(W - u), abs(v), abs(H - v))
        if not in_image(u, v, W, H):
            continue
        for i in range(len(fr["features"])):
            if fr["point_id"][i] >= 0:
                continue
            m = min(m, abs(abs(float(np.float32(fr["features"][i, 1])) - u) - r),
                    abs(abs(float(np.float32(fr["features"][i, 2])) - v) - r))
            if fr["u_right"] is not None:
                m = min(m, abs(xr))
                if xr > 0:
                    m = min(m, abs(abs(float(fr["u_right"][i]) - xr) - r))
        if res["status"][p] in (GOOD, FAILED):
            b, s = float(res["best"][p]), float(res["second"][p])
            m = min(m, abs(b - max_distance), abs(b - max_ratio * s))
    return m


# ---- MapBuilder::TrackLocalMap's merge -------------------------------------------------------------------------
def good_list(res):
    """good_projections: (keypoint, local index) in local order"""
    p = np.flatnonzero(res["status"] == GOOD).astype(np.int32)
    return res["best_idx"][p].astype(np.int32), p


def merge(fr, lm, good_kp, good_point):
    """map_builder.cc:763-768: a good projection fills its keypoint's slot only where the frame holds no non-bad
    point; of several the last in list order wins.  -> (assoc_id [n1], winner [n1]: local index or -1)"""
    n1 = len(fr["features"])
    assoc = np.asarray(fr["point_id"], np.int32).copy()
    winner = np.full(n1, -1, np.int32)
    for kp, p in zip(good_kp, good_point):
        if fr["point_id"][kp] >= 0:
            continue
        assoc[kp] = lm["ids"][p]
        winner[kp] = p
    return assoc, winner


def track_table(fr, lm, winner, K):
    """What the merge writes into the tracker's keyframe slot (n0 = K) and the identity indices it chains with."""
    n1 = len(fr["features"])
    pts, state, tid, idx = np.zeros((K, 3)), np.zeros(K, np.uint8), np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    good = fr.get("point_good")
    for j in range(n1):
        if fr["point_id"][j] >= 0:
            pts[j], tid[j] = fr["point_xyz"][j], fr["point_id"][j]
            state[j] = 1 if good is None or good[j] else 2
        elif winner[j] >= 0:
            pts[j], tid[j], state[j] = lm["pos"][winner[j]], lm["ids"][winner[j]], 1
        if state[j]:
            idx[j] = j
    return pts, state, tid, idx


def track_local_map_gate(n_good, n_inliers, min_num_match, num_inlier_thr):
    """TrackLocalMap's return value from the chain's counts"""
    if n_good < 3:
        return -1
    return n_inliers if (n_inliers > min_num_match and n_inliers > num_inlier_thr) else -1


# ---- local map selection on a plain graph ----------------------------------------------------------------------
# graph: dict(frames = {id: dict(slots = [point id or -1], conn = {frame id: weight})},
#             points = {id: dict(type = 0 untriangulated / 1 good / 2 bad, obs = {frame id: keypoint}, p = [3])})
def reference_keyframe(graph, current_frame_id, point_ids, current_ref):
    votes = {}
    for pid in point_ids:
        q = graph["points"].get(int(pid)) if pid >= 0 else None
        if q is None or q["type"] == 2:
            continue
        for f in q["obs"]:
            if f == current_frame_id or f not in graph["frames"]:
                continue
            votes[f] = votes.get(f, 0) + 1
    best, best_n = current_ref, -1
    for f in sorted(votes):  # ascending frame id stands in for the reference's pointer order
        if votes[f] > best_n:
            best, best_n = f, votes[f]
    return best, best != current_ref


def local_mappoints(graph, ref):
    order = sorted((w, f) for f, w in graph["frames"][ref]["conn"].items())  # GetOrderedConnections(-1)
    ids, seen = [], set()
    for _, f in order:
        for pid in graph["frames"][f]["slots"]:
            q = graph["points"].get(pid) if pid >= 0 else None
            if q is None or q["type"] != 1 or pid in seen:
                continue
            seen.add(pid)
            ids.append(pid)
    pos = np.array([graph["points"][i]["p"] for i in ids], np.float64).reshape(-1, 3)
    return np.array(ids, np.int32), pos
