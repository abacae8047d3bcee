"""Plain Python / numpy restatement of keyframe insertion, the reference for csrc/kf_kernels.hip,
csrc/kf_triangulate.hpp and rspl_map_insert_keyframe (csrc/map.cpp):

  MapBuilder::InsertKeyframe / Init's ids   src/map_builder.cc:639-682, :390-403
  Frame::AddRightFeatures                   src/frame.cc:150-177
  Map::InsertKeyframe                       src/map.cc:24-103
  Map::TriangulateMappoint                  src/map.cc:292-339
  Map::TriangulateMaplineByMappoints        src/map.cc:341-419

Scalar fp64 (Python floats) in the order the C++ states its operations; float32 (numpy scalars) for the line
fit.  The map structures are oracle/map_ref.py's."""
import math

import numpy as np

import map_ref

F32 = np.float32
RANK_TOL = 1e-5
TRI_FEW, TRI_OK, TRI_RANK = 0, 1, 2


# ------------------------------------------------------------------------------------------------
# the stereo stage
# ------------------------------------------------------------------------------------------------
def mutual(idx0, idx1, n_right):
    """point_matching.cc:24-31 from the left side: partner of left keypoint i or -1"""
    out = np.full(len(idx0), -1, np.int64)
    for i, j in enumerate(idx0):
        if 0 <= j < n_right and idx1[j] == i:
            out[i] = j
    return out


def stereo(p, init=False, n_left=None, n_right=None):
    """The stereo stage on a synthetic.keyframe_problem-shaped dict.  Returns the per-keypoint arrays, the
    counts and the tracker table (points, state, track id) the device fills."""
    FL, FR = p["feat_left"], p["feat_right"]
    nl = len(FL) if n_left is None else n_left
    nr = len(FR) if n_right is None else n_right
    fx, fy, cx, cy, bf = [float(c) for c in p["cam"]]
    mn, mx, my = [float(w) for w in p["window"]]
    T = np.asarray(p["Twc"], np.float64).reshape(4, 4)
    R = [[float(T[r, c]) for c in range(3)] for r in range(3)]
    t = [float(T[r, 3]) for r in range(3)]
    fx_inv, fy_inv = 1.0 / fx, 1.0 / fy
    part = mutual(p["idx0"][:nl], p["idx1"], nr)
    u_right, depth = np.full(nl, -1.0), np.full(nl, -1.0)
    n_matches = n_kept = 0
    for i in range(nl):
        j = part[i]
        if j < 0:
            continue
        n_matches += 1
        xl, yl, xr, yr = float(FL[i, 1]), float(FL[i, 2]), float(FR[j, 1]), float(FR[j, 2])
        dx, dy = abs(xl - xr), abs(yl - yr)
        if dx > mn and dx < mx and dy <= my:   # frame.cc:164: strict in x, inclusive in y
            n_kept += 1
            u_right[i] = xr
            depth[i] = bf / (xl - xr)          # the signed difference (:176)
    tid_in = np.full(nl, -1, np.int64)
    if not init and p.get("track_id") is not None:
        tid_in[:] = p["track_id"][:nl]
    slot = np.full(nl, -1, np.int64)
    if p.get("point_slot") is not None:
        slot[:] = p["point_slot"][:nl]
    track_id = tid_in.copy()
    nxt = int(p["next_track_id"])
    if init:   # MapBuilder::Init (:390-403): the keypoints with a depth, then InsertKeyframe's loop over the rest
        for i in range(nl):
            if depth[i] > 0:
                track_id[i] = nxt
                nxt += 1
    for i in range(nl):   # map_builder.cc:660-665
        if track_id[i] < 0:
            track_id[i] = nxt
            nxt += 1
    new_point, new_position = np.zeros(nl, np.uint8), np.zeros((nl, 3))
    tbl_p, tbl_s = np.zeros((nl, 3)), np.zeros(nl, np.uint8)
    for i in range(nl):
        if slot[i] >= 0:
            tbl_p[i], tbl_s[i] = p["points"][i], p["state"][i]
            continue
        if track_id[i] < 0:
            continue
        if depth[i] > 0:   # Frame::BackProjectPoint (:313), Camera::BackProjectStereo, map.cc:50
            x, y, ur = float(FL[i, 1]), float(FL[i, 2]), float(u_right[i])
            d = bf / (x - ur)
            pf = [((x - cx) * fx_inv) * d, ((y - cy) * fy_inv) * d, 1.0 * d]
            new_position[i] = [(R[r][0] * pf[0] + R[r][1] * pf[1] + R[r][2] * pf[2]) + t[r] for r in range(3)]
            new_point[i] = 1
            tbl_p[i], tbl_s[i] = new_position[i], 1
        elif not init:
            new_point[i] = 2
            tbl_s[i] = 2
    return dict(n_keypoints=nl, n_matches=n_matches, n_stereo_matches=n_kept, n_new_ids=nxt - int(p["next_track_id"]),
                n_new_points=int((new_point != 0).sum()), n_new_good=int((new_point == 1).sum()), next_track_id=nxt,
                u_right=u_right, depth=depth, track_id=track_id.astype(np.int32), new_point=new_point,
                new_position=new_position, table=(tbl_p, tbl_s, track_id.astype(np.int32)))


# ------------------------------------------------------------------------------------------------
# Map::TriangulateMappoint
# ------------------------------------------------------------------------------------------------
def _householder(A, y, K):
    c0 = A[K][K]
    tail2 = 0.0
    for r in range(K + 1, 3):
        tail2 = tail2 + A[r][K] * A[r][K]
    if not tail2 > 2.2250738585072014e-308:
        return c0
    beta = math.sqrt(c0 * c0 + tail2)
    if c0 >= 0.0:
        beta = -beta
    den, tau = c0 - beta, (beta - c0) / beta
    v = [0.0, 0.0, 0.0]
    for r in range(K + 1, 3):
        v[r] = A[r][K] / den
    for c in range(K + 1, 3):
        s = A[K][c]
        for r in range(K + 1, 3):
            s = s + v[r] * A[r][c]
        ts = tau * s
        A[K][c] = A[K][c] - ts
        for r in range(K + 1, 3):
            A[r][c] = A[r][c] - v[r] * ts
    s = y[K]
    for r in range(K + 1, 3):
        s = s + v[r] * y[r]
    ts = tau * s
    y[K] = y[K] - ts
    for r in range(K + 1, 3):
        y[r] = y[r] - v[r] * ts
    return beta


def _swap_cols(A, perm, p, q):
    for r in range(3):
        A[r][p], A[r][q] = A[r][q], A[r][p]
    perm[p], perm[q] = perm[q], perm[p]


def solve3_colpiv(A, y):
    """Column-pivoted Householder QR of a 3x3 (Eigen::ColPivHouseholderQR, threshold 1e-5).
    Returns (status, x, min |R_ii| / max |R_ii|)."""
    A, y, perm = [list(r) for r in A], list(y), [0, 1, 2]
    n = [math.sqrt(A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c]) for c in range(3)]
    if n[1] > n[0] and not n[2] > n[1]:
        _swap_cols(A, perm, 0, 1)
    elif n[2] > n[0] and n[2] > n[1]:
        _swap_cols(A, perm, 0, 2)
    r0 = _householder(A, y, 0)
    n1 = math.sqrt(A[1][1] * A[1][1] + A[2][1] * A[2][1])
    n2 = math.sqrt(A[1][2] * A[1][2] + A[2][2] * A[2][2])
    if n2 > n1:
        _swap_cols(A, perm, 1, 2)
    r1 = _householder(A, y, 1)
    r2 = A[2][2]
    a = [abs(r0), abs(r1), abs(r2)]
    mx, mn = max(a), min(a)
    ratio = mn / mx if mx > 0.0 else 0.0
    thr = mx * RANK_TOL
    if sum(v > thr for v in a) < 3:
        return TRI_RANK, [0.0, 0.0, 0.0], ratio
    z2 = y[2] / r2
    z1 = (y[1] - A[1][2] * z2) / r1
    z0 = (y[0] - A[0][1] * z1 - A[0][2] * z2) / r0
    x = [0.0, 0.0, 0.0]
    for j, z in zip(perm, (z0, z1, z2)):
        x[j] = z
    return TRI_OK, x, ratio


def triangulate_point(Twc, obs_pose, obs_xy, cam, reverse=False):
    """One map point.  Returns (status, position [3], pivot ratio, AxtAx [3, 3], valid observers)."""
    fx_inv, fy_inv, cx, cy = 1.0 / float(cam[0]), 1.0 / float(cam[1]), float(cam[2]), float(cam[3])
    S = [[0.0] * 3 for _ in range(3)]
    sc, sb = [0.0] * 3, [0.0] * 3
    n = 0
    ks = range(len(obs_pose) - 1, -1, -1) if reverse else range(len(obs_pose))
    for k in ks:
        f = int(obs_pose[k])
        if f < 0:
            continue
        T = Twc[f]
        u, v = (float(obs_xy[k][0]) - cx) * fx_inv, (float(obs_xy[k][1]) - cy) * fy_inv
        b = [float(T[r][0]) * u + float(T[r][1]) * v + float(T[r][2]) * 1.0 for r in range(3)]
        c = [float(T[r][3]) for r in range(3)]
        inv = 1.0 / (b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
        bc = b[0] * c[0] + b[1] * c[1] + b[2] * c[2]
        d = [b[r] * inv for r in range(3)]
        for r in range(3):
            sc[r] = sc[r] + c[r]
            sb[r] = sb[r] + d[r] * bc
        for r in range(3):
            for q in range(3):
                S[r][q] = S[r][q] + d[r] * b[q]
        n += 1
    if n < 2:
        return TRI_FEW, np.zeros(3), 0.0, None, n
    A = [[(float(n) if r == q else 0.0) - S[r][q] for q in range(3)] for r in range(3)]
    y = [sc[r] - sb[r] for r in range(3)]
    st, x, ratio = solve3_colpiv(A, y)
    return st, np.array(x), ratio, np.array(A), n


def triangulate(Twc, cam, offsets, obs_pose, obs_xy, reverse=False):
    """The batch: (position [n, 3], status [n], ratio [n], [AxtAx or None], valid observers [n])"""
    Twc = np.asarray(Twc, np.float64).reshape(-1, 4, 4)
    obs_xy = np.asarray(obs_xy, np.float64).reshape(-1, 2)
    out = [triangulate_point(Twc, obs_pose[a:b], obs_xy[a:b], cam, reverse) for a, b in zip(offsets[:-1], offsets[1:])]
    return (np.array([o[1] for o in out]).reshape(-1, 3), np.array([o[0] for o in out], np.uint8),
            np.array([o[2] for o in out]), [o[3] for o in out], np.array([o[4] for o in out], np.int64))


def position_bound(A, n_obs, p_ref):
    """4 (3 + n_obs) 2^-53 kappa_2(AxtAx) |p_ref|: the backward-stable 3x3 solve plus the n_obs-term sums"""
    return 4.0 * (3 + n_obs) * 2.0 ** -53 * np.linalg.cond(A, 2) * np.linalg.norm(p_ref)


# ------------------------------------------------------------------------------------------------
# Map::TriangulateMaplineByMappoints: cv::fitLine(DIST_L2) restated, float32
# ------------------------------------------------------------------------------------------------
def fit_line_l2(pts):
    """pts: list of (x, y, z) float32 -> [vx, vy, vz, x0, y0, z0] float32"""
    with np.errstate(all="ignore"):  # theta * theta may overflow to inf, which the rotation handles (t = 0)
        return _fit_line_l2(pts)


def _fit_line_l2(pts):
    z = F32(0)
    x0 = y0 = z0 = x2 = y2 = z2 = xy = yz = xz = z
    for (px, py, pz) in pts:
        x2 = x2 + px * px; y2 = y2 + py * py; z2 = z2 + pz * pz
        xy = xy + px * py; yz = yz + py * pz; xz = xz + px * pz
        x0 = x0 + px; y0 = y0 + py; z0 = z0 + pz
    w0 = F32(len(pts))
    x2, y2, z2, xy, yz, xz, x0, y0, z0 = [v / w0 for v in (x2, y2, z2, xy, yz, xz, x0, y0, z0)]
    dx2, dy2, dz2 = x2 - x0 * x0, y2 - y0 * y0, z2 - z0 * z0
    dxy, dxz, dyz = xy - x0 * y0, xz - x0 * z0, yz - y0 * z0
    a = [[dz2 + dy2, -dxy, -dxz], [-dxy, dx2 + dz2, -dyz], [-dxz, -dyz, dy2 + dx2]]
    v = [[F32(1), F32(0), F32(0)], [F32(0), F32(1), F32(0)], [F32(0), F32(0), F32(1)]]
    one, two = F32(1), F32(2)
    for _ in range(8):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = a[p][q]
            if apq == 0:
                continue
            theta = (a[q][q] - a[p][p]) / (two * apq)
            t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
            c = one / np.sqrt(t * t + one)
            s = t * c
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            a[p][q] = a[q][p] = F32(0)
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * arp - s * arq
            a[r][q] = a[q][r] = s * arp + c * arq
            for i in range(3):
                vip, viq = v[i][p], v[i][q]
                v[i][p] = c * vip - s * viq
                v[i][q] = s * vip + c * viq
    e0, e1, e2 = a[0][0], a[1][1], a[2][2]
    i = (0 if e0 < e2 else 2) if e0 < e1 else (1 if e1 < e2 else 2)
    n = F32(np.sqrt(float(v[0][i]) * float(v[0][i]) + float(v[1][i]) * float(v[1][i]) + float(v[2][i]) * float(v[2][i])))
    out = [v[0][i] / n, v[1][i] / n, v[2][i] / n, x0, y0, z0]
    assert all(type(o) is F32 for o in out)   # no operation above was promoted to double
    return out


def point_line_distance(p, line):
    x, y, z = p[0] - line[3], p[1] - line[4], p[2] - line[5]
    c0, c1, c2 = line[1] * z - line[2] * y, line[2] * x - line[0] * z, line[0] * y - line[1] * x
    return np.sqrt(c0 * c0 + c1 * c1 + c2 * c2)


def line_from_cartesian(c):
    """g2o::Line3D::fromCartesian (point | direction) -> (w, d), Python floats"""
    c = [float(v) for v in c]
    n = math.sqrt(c[3] * c[3] + c[4] * c[4] + c[5] * c[5])
    d = [c[3] / n, c[4] / n, c[5] / n]
    dp = d[0] * c[0] + d[1] * c[1] + d[2] * c[2]
    p = [c[0] - d[0] * dp, c[1] - d[1] * dp, c[2] - d[2] * dp]
    q = [p[0] + d[0], p[1] + d[1], p[2] + d[2]]
    return np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0], d[0], d[1], d[2]])


def triangulate_mapline(mr, l):
    if l.type == map_ref.GOOD:
        return True
    if len(l.obs) < 2:
        return False
    pts = []
    for fid in sorted(l.obs):
        f = mr.keyframes.get(fid)
        if f is None:
            continue
        k = l.obs[fid]
        if not 0 <= k < len(f.points_on_lines):
            continue
        for kp in sorted(f.points_on_lines[k]):
            if not 0 <= kp < len(f.mappoints):
                continue
            q = f.mappoints[kp]
            if q is None or q.type != map_ref.GOOD:
                continue
            pts.append((F32(q.p[0]), F32(q.p[1]), F32(q.p[2])))
    if len(pts) < 2:
        return False
    for _ in range(4):
        line = fit_line_l2(pts)
        before = len(pts)
        pts = [p for p in pts if float(point_line_distance(p, line)) < 0.2]
        if len(pts) == before or len(pts) < 3:
            break
    if len(pts) < 2:
        return False
    l.L = line_from_cartesian([line[3], line[4], line[5], line[0], line[1], line[2]])
    l.type = map_ref.GOOD
    md, max_v = 0, abs(line[0])
    for i in (1, 2):
        if abs(line[i]) > max_v:
            md, max_v = i, abs(line[i])
    lo = hi = 0
    for j in range(1, len(pts)):
        if pts[j][md] < pts[lo][md]:
            lo = j
        if pts[j][md] > pts[hi][md]:
            hi = j
    l.endpoints = np.array([float(v) for v in pts[lo] + pts[hi]])
    l.endpoints_valid = True
    for fid in l.obs:
        if fid in mr.keyframes:
            l.incl[fid] = 1
    return True


# ------------------------------------------------------------------------------------------------
# Map::InsertKeyframe on oracle/map_ref.py's structures
# ------------------------------------------------------------------------------------------------
def insert_keyframe(mr, f, stage, next_line_track_id):
    """f: a synthetic.raw_sequence keyframe; stage: its stereo-stage result (``stereo`` above).  Everything of
    map.cc:24-103 (no LocalMapOptimization).  Returns (report dict, next line track id)."""
    n = len(f["feat_left"])
    kp = np.column_stack([f["feat_left"][:, 1:3], stage["u_right"]]) if n else np.zeros((0, 3))
    fid = f["id"]
    if fid in mr.keyframes:
        raise ValueError(f"frame {fid} exists")
    fresh = set()
    for i in range(n):
        if f["point_slot"][i] < 0 and stage["new_point"][i]:
            t = int(stage["track_id"][i])
            if t in mr.mappoints or t in fresh:
                raise ValueError(f"new map point {t} is already in the map")
            fresh.add(t)
    fr = map_ref.Frame(fid, f["timestamp"], f["Twc"], kp, f["lines_left"], f["lines_right"], f["lines_right_valid"],
                       f["points_on_lines"], f["parent_id"] if f["parent_id"] >= 0 else None)
    mr.insert_keyframe(fr)
    first = len(mr.keyframes) < 2
    rep = dict(n_new_points=0, n_new_lines=0, n_tri_candidates=0, n_tri_ok=0, n_tri_rank_failures=0,
               n_lines_triangulated=0, ratios=[], tri=[])  # tri: (id, status, position, AxtAx, valid observers)
    cand = []
    for i in range(n):
        slot = int(f["point_slot"][i])
        if slot >= 0:
            q = mr.mappoints[slot]
        elif stage["new_point"][i]:
            good = stage["new_point"][i] == 1
            q = map_ref.Mappoint(int(stage["track_id"][i]), stage["new_position"][i] if good else np.zeros(3),
                                 map_ref.GOOD if good else map_ref.UNTRI)
            mr.mappoints[q.id] = q
            rep["n_new_points"] += 1
        else:
            continue
        fr.mappoints[i] = q
        q.obs[fid] = i
        if not first and q.type == map_ref.UNTRI and q.num_obs() > 2:
            cand.append(q)
    rep["n_tri_candidates"] = len(cand)
    cam = mr.camera
    for q in cand:
        frames = sorted(q.obs)
        poses, op, xy = [], [], []
        for g in frames:
            of, k = mr.keyframes.get(g), q.obs[g]
            if of is not None and 0 <= k < len(of.kp):
                op.append(len(poses))
                poses.append(of.pose)
                xy.append(of.kp[k, :2])
            else:
                op.append(-1)
                xy.append([0.0, 0.0])
        st, p, ratio, A, nv = triangulate_point(poses, op, xy, cam)
        rep["ratios"].append(ratio)
        rep["tri"].append((q.id, st, p, A, nv))
        if st == TRI_OK:
            q.p, q.type = p, map_ref.GOOD
            rep["n_tri_ok"] += 1
        elif st == TRI_RANK:
            rep["n_tri_rank_failures"] += 1
    nxt = next_line_track_id
    for i in range(len(f["lines_left"])):
        lid = int(f["line_track_id"][i])
        if lid < 0:
            lid, nxt = nxt, nxt + 1
        slot = int(f["line_slot"][i])
        if slot >= 0:
            l = mr.maplines[slot]
        else:
            if lid in mr.maplines:
                raise ValueError(f"new map line {lid} is already in the map")
            l = map_ref.Mapline(lid, np.zeros(6), map_ref.UNTRI)
            l.incl = {}
            mr.maplines[lid] = l
            rep["n_new_lines"] += 1
        fr.maplines[i] = l
        l.obs[fid] = i
        if l.incl.get(fid, -1) < 0:
            l.incl[fid] = 0
        if not first and l.type == map_ref.UNTRI and l.num_obs() >= 2:
            rep["n_lines_triangulated"] += bool(triangulate_mapline(mr, l))
    return rep, nxt
