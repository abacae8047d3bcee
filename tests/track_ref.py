"""numpy restatement of the host steps of MapBuilder::TrackFrame + FramePoseOptimization
(src/map_builder.cc:448-611) that rspl_track_* runs on the device: the mutual check and the `inliers`
vector (step 1), the ordered correspondences and edges (step 2), the seed gate and pose conversion
(step 4) and the write-back (step 6).  PnP and FrameOptimization themselves are oracle.pnp /
oracle.frame_opt.  Inputs are the dicts synthetic.track_problem returns."""
import numpy as np

from rspl_slam_amd import synthetic as SY
from rspl_slam_amd.ba_types import FrameProblem, OptimizationConfig

TH_MONO, TH_STEREO = 5.991, 7.815  # tracking OptimizationConfig (configs/configs_euroc.yaml)


def matches(idx0, idx1, n0):
    """match_kf[i] = j iff j = idx1[i], 0 <= j < n0 and idx0[j] == i (point_matching.cc:24-31), else -1"""
    out = np.full(len(idx1), -1, np.int32)
    for i, j in enumerate(idx1):
        if 0 <= j < n0 and idx0[j] == i:
            out[i] = j
    return out


def gather(p):
    """Steps 1 and 2.  Correspondences in ascending current keypoint index, kept when the partner's state
    is 1; the PnP copy float-rounded; edges mono first then stereo, each in ascending index."""
    n0 = len(p["state"])
    mk = matches(p["idx0"], p["idx1"], n0)
    inl = np.where(mk >= 0, p["track_id"][np.maximum(mk, 0)] if n0 else -1, -1).astype(np.int32)
    corr = np.array([i for i, j in enumerate(mk) if j >= 0 and p["state"][j] == 1], np.int64)
    j = mk[corr]
    X = p["points"][j].reshape(-1, 3)
    uv = p["features"][corr, 1:3].reshape(-1, 2)
    ur = p["u_right"][corr] if p["u_right"] is not None else np.full(len(corr), -1.0)
    stereo = ur > 0
    order = np.concatenate([np.flatnonzero(~stereo), np.flatnonzero(stereo)]).astype(np.int64)
    edges = np.zeros((len(corr), 12))
    edges[:, 0:3] = X[order]
    edges[:, 3:5] = uv[order]
    edges[:, 5] = np.where(stereo[order], ur[order], 0.0)
    edges[:, 6:11] = p["cam"]
    edges[:, 11] = stereo[order]
    return dict(match_kf=mk, inl=inl, corr_kp=corr.astype(np.int32), n_matches=int((mk >= 0).sum()),
                pnp_points=X.astype(np.float32).astype(np.float64), pnp_keypoints=uv.astype(np.float32).astype(np.float64),
                edge_kp=corr[order].astype(np.int32), edges=edges, n_mono=int((~stereo).sum()), n_stereo=int(stereo.sum()))


def normalize(q_wxyz):
    q = np.array(q_wxyz, np.float64)
    if q[0] < 0:
        q = -q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def seed(n_pnp, Rwc, twc, last_Twc, min_num_match=10):
    """Step 4: (pnp_used, q (x, y, z, w), p) of the T_wc FrameOptimization starts from."""
    last_Twc = np.asarray(last_Twc, np.float64)
    use = n_pnp > 0
    if use:
        d = np.asarray(twc) - last_Twc[:3, 3]
        use = not (np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) > 0.5 or n_pnp < min_num_match)
    R, t = (np.asarray(Rwc), np.asarray(twc)) if use else (last_Twc[:3, :3], last_Twc[:3, 3])
    x, y, z, w = SY.R_to_quat_xyzw(R)
    w, x, y, z = normalize([w, x, y, z])
    return bool(use), np.array([x, y, z, w]), np.array(t, np.float64)


def frame_problem(g, q, p, th=(TH_MONO, TH_STEREO)):
    """FrameOptimization's input for gather() output `g` (or the device's own stage with the same keys)
    started from T_wc = (q, p)."""
    E = np.asarray(g["edges"]).reshape(-1, 12)
    nm = g["n_mono"]
    cam = E[0, 6:11] if len(E) else np.array([1.0, 1.0, 0.0, 0.0, 0.0])
    return FrameProblem(cameras=np.array([cam]), pose_q=q, pose_p=p, points=E[:, 0:3],
                        mono=dict(lm=np.arange(nm), obs=E[:nm, 3:5]),
                        stereo=dict(lm=np.arange(nm, len(E)), obs=E[nm:, 3:6]),
                        cfg=OptimizationConfig(mono_point=th[0], stereo_point=th[1]))


def write_back(g, edge_inlier, n_inliers, min_num_match=10):
    """Step 6: (pose_set, track_id [n1], kept [n1]).  `> 0` strictly, as the reference: track id 0 is
    dropped."""
    mk, inl = g["match_kf"], g["inl"].copy()
    n1 = len(mk)
    pose_set = n_inliers > min_num_match
    tid, kept = np.full(n1, -1, np.int32), np.zeros(n1, bool)
    if pose_set:
        flags = np.asarray(edge_inlier).astype(bool)
        inl[g["edge_kp"][~flags]] = -1
        ok = (mk >= 0) & (inl > 0)
        tid[ok] = inl[ok]
        kept = ok
    else:
        kept = mk >= 0
    return bool(pose_set), tid, kept


def chain(p, oracle, min_num_match=10, seed_eps=0.0):
    """The whole step on the CPU: gather -> oracle.pnp -> seed -> oracle.frame_opt -> write_back.
    seed_eps perturbs the seed pose (the end-to-end test's conditioning check)."""
    g = gather(p)
    n_pnp, Rwc, twc, pinl, _ = oracle.pnp(np.array(p["cam"][:4]), g["pnp_points"], g["pnp_keypoints"])
    used, q, t = seed(n_pnp, Rwc, twc, p["last_Twc"], min_num_match)
    if seed_eps:
        t = t + seed_eps
        w, x, y, z = normalize([q[3], q[0] + seed_eps, q[1] - seed_eps, q[2] + seed_eps])
        q = np.array([x, y, z, w])
    r = oracle.frame_opt(frame_problem(g, q, t))
    flags = np.concatenate([r.inlier["mono"], r.inlier["stereo"]])
    pose_set, tid, kept = write_back(g, flags, r.n_inliers, min_num_match)
    if pose_set:
        pose_q, pose_p = r.pose_q, r.pose_p
    else:
        _, pose_q, pose_p = seed(0, None, None, p["last_Twc"])
    return dict(gather=g, n_pnp_inliers=n_pnp, pnp_used=used, seed_q=q, seed_p=t, frame=r, flags=flags,
                pose_set=pose_set, pose_q=np.asarray(pose_q), pose_p=np.asarray(pose_p), n_inliers=r.n_inliers,
                track_id=tid, kept=kept)
