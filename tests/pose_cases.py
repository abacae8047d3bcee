"""Shared cases of the pose solvers' edge tests (tests/test_pose_cases_cpu.py on the oracle alone,
tests/test_gpu_pose_edges.py on the device): SolvePnPWithCV and FrameOptimization inputs that
synthetic.pnp_problem / synthetic.frame_problem never draw -- degenerate geometry (a tilted plane, a repeated map
point, world points exactly on z = 0, nothing but outliers, points behind the camera, a poor seed, a rank-deficient
system) and the sizes at which the kernels change path (the 64 / 256 counting strides of the PnP kernels, the
512 | 513 edge switch between LDS and global memory and the staging loop's tails in frame_opt_kernel).

Every case is seeded and builds on the two synthetic generators.  The seeds below were chosen on the CPU so that
each case reaches the path it is meant to reach; tests/test_pose_cases_cpu.py asserts that for every one of them,
so a change to a generator cannot quietly turn an edge test into a generic one.

PnP cases return (K4, X, kp): X and kp hold float-representable values (as float64), which is what
rspl_pnp_solve and the oracle both round their inputs to (cv::Point3f / cv::Point2f), so a construction such as
"z exactly 0" or "the same point 40 times" is what the solver sees."""
import functools

import numpy as np

from rspl_slam_amd import ba_types as BT
from rspl_slam_amd import synthetic as SY

# the C5 workload's 1920 x 1080 camera: EuRoC's rectified intrinsics scaled to the C5 image size, the way
# tools/bench_rect.py scales EuRoC's calibration for its C5 row
C5_W, C5_H = 1920, 1080
C5_CAM = (SY.EUROC_FX * C5_W / 752, SY.EUROC_FY * C5_H / 480, SY.EUROC_CX * C5_W / 752, SY.EUROC_CY * C5_H / 480)

# --- the committed seeds (chosen on the CPU, conditions asserted in tests/test_pose_cases_cpu.py) ---
TILTED_PLANE_SEEDS = (0, 1, 2, 3)
REPEATED_POINT_SEEDS = (1, 3, 5)      # only seeds on which the mirror and the independent oracle agree on the inlier set
WORLD_PLANE_SEED = 0
PNP_ALL_OUTLIERS_SEED = 0
COUNT_EDGES = (8, 9, 63, 64, 65, 255, 256, 257)
COUNT_EDGES_SEED = {8: 41, 9: 41, 63: 42, 64: 43, 65: 44, 255: 45, 256: 46, 257: 47}  # each with a non-empty inlier set
C5_SEED = 5
GENERIC_SEED = 0
FRAME_ALL_OUTLIERS_SEED = 1
BEHIND_CAMERA_SEED = 0
POOR_SEED_SEED = 2
ONE_POINT_SEED = 1
EDGES_SEED = 3                        # edges_512, edges_513 and frame 0 of the variant batches
STAGING_TAILS = (74, 75, 85, 86)
STAGING_TAILS_SEED = 60               # + the index of the count
FILL_SEED = 500                       # + the frame's index: the 12-edge frames that fill a large batch


def _f32(a):
    """float-representable values as float64 (cv::Point3f / cv::Point2f)"""
    return np.ascontiguousarray(a, np.float64).astype(np.float32).astype(np.float64)


def _camera_frame(X, gt):
    """the points of a pnp_problem in its ground-truth camera frame"""
    return (X - gt["twc"]) @ gt["Rwc"]


# ----------------------------------------------------------------------------------------------------------
# SolvePnPWithCV
# ----------------------------------------------------------------------------------------------------------
def generic(seed=GENERIC_SEED, n=300):
    K, X, kp, _ = SY.pnp_problem(n_points=n, outlier_frac=0.2, pixel_sigma=0.8, seed=seed)
    return K, _f32(X), _f32(kp)


def tilted_plane(seed=TILTED_PLANE_SEEDS[0]):
    """200 points on the plane z_c = 4 / (1 - 0.3 x_n) of the camera frame (x_n = x_c / z_c: the plane
    z_c = 4 + 0.3 x_c, about 17 degrees off fronto-parallel), 20 % outliers, sigma 0.8 px: coplanar but not
    axis-aligned world points, on which a few minimal solves fail"""
    K, X, kp, gt = SY.pnp_problem(n_points=200, outlier_frac=0.2, pixel_sigma=0.8, seed=seed)
    Xc = _camera_frame(X, gt)
    xn, yn = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    z = 4.0 / (1.0 - 0.3 * xn)
    assert (z > 0).all()
    Xp = np.stack([xn * z, yn * z, z], 1) @ gt["Rwc"].T + gt["twc"]
    return K, _f32(Xp), _f32(kp)


def repeated_point(seed=REPEATED_POINT_SEEDS[0]):
    """60 correspondences, the first 40 all equal to correspondence 0 (one map point matched 40 times): every
    subset with two or more of them has coincident control points"""
    K, X, kp, _ = SY.pnp_problem(n_points=60, outlier_frac=0.2, pixel_sigma=0.8, seed=seed)
    X, kp = _f32(X), _f32(kp)
    X[:40] = X[0]
    kp[:40] = kp[0]
    return K, X, kp


def world_plane_z0(seed=WORLD_PLANE_SEED):
    """120 world points with z exactly 0 (the pixels' rays cut with the world plane z = 0, the camera 6 m in
    front of it), 20 % outliers: exactly coplanar, axis-aligned points -- the smallest PCA eigenvalue of every
    subset is 0 and every minimal solve fails"""
    K, X, kp, gt = SY.pnp_problem(n_points=120, outlier_frac=0.2, pixel_sigma=0.8, seed=seed)
    Xc = _camera_frame(X, gt)
    d = np.stack([Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2], np.ones(len(Xc))], 1) @ gt["Rwc"].T
    twc = np.array([gt["twc"][0], gt["twc"][1], -6.0])
    assert (d[:, 2] > 0.1).all()
    Xw = twc + d * (6.0 / d[:, 2])[:, None]
    Xw[:, 2] = 0.0
    return K, _f32(Xw), _f32(kp)


def pnp_all_outliers(seed=PNP_ALL_OUTLIERS_SEED):
    K, X, kp, _ = SY.pnp_problem(n_points=100, outlier_frac=1.0, seed=seed)
    return K, _f32(X), _f32(kp)


def count_edge(n):
    """n correspondences around the counting strides (64 per wave in pnp_hyp_kernel, 256 in pnp_final_kernel) and
    at the smallest accepted counts, 20 % outliers"""
    K, X, kp, _ = SY.pnp_problem(n_points=n, outlier_frac=0.2, pixel_sigma=0.8, seed=COUNT_EDGES_SEED[n])
    return K, _f32(X), _f32(kp)


def c5_camera(seed=C5_SEED):
    K, X, kp, _ = SY.pnp_problem(n_points=300, outlier_frac=0.2, pixel_sigma=0.8, seed=seed, width=C5_W, height=C5_H,
                                 cam=C5_CAM)
    return K, _f32(X), _f32(kp)


def seven_points(seed=7):
    """below the 8-correspondence guard: nothing runs"""
    K, X, kp, _ = SY.pnp_problem(n_points=7, outlier_frac=0.0, seed=seed)
    return K, _f32(X), _f32(kp)


def pnp_cases():
    """{name: (K4, X, kp)} of every PnP case"""
    c = {f"tilted_plane[{s}]": tilted_plane(s) for s in TILTED_PLANE_SEEDS}
    c.update({f"repeated_point[{s}]": repeated_point(s) for s in REPEATED_POINT_SEEDS})
    c["world_plane_z0"] = world_plane_z0()
    c["all_outliers"] = pnp_all_outliers()
    c.update({f"count_edges[{n}]": count_edge(n) for n in COUNT_EDGES})
    c["c5_camera"] = c5_camera()
    return c


HYPOTHESIS_CASES = ("tilted_plane", "repeated_point", "world_plane_z0")  # debug_hypotheses compared as well


def reprojection_cost(K4, X, kp, Rwc, twc, mask):
    """sum of squared reprojection errors (px^2) over `mask` at the pose T_wc = (Rwc, twc), in np.longdouble and
    plain numpy: no code of the project's"""
    L = np.longdouble
    R, t = np.asarray(Rwc, L), np.asarray(twc, L)
    Xc = (np.asarray(X, L) - t) @ R          # R_cw (X - t_wc) per row
    u = L(K4[0]) * Xc[:, 0] / Xc[:, 2] + L(K4[2])
    v = L(K4[1]) * Xc[:, 1] / Xc[:, 2] + L(K4[3])
    e = (np.asarray(kp, L)[:, 0] - u) ** 2 + (np.asarray(kp, L)[:, 1] - v) ** 2
    return e[np.asarray(mask, bool)].sum()


# ----------------------------------------------------------------------------------------------------------
# FrameOptimization
# ----------------------------------------------------------------------------------------------------------
def frame_all_outliers(seed=FRAME_ALL_OUTLIERS_SEED):
    return SY.frame_problem(n_points=150, outlier_frac=1.0, seed=seed)[0]


def behind_camera(seed=BEHIND_CAMERA_SEED):
    """150 points, every seventh mirrored through the camera's image plane (z_c -> -z_c at the true pose): map
    points behind the camera, as after a bad PnP seed"""
    prob, gt = SY.frame_problem(n_points=150, outlier_frac=0.1, seed=seed)
    R = SY.quat_xyzw_to_R(gt["pose_q"])
    Xc = (prob.points - gt["pose_p"]) @ R
    Xc[::7, 2] *= -1.0
    prob.points = np.ascontiguousarray(Xc @ R.T + gt["pose_p"])
    return prob


def poor_seed(seed=POOR_SEED_SEED):
    return SY.frame_problem(n_points=150, outlier_frac=0.1, seed=seed, init_rot=0.5, init_trans=3.0)[0]


def one_point_mono(seed=ONE_POINT_SEED):
    """the 12 mono edges of a 12-point frame, all attached to ONE world point (point 0): a 6 x 6 system of rank 2
    whose observations, spread over the image, no pose can meet -- after the first round every edge is an
    outlier"""
    prob, _ = SY.frame_problem(n_points=12, outlier_frac=0.0, seed=seed, stereo_frac=0.0)
    return BT.FrameProblem(cameras=prob.cameras, pose_q=prob.pose_q, pose_p=prob.pose_p, points=prob.points[:1],
                           mono=dict(lm=np.zeros(12, np.int32), obs=prob.mono["obs"]))


def edges(n, seed=EDGES_SEED):
    """a frame of exactly n edges (one per point): edges(512) and edges(513) straddle kLdsEdges"""
    return SY.frame_problem(n_points=n, outlier_frac=0.1, seed=seed)[0]


def staging_tail(n):
    """n edges, six 16-byte pieces each, staged by 64 threads: no lane (74), two lanes (75), 62 lanes (85) and all
    lanes (86, with a four-piece tail behind) take the eight-deep pass of the staging loop"""
    return SY.frame_problem(n_points=n, outlier_frac=0.1, seed=STAGING_TAILS_SEED + STAGING_TAILS.index(n))[0]


def fill_frame(i):
    return SY.frame_problem(n_points=12, outlier_frac=0.0, seed=FILL_SEED + i)[0]


def tiny_frame(n, seed=80):
    return SY.frame_problem(n_points=n, outlier_frac=0.0, seed=seed + n)[0]


def empty_frame():
    return BT.FrameProblem(cameras=edges(12).cameras, pose_q=[0, 0, 0, 1], pose_p=[0.5, 0, 0], points=np.zeros((0, 3)))


def reordered(prob, k):
    """the same problem with its edges in another order: reversed (k = 0) or in a seeded permutation"""
    rng = np.random.default_rng(k)

    def pm(d):
        n = len(d["lm"])
        o = np.arange(n)[::-1] if k == 0 else rng.permutation(n)
        return {key: d[key][o] for key in ("lm", "cam", "obs", "inlier")}

    return BT.FrameProblem(cameras=prob.cameras, pose_q=prob.pose_q, pose_p=prob.pose_p, points=prob.points,
                           mono=pm(prob.mono), stereo=pm(prob.stereo), cfg=prob.cfg)


def order_spread(prob, orders=8):
    """The oracle's own pose spread on `prob`: the largest change of its result (position, quaternion) when the
    SAME problem is given with its edges reordered.  The order only changes how the sums of H, b and chi2 round;
    g2o's stop test (rho == 0, or 10 rejected trials) is decided by the last ulp of chi2, so two orders may stop
    one or more LM steps apart.  On a well-conditioned frame that moves the pose by 1e-13; on a frame of 10 or 12
    edges, whose weakest direction is three to four orders flatter, by up to 6e-9 with chi2 equal to 1e-14.  A
    device reduction tree is one more order: where this spread exceeds a tenth of the 1e-9 contract, the contract
    measures the stop test, not the kernel (tests/test_gpu_pose_edges.py uses 10 x this spread there)."""
    import oracle
    r = oracle.frame_opt(prob)
    worst = 0.0
    for k in range(orders):
        q = oracle.frame_opt(reordered(prob, k))
        s = np.sign(np.dot(r.pose_q, q.pose_q))
        worst = max(worst, float(np.abs(r.pose_p - q.pose_p).max()), float(np.abs(r.pose_q - s * q.pose_q).max()))
    return worst


def n_edges(prob):
    return prob.n_edges("mono") + prob.n_edges("stereo")


def frame_cases():
    """{name: FrameProblem} of every frame case"""
    c = {"all_outliers": frame_all_outliers(), "behind_camera": behind_camera(), "poor_seed": poor_seed(),
         "one_point_mono": one_point_mono(), "edges_512": edges(512), "edges_513": edges(513)}
    c.update({f"staging_tails[{n}]": staging_tail(n) for n in STAGING_TAILS})
    return c


@functools.lru_cache(maxsize=None)
def variant_batches():
    """The four batches that select frame_opt_kernel's four instantiations (frame_kernels.hip::optimize: one wave
    per frame above 256 frames, global memory above kLdsEdges = 512 edges in the batch's largest frame), frame 0
    drawn from the same seed in all four:
      A   1 frame of 512 edges                                                       <true, 4>
      B   1 frame of 513 edges                                                       <false, 4>
      C   257 frames: 400 edges, the four staging_tails frames, 252 12-edge frames   <true, 1>
      D   C with its last frame replaced by B's 513-edge frame                       <false, 1>
    Returns {name: (instantiation, [FrameProblem])}."""
    C = [edges(400)] + [staging_tail(n) for n in STAGING_TAILS] + [fill_frame(i) for i in range(5, 257)]
    D = C[:-1] + [edges(513)]
    return {"A": ("<true,4>", [edges(512)]), "B": ("<false,4>", [edges(513)]), "C": ("<true,1>", C),
            "D": ("<false,1>", D)}


def z_camera(prob, res):
    """z_c of every edge's point at the pose of a FrameResult"""
    R = SY.quat_xyzw_to_R(res.pose_q)
    Xc = (prob.points - res.pose_p) @ R
    return np.concatenate([Xc[prob.mono["lm"], 2], Xc[prob.stereo["lm"], 2]])
