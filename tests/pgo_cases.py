"""Seeded pose-graph cases for the pgo tests (tests/pgo_ref.py is the reference).

A case is a ring trajectory with edges to the next `span` keyframes, consistent measurements (zero residual) or
noisy ones (sigma_t 0.02 m, sigma_r 0.01 rad), initial poses from integrated odometry with 1 % drift, pose 0 fixed.
n_free sits at the sizes where the tile code (16 poses per tile) can go wrong.

POSE_TOL / GRAD_TOL: measured on a CPU per case at the default parameters, the host twin against pgo_ref: the
distance of its poses from pgo_ref's (max over poses of |dp| in m and of the rotation angle in rad), and |J^T W e| at
its poses relative to the initial one.  The GPU tests allow ten times these values (stationarity capped at 1e-6); a
case above 1e-7 is replaced, not loosened.  Status and iteration count are compared on every case at the default
parameters: the contract ends a call at the first trial the cost cannot resolve (include/rspl.h), so the last decision
never rests on rounding, and pgo_ref dense, pgo_ref sparse and the host twin agree in status, iterations and trials.
"""
import functools

import numpy as np

import pgo_ref

SIGMA_T, SIGMA_R, DRIFT = 0.02, 0.01, 0.01


def _compose(qa, pa, qb, pb):
    return pgo_ref.qmul(qa, qb), pa + pgo_ref.qmat(qa) @ pb


def _relative(qi, pi, qj, pj):
    return pgo_ref.qmul(pgo_ref.qconj(qi), qj), pgo_ref.qmat(qi).T @ (pj - pi)


def ring_truth(n, radius=10.0):
    """n poses on a circle of `radius`, heading along the tangent, with a gentle climb and roll"""
    q, p = np.zeros((n, 4)), np.zeros((n, 3))
    for i in range(n):
        a = 2 * np.pi * i / max(n, 8)
        p[i] = [radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(3 * a)]
        yaw = pgo_ref.qexp(np.array([0.0, 0.0, a + np.pi / 2]))
        roll = pgo_ref.qexp(np.array([0.1 * np.sin(2 * a), 0.05 * np.cos(a), 0.0]))
        q[i] = pgo_ref.qmul(yaw, roll)
    return q, p


def build(n_poses, span, seed, noisy, loops=(), extra_edges=(), fixed=(0,), weights=None, offset=0):
    """one ring: dict of arrays; `loops` / `extra_edges`: (i, j) pairs measured like any other edge"""
    rng = np.random.default_rng(seed)
    tq, tp = ring_truth(n_poses)
    pairs = [(i, i + k) for i in range(n_poses) for k in range(1, span + 1) if i + k < n_poses]
    pairs += list(loops) + list(extra_edges)
    ei, ej, eq, ep = [], [], [], []
    for i, j in pairs:
        zq, zp = _relative(tq[i], tp[i], tq[j], tp[j])
        if noisy:
            zq = pgo_ref.qmul(zq, pgo_ref.qexp(SIGMA_R * rng.standard_normal(3)))
            zp = zp + SIGMA_T * rng.standard_normal(3)
        ei.append(i + offset); ej.append(j + offset); eq.append(zq); ep.append(zp)
    # integrated odometry with drift, from the true pose 0
    q, p = tq.copy(), tp.copy()
    for i in range(1, n_poses):
        zq, zp = _relative(tq[i - 1], tp[i - 1], tq[i], tp[i])
        zq = pgo_ref.qmul(zq, pgo_ref.qexp(DRIFT * np.array([0.3, -0.2, 1.0]) * np.linalg.norm(pgo_ref.qlog(zq))))
        q[i], p[i] = _compose(q[i - 1], p[i - 1], zq, (1 + DRIFT) * zp)
        q[i] /= np.linalg.norm(q[i])
    ne = len(ei)
    if weights is None:
        w = np.ones((ne, 2))
    else:
        w = 10.0 ** rng.uniform(np.log10(weights[0]), np.log10(weights[1]), (ne, 2))
    fx = np.zeros(n_poses, np.uint8)
    fx[list(fixed)] = 1
    return dict(pose_q=q, pose_p=p, pose_fixed=fx, edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32),
                edge_q=np.array(eq).reshape(-1, 4), edge_p=np.array(ep).reshape(-1, 3), edge_w=w, truth_q=tq, truth_p=tp)


def _join(a, b):
    out = {}
    for k in a:
        out[k] = np.concatenate([a[k], b[k]])
    return out


def _two_components():
    return _join(build(13, 2, 21, True, loops=[(12, 1)]), build(12, 2, 22, True, loops=[(11, 2)], offset=13))


def _isolated():
    c = build(11, 2, 23, True, loops=[(10, 1)])
    c["pose_q"] = np.vstack([c["pose_q"], [[0.1, -0.2, 0.3, 0.9]]])
    c["pose_q"][-1] /= np.linalg.norm(c["pose_q"][-1])
    c["pose_p"] = np.vstack([c["pose_p"], [[1.0, 2.0, 3.0]]])
    c["truth_q"] = np.vstack([c["truth_q"], c["pose_q"][-1:]])
    c["truth_p"] = np.vstack([c["truth_p"], c["pose_p"][-1:]])
    c["pose_fixed"] = np.append(c["pose_fixed"], 0).astype(np.uint8)
    return c


def _rot170():
    c = build(9, 2, 24, True, loops=[(8, 1)])
    # turn the last pose so that edge (7, 8) starts 170 degrees off
    c["pose_q"][8] = pgo_ref.qmul(c["pose_q"][8], pgo_ref.qexp(np.deg2rad(170.0) * np.array([0.0, 0.6, 0.8])))
    return c


# name -> builder; n_free is one less than the pose count of a single ring
CASES = {
    "n1": lambda: build(2, 1, 1, True),
    "n15": lambda: build(16, 2, 2, True, loops=[(15, 1)]),
    "n16": lambda: build(17, 2, 3, True, loops=[(16, 1)]),
    "n17": lambda: build(18, 2, 4, True, loops=[(17, 1)]),
    "n33_arrow": lambda: build(34, 2, 5, True, loops=[(33, 2)]),   # the last pose to free pose 1: an arrow row of fill
    "n40_hub": lambda: build(41, 1, 13, True, extra_edges=[(i, 40) for i in range(1, 39)]),  # degree 39, last tile
    "n130": lambda: build(131, 4, 7, True, loops=[(130, 1), (100, 3), (64, 2)]),            # nine tiles
    "two_components": _two_components,
    "isolated": _isolated,
    "rot170": _rot170,
    "zero20": lambda: build(21, 2, 8, False, loops=[(20, 1)]),     # zero residual: ends in the small-angle branches
    "zero40": lambda: build(41, 2, 9, False, loops=[(40, 1)]),
    "weights": lambda: build(25, 3, 18, True, loops=[(24, 1)], weights=(1e-2, 1e4)),
}
NOISY = ("n1", "n15", "n16", "n17", "n33_arrow", "n40_hub", "n130", "two_components", "isolated", "rot170", "weights")

# measured on a CPU: host twin against pgo_ref (see the module docstring)
POSE_TOL = {"n1": 1.1e-16, "n15": 4.4e-15, "n16": 1.8e-15, "n17": 4.7e-15, "n33_arrow": 3.0e-15, "n40_hub": 9.7e-15,
            "n130": 7.1e-15, "two_components": 6.4e-15, "isolated": 4.4e-15, "rot170": 3.6e-15, "zero20": 1.8e-15,
            "zero40": 3.6e-15, "weights": 6.2e-15}
GRAD_TOL = {"n1": 5.1e-15, "n15": 1.6e-09, "n16": 3.1e-09, "n17": 2.8e-09, "n33_arrow": 8.4e-09, "n40_hub": 3.0e-11,
            "n130": 8.4e-08, "two_components": 6.1e-09, "isolated": 1.2e-09, "rot170": 8.3e-12, "zero20": 2.2e-14,
            "zero40": 2.3e-14, "weights": 5.9e-09}
GRAD_CAP = 1e-6  # of the initial gradient
ZERO = ("zero20", "zero40")

PROBLEM_KEYS = ("pose_q", "pose_p", "pose_fixed", "edge_i", "edge_j", "edge_q", "edge_p", "edge_w")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def args(c):
    return tuple(c[k] for k in PROBLEM_KEYS)


def problem(name):
    return pgo_ref.Problem(*args(case(name)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """pgo_ref's solve of the case, computed once per process"""
    return pgo_ref.solve(problem(name))


@functools.lru_cache(maxsize=None)
def initial_gradient(name):
    P = problem(name)
    return pgo_ref.gradient_norm(P, P.pose_q, P.pose_p)


@functools.lru_cache(maxsize=None)
def reference_system(name):
    """(e, H, b, lambda_0) of the case's first linearisation"""
    e, H, b = pgo_ref.linearise(problem(name))
    return e, H, b, 1e-5 * float(H.diagonal().max())


def pose_distance(qa, pa, qb, pb):
    """(max |dp|, max rotation angle) between two pose sets"""
    dp = float(np.abs(np.asarray(pa) - np.asarray(pb)).max())
    da = max(float(np.linalg.norm(pgo_ref.qlog(pgo_ref.qmul(pgo_ref.qconj(x), y)))) for x, y in zip(qa, qb))
    return dp, da


def lone_free_pose():
    """two fixed poses with an edge between them and one free pose that no edge touches"""
    c = build(2, 1, 12, True, fixed=(0, 1))
    for k, v in (("pose_q", [[0.5, -0.5, 0.5, 0.5]]), ("pose_p", [[3.0, -2.0, 1.0]])):
        c[k] = np.vstack([c[k], v])
        c["truth_" + k[5:]] = np.vstack([c["truth_" + k[5:]], v])
    c["pose_fixed"] = np.array([1, 1, 0], np.uint8)
    return c


def big_ring(n_poses, span=4, n_loops=3, seed=11):
    """the zero-residual ring of the scale test and tools/bench_pgo.py"""
    loops = [(n_poses - 1 - 7 * k, 1 + 5 * k) for k in range(n_loops)]
    return build(n_poses, span, seed, False, loops=loops)


# ---- the bounds on an LM result, shared by the CPU test of the host twin and the GPU tests ------------------------
def check_default(name, out, log=print):
    """`out`: a solve of case `name` at the default parameters (dict of api.pgo_host / PoseGraph.solve)"""
    R, P = reference(name), problem(name)
    dc = abs(out["cost_final"] - R.cost_final)
    dp, da = pose_distance(R.pose_q, R.pose_p, out["pose_q"], out["pose_p"])
    g = pgo_ref.gradient_norm(P, out["pose_q"], out["pose_p"]) / initial_gradient(name)
    pose_tol, grad_tol = 10 * POSE_TOL[name], min(10 * GRAD_TOL[name], GRAD_CAP)
    log(f"{name}: |dF| {dc:.3e} (F {R.cost_final:.3e}) dp {dp:.3e} da {da:.3e} (tol {pose_tol:.1e}) "
        f"grad {g:.3e} (tol {grad_tol:.1e}) status {out['status']}/{R.status} iterations {out['iterations']}/{R.iterations} "
        f"trials {out['trials']}/{R.trials}")
    assert abs(out["cost_initial"] - R.cost_initial) <= 1e-10 * R.cost_initial + 1e-24
    assert dc <= 1e-10 * R.cost_final + 1e-24, (name, dc)
    assert out["status"] == R.status, (name, out["status"], R.status)
    assert abs(out["iterations"] - R.iterations) <= 1, (name, out["iterations"], R.iterations)
    assert max(dp, da) <= pose_tol, (name, dp, da)
    assert g <= grad_tol, (name, g)


# ---- the two-lap scene of the CloseLoop test --------------------------------------------------------------------
LOOP_CAM, LOOP_W, LOOP_H = (256.0, 256.0, 256.0, 192.0, 32.0), 512, 384


def _outward_pose(angle, radius=4.0):
    """a camera on a circle about the z axis looking outward: camera z radial, x along the tangent, y down"""
    T = np.eye(4)
    r = np.array([np.cos(angle), np.sin(angle), 0.0])
    T[:3, 0], T[:3, 1], T[:3, 2] = [-np.sin(angle), np.cos(angle), 0.0], [0.0, 0.0, -1.0], r
    T[:3, 0] = np.cross(T[:3, 1], T[:3, 2])
    T[:3, 3] = radius * r
    return T


def loop_project(T, X):
    """(visible mask, pixels [n, 2]) of world points X in the camera T_wc = T"""
    pc = (X - T[:3, 3]) @ T[:3, :3]
    z = np.where(pc[:, 2] > 0.5, pc[:, 2], 1.0)
    u = LOOP_CAM[0] * pc[:, 0] / z + LOOP_CAM[2]
    v = LOOP_CAM[1] * pc[:, 1] / z + LOOP_CAM[3]
    vis = (pc[:, 2] > 0.5) & (u > 1) & (u < LOOP_W - 1) & (v > 1) & (v < LOOP_H - 1)
    return vis, np.stack([u, v], axis=1)


def loop_scene(n_per_lap=12, n_points=600, seed=31):
    """Two laps of `n_per_lap` keyframes past `n_points` points on a wall.  Lap 1 (ids 0..) is mapped at the truth and
    observes the points; lap 2 (ids n_per_lap..) revisits the same places with a drift that grows by a fixed motion
    per keyframe and observes nothing yet.  Returns dict: truth [2n][4][4], estimate [2n][4][4], points [n][3],
    descriptors [n][256], sees {lap-1 id: point ids}, and the closing keyframe's features [k][259] (its image is taken
    at its true pose) with the ids of the points behind them."""
    rng = np.random.default_rng(seed)
    n = n_per_lap
    a = rng.uniform(0, 2 * np.pi, n_points)
    X = np.stack([9.0 * np.cos(a), 9.0 * np.sin(a), rng.uniform(-1.5, 1.5, n_points)], axis=1)
    desc = rng.standard_normal((n_points, 256))
    desc /= np.linalg.norm(desc, axis=1, keepdims=True)
    truth = np.array([_outward_pose(2 * np.pi * (k % n) / n) for k in range(2 * n)])
    step = np.eye(4)  # the drift one lap-2 step adds, in the camera frame
    step[:3, :3] = pgo_ref.qmat(pgo_ref.qexp(np.array([0.002, -0.004, 0.003])))
    step[:3, 3] = [0.03, -0.01, 0.02]
    est = truth.copy()
    for k in range(n, 2 * n):
        est[k] = est[k - 1] @ (np.linalg.inv(truth[k - 1]) @ truth[k]) @ step
    sees = {k: np.flatnonzero(loop_project(truth[k], X)[0]) for k in range(n)}
    vis, px = loop_project(truth[2 * n - 1], X)
    ids = np.flatnonzero(vis)
    F = np.zeros((len(ids), 259))
    F[:, 0], F[:, 1:3], F[:, 3:] = 0.5, px[ids], desc[ids]
    return dict(truth=truth, estimate=est, points=X, descriptors=desc, sees=sees, features=F, feature_ids=ids)


def loop_map(pkg, S):
    """the native map of loop_scene: keyframes with parents, lap 1's points and observations, its connections"""
    M = pkg.mapping.Map(list(LOOP_CAM))
    n2 = len(S["truth"])
    M.InsertMappoints(np.arange(len(S["points"]), dtype=np.int32), S["points"])
    for k in range(n2):
        pts = S["sees"].get(k, np.zeros(0, np.int64))
        px = loop_project(S["truth"][k], S["points"][pts])[1] if len(pts) else np.zeros((0, 2))
        kps = np.concatenate([px, -np.ones((len(pts), 1))], axis=1) if len(pts) else np.zeros((1, 3))
        M.InsertKeyframe(k, 0.1 * k, S["estimate"][k], kps, parent_id=k - 1)
        if len(pts):
            M.AddPointObservations(k, pts.astype(np.int32), np.arange(len(pts), dtype=np.int32))
    for k in S["sees"]:
        M.UpdateFrameConnection(k)
    return M


def loop_errors(M, S):
    """per keyframe: the distance of its position from the truth"""
    return np.array([np.linalg.norm(M.GetPose(k)[:3, 3] - S["truth"][k][:3, 3]) for k in range(len(S["truth"]))])
