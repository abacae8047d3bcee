"""Shared scenes of the F-matrix RANSAC tests (tests/test_fm_cpu.py, tests/test_gpu_fm.py, tools/bench_fm.py).

Two pinhole views (EuRoC's left intrinsics, tests/golden/calib/euroc.yaml) of seeded random 3-D points at
2 - 20 m, a relative pose with rotation and translation, pixels rounded to float.  A chosen fraction of the
matches is replaced by outliers at least 30 px off their epipolar line in image 1; inliers are exact or carry
at most 0.3 px of noise; the ground-truth inlier set is returned.

`checked_scene` is what every equality assertion uses: it runs tests/fm_ref.py on the scene and asserts the
PRECONDITION that no decision of the restatement sits at rounding level -- among the iterations fm_ref
evaluates, no (model, correspondence) error within the relative margin MARGIN of the threshold and no cubic
discriminant within MARGIN of zero (relative to |Q^3| + R^2).  A scene that fails it is not used: change the
seed, never the margin.

MARGIN: 100 x the largest relative difference measured between the device's per-hypothesis errors
(rspl_fm_debug_hypotheses' F evaluated in numpy; errors within a factor 100 of the threshold, where a difference
can decide) and fm_ref's on these scenes: tests/test_gpu_fm.py prints it and asserts that MEASURED_REL_ERR stays
an upper bound (DESIGN 5e records both).  The winning model must also not tie with another model of its
iteration: the order of a subset's models follows the null-space basis and is not part of the contract.
"""
import functools
import pathlib
import re

import numpy as np

import fm_ref

ROOT = pathlib.Path(__file__).resolve().parents[1]
MEASURED_REL_ERR = 3.2e-8  # the largest relative (device - fm_ref) per-hypothesis error difference (3.16e-8), rounded up
MARGIN = 100 * MEASURED_REL_ERR
WIDTH, HEIGHT = 752, 480


@functools.lru_cache(maxsize=None)
def intrinsics():
    """fx, fy, cx, cy of LEFT.K"""
    text = (ROOT / "tests" / "golden" / "calib" / "euroc.yaml").read_text()
    m = re.search(r"LEFT\.K:.*?data:\s*\[([^\]]*)\]", text, re.S)
    k = [float(v) for v in m.group(1).split(",")]
    return k[0], k[4], k[2], k[5]


def relative_pose(rng):
    """R, t of view 1 (x1 = R x0 + t): a few degrees about a random axis and ~0.3 m of translation"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = np.deg2rad(rng.uniform(3.0, 8.0))
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t = rng.normal(size=3)
    t *= rng.uniform(0.2, 0.5) / np.linalg.norm(t)
    return R, t


def true_F(R, t):
    fx, fy, cx, cy = intrinsics()
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    return Ki.T @ tx @ R @ Ki


def scene(n, outliers=0.0, noise=0.0, seed=0):
    """(points0 [n, 2], points1 [n, 2], inlier [n] bool, F_true [3, 3]); float-rounded pixels as float64"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = intrinsics()
    R, t = relative_pose(rng)
    F = true_F(R, t)
    p0 = np.zeros((n, 2))
    p1 = np.zeros((n, 2))
    k = 0
    while k < n:  # points in front of both cameras and inside both images
        z = rng.uniform(2.0, 20.0)
        u, v = rng.uniform(8, WIDTH - 8), rng.uniform(8, HEIGHT - 8)
        X = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        Y = R @ X + t
        if Y[2] < 0.5:
            continue
        a, b = fx * Y[0] / Y[2] + cx, fy * Y[1] / Y[2] + cy
        if not (8 <= a < WIDTH - 8 and 8 <= b < HEIGHT - 8):
            continue
        p0[k] = (u, v)
        p1[k] = (a, b)
        k += 1
    if noise > 0:
        p1 += rng.uniform(-noise, noise, size=p1.shape) / np.sqrt(2.0)  # at most `noise` px in length
    inl = np.ones(n, bool)
    n_out = int(round(outliers * n))
    for i in rng.permutation(n)[:n_out]:
        line = F @ np.array([p0[i, 0], p0[i, 1], 1.0])
        nrm = np.hypot(line[0], line[1])
        while True:  # at least 30 px off the epipolar line of its partner
            q = np.array([rng.uniform(8, WIDTH - 8), rng.uniform(8, HEIGHT - 8)])
            if abs(line[0] * q[0] + line[1] * q[1] + line[2]) / nrm >= 30.0:
                break
        p1[i] = q
        inl[i] = False
    return fm_ref.to_point2f(p0), fm_ref.to_point2f(p1), inl, F


def precondition(ref, margin=MARGIN):
    """the smallest decision margins among the iterations fm_ref evaluated: (error margin, discriminant margin)"""
    em = min([r["margin"] for r in ref["trace"]] + [np.inf])
    dm = min([r["disc"] for r in ref["trace"] if r["disc"] is not None] + [np.inf])
    return em, dm


@functools.lru_cache(maxsize=None)
def checked_scene(n, outliers=0.0, noise=0.0, seed=0, max_iters=1000):
    """scene() + fm_ref's result with its trace, the precondition asserted: (p0, p1, inl, ref)"""
    p0, p1, inl, _ = scene(n, outliers, noise, seed)
    ref = fm_ref.find_fundamental(p0, p1, 3.0, 0.99, max_iters, trace=True)
    em, dm = precondition(ref)
    assert em > MARGIN and dm > MARGIN, (
        f"scene n={n} outliers={outliers} noise={noise} seed={seed}: error margin {em:.3g}, discriminant margin "
        f"{dm:.3g} inside {MARGIN:.3g}: pick another seed")
    assert not ref["order_dependent"], f"scene n={n} seed={seed}: two models of one iteration tie: pick another seed"
    return p0, p1, inl, ref


def pure_outliers(n, seed=0):
    """n unrelated pixel pairs"""
    rng = np.random.default_rng(seed)
    p0 = np.stack([rng.uniform(8, WIDTH - 8, n), rng.uniform(8, HEIGHT - 8, n)], 1)
    p1 = np.stack([rng.uniform(8, WIDTH - 8, n), rng.uniform(8, HEIGHT - 8, n)], 1)
    return fm_ref.to_point2f(p0), fm_ref.to_point2f(p1)


def superpoint_records(points, cap, rng):
    """[cap][259] SuperPoint records (score, x, y, descriptor) holding `points` in rows 1, 2"""
    rec = rng.uniform(-1, 1, size=(cap, 259))
    rec[:, 0] = rng.uniform(0.1, 1.0, cap)
    rec[:len(points), 1:3] = points
    return rec
