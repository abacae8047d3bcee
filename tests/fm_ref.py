"""cv::findFundamentalMat(points0, points1, cv::FM_RANSAC, 3, 0.99, mask) restated in numpy / Python floats.

The checker of rspl_fm_* (never called by the product).  What is restated is the published algorithm of
OpenCV 4.2 (modules/calib3d/src/fundam.cpp run7Point / FMEstimatorCallback, ptsetreg.cpp
RANSACPointSetRegistrator, core's cv::RNG and solveCubic): the raw-pixel 7-point solver without the
Hartley normalisation later releases added.  OpenCV is neither vendored in the reference nor present
here, so parity with the reference's binary is UNPINNED: this file is a restatement, not a recording.

  inputs      pixel pairs rounded to float (cv::Point2f); everything after that in double
  n < 7       no model, nothing rejected, n_inliers = -1 (OpenCV leaves the mask unallocated)
  n == 7      the 7-point solver directly, mask all ones, no RANSAC
  n >= 8      RANSACPointSetRegistrator::run, modelPoints 7, threshold 3, confidence 0.99, maxIters 1000
  subsets     cv::RNG (multiply-with-carry, seed (uint64)-1), `% count`, 7 distinct indices, checkSubset
              (the last point collinear with a pair of earlier ones in either image) redraws the whole
              subset from the continuing stream, at most 10000 attempts per iteration
  solver      7x9 design matrix, two-dimensional null space, det(l G + H) = 0 with G = f1 - f2, H = f2,
              real roots (solveCubic), F33 = 1 when |F33| > DBL_EPSILON; a model with a non-finite
              entry is no model (dropped, the others keep their order)
  error       max(d1^2 s1, d2^2 s2) rounded to float, compared <= (float)(3 * 3)
  acceptance  in sequence: count > max(best, 6) replaces the best, then RANSACUpdateNumIters; no refit

The null space here is numpy's SVD; the models of a subset do not depend on the basis once F33 = 1, so a
product that eliminates instead compares at rounding level wherever the cubic's discriminant is away from 0.
Their ORDER does depend on it (the cubic's parameter is basis-dependent): it matters only when two models of one
iteration tie at the winning count, which `order_dependent` reports.
"""
import math

import numpy as np

MODEL_POINTS = 7
MAX_ATTEMPTS = 10000
DBL_EPSILON = 2.220446049250313e-16
FLT_EPSILON = 1.1920928955078125e-07
DBL_MIN = 2.2250738585072014e-308


class RNG:
    """cv::RNG: multiply-with-carry, as RANSACPointSetRegistrator::run seeds it"""

    def __init__(self, state=(1 << 64) - 1):
        self.state = state
        self.draws = 0

    def next(self):
        s = self.state
        s = ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32)) & 0xFFFFFFFFFFFFFFFF
        self.state = s
        self.draws += 1
        return s & 0xFFFFFFFF

    def uniform(self, count):
        return self.next() % count


def to_point2f(p):
    return np.asarray(p, np.float64).reshape(-1, 2).astype(np.float32).astype(np.float64)


def have_collinear(pts):
    """haveCollinearPoints(m, count): the LAST point against every pair of earlier ones"""
    i = len(pts) - 1
    for j in range(i):
        dx1 = pts[j][0] - pts[i][0]
        dy1 = pts[j][1] - pts[i][1]
        for k in range(j):
            dx2 = pts[k][0] - pts[i][0]
            dy2 = pts[k][1] - pts[i][1]
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def check_subset(p0, p1, idx):
    return not have_collinear(p0[idx]) and not have_collinear(p1[idx])


def get_subset(rng, count, model_points=MODEL_POINTS, p0=None, p1=None, max_attempts=MAX_ATTEMPTS):
    """getSubset: (indices or None, attempts that failed checkSubset).  p0 None: no subset check."""
    redrawn = 0
    for _ in range(max_attempts):
        idx = []
        for _i in range(model_points):
            v = rng.uniform(count)
            while v in idx:
                v = rng.uniform(count)
            idx.append(v)
        if p0 is not None and not check_subset(p0, p1, idx):
            redrawn += 1
            continue
        return idx, redrawn
    return None, redrawn


def subsets(count, iters, p0=None, p1=None, model_points=MODEL_POINTS, max_attempts=MAX_ATTEMPTS):
    """the subsets `iters` iterations draw: ([found][model_points] int32, redraws, raw draws consumed)"""
    if p0 is not None:
        p0, p1 = to_point2f(p0), to_point2f(p1)
    rng = RNG()
    out, redraws = [], 0
    for _ in range(iters):
        idx, r = get_subset(rng, count, model_points, p0, p1, max_attempts)
        redraws += r
        if idx is None:
            break
        out.append(idx)
    return np.asarray(out, np.int32).reshape(-1, model_points), redraws, rng.draws


def _det3(a, b, c):  # columns
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1]) + c[0] * (a[1] * b[2] - a[2] * b[1]))


def solve_cubic(c):
    """cv::solveCubic for c[0] x^3 + c[1] x^2 + c[2] x + c[3]: (roots, relative discriminant or None)"""
    a0, a1, a2, a3 = (float(v) for v in c)
    if a0 == 0:
        if a1 == 0:
            if a2 == 0:
                return [], None
            return [-a3 / a2], None
        d = a2 * a2 - 4 * a1 * a3
        if d < 0:
            return [], None
        d = math.sqrt(d)
        q1, q2 = (-a2 + d) * 0.5, (a2 + d) * -0.5
        if abs(q1) > abs(q2):
            r = [q1 / a1, a3 / q1]
        else:
            r = [q2 / a1, a3 / q2]
        return (r if d > 0 else r[:1]), None
    a0 = 1.0 / a0
    a1 *= a0
    a2 *= a0
    a3 *= a0
    Q = (a1 * a1 - 3 * a2) * (1.0 / 9)
    R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1.0 / 54)
    Qc = Q * Q * Q
    d = Qc - R * R
    rel = abs(d) / max(abs(Qc) + R * R, DBL_MIN)
    if d > 0:
        theta = math.acos(R / math.sqrt(Qc))
        t0 = -2 * math.sqrt(Q)
        t1 = theta * (1.0 / 3)
        t2 = a1 * (1.0 / 3)
        return [t0 * math.cos(t1) - t2, t0 * math.cos(t1 + 2 * math.pi / 3) - t2,
                t0 * math.cos(t1 + 4 * math.pi / 3) - t2], rel
    if d == 0:
        if R >= 0:
            x0 = -2 * R ** (1.0 / 3) - a1 / 3
            x1 = R ** (1.0 / 3) - a1 / 3
        else:
            x0 = 2 * (-R) ** (1.0 / 3) - a1 / 3
            x1 = -((-R) ** (1.0 / 3)) - a1 / 3
        return ([x0] if x0 == x1 else [x0, x1]), rel
    d = math.sqrt(-d)
    e = (d + abs(R)) ** (1.0 / 3)
    if R > 0:
        e = -e
    return [(e + Q / e) - a1 * (1.0 / 3)], rel


def seven_point(p0, p1):
    """run7Point on seven float-rounded pairs: ([k][9] models, relative discriminant of the cubic)"""
    p0, p1 = np.asarray(p0, np.float64).reshape(7, 2), np.asarray(p1, np.float64).reshape(7, 2)
    x0, y0, x1, y1 = p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1]
    A = np.stack([x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, np.ones(7)], axis=1)
    if not np.all(np.isfinite(A)):
        return np.zeros((0, 9)), None
    _, _, vt = np.linalg.svd(A, full_matrices=True)
    f1, f2 = vt[7], vt[8]
    G, H = (f1 - f2).reshape(3, 3), f2.reshape(3, 3)
    g, h = [G[:, k] for k in range(3)], [H[:, k] for k in range(3)]
    c = [_det3(g[0], g[1], g[2]),
         _det3(h[0], g[1], g[2]) + _det3(g[0], h[1], g[2]) + _det3(g[0], g[1], h[2]),
         _det3(g[0], h[1], h[2]) + _det3(h[0], g[1], h[2]) + _det3(h[0], h[1], g[2]),
         _det3(h[0], h[1], h[2])]
    roots, rel = solve_cubic(c)
    Gf, Hf = G.reshape(9), H.reshape(9)
    models = []
    for r in roots:
        lam, mu = r, 1.0
        s = Gf[8] * r + Hf[8]
        F = np.empty(9)
        if abs(s) > DBL_EPSILON:
            mu = 1.0 / s
            lam *= mu
            F[8] = 1.0
        else:
            F[8] = 0.0
        F[:8] = Gf[:8] * lam + Hf[:8] * mu
        if np.all(np.isfinite(F)):
            models.append(F)
    return np.asarray(models, np.float64).reshape(-1, 9), rel


def errors_f64(F, p0, p1):
    """FMEstimatorCallback::computeError before the rounding to float"""
    x0, y0, x1, y1 = p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1]
    with np.errstate(all="ignore"):
        a = F[0] * x0 + F[1] * y0 + F[2]
        b = F[3] * x0 + F[4] * y0 + F[5]
        c = F[6] * x0 + F[7] * y0 + F[8]
        s2 = 1.0 / (a * a + b * b)
        d2 = x1 * a + y1 * b + c
        a = F[0] * x1 + F[3] * y1 + F[6]
        b = F[1] * x1 + F[4] * y1 + F[7]
        c = F[2] * x1 + F[5] * y1 + F[8]
        s1 = 1.0 / (a * a + b * b)
        d1 = x0 * a + y0 * b + c
        return np.maximum(d1 * d1 * s1, d2 * d2 * s2)


def errors(F, p0, p1):
    with np.errstate(all="ignore"):
        return errors_f64(F, p0, p1).astype(np.float32)


def update_num_iters(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters"""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))  # cvRound: to nearest even


def find_fundamental(points0, points1, threshold=3.0, confidence=0.99, max_iters=1000, trace=False,
                     max_attempts=MAX_ATTEMPTS):
    """dict(mask uint8 [n], n_inliers, hypotheses, F [9] or None, trace, redraws, order_dependent = the
    winning model tied with another of its iteration).  trace: one dict per iteration
    evaluated (subset, models, counts, disc = relative discriminant, margin = the smallest relative distance of
    a (model, correspondence) error from the threshold, accepted = the model index taken or -1)."""
    p0, p1 = to_point2f(points0), to_point2f(points1)
    n = len(p0)
    res = dict(mask=np.ones(n, np.uint8), n_inliers=-1, hypotheses=0, F=None, trace=[], redraws=0,
               order_dependent=False)
    if n < MODEL_POINTS:
        return res
    thr = np.float32(threshold * threshold)

    def note(idx, models, rel):
        rec = dict(subset=list(idx), models=models, disc=rel, counts=[], margin=np.inf, accepted=-1)
        for F in models:
            e64 = errors_f64(F, p0, p1)
            with np.errstate(all="ignore"):
                rec["counts"].append(int(np.count_nonzero(e64.astype(np.float32) <= thr)))
                m = np.abs(e64 - float(thr)) / float(thr)
            m = m[np.isfinite(m)]
            if len(m):
                rec["margin"] = min(rec["margin"], float(m.min()))
        return rec

    if n == MODEL_POINTS:
        models, rel = seven_point(p0, p1)
        res["hypotheses"] = 1
        if trace:
            res["trace"].append(note(range(7), models, rel))
        if len(models):
            res["n_inliers"] = 7
            res["F"] = models[0].copy()
        return res
    rng = RNG()
    niters, best, it = max_iters, 0, 0
    best_mask = None
    while it < niters:
        idx, r = get_subset(rng, n, MODEL_POINTS, p0, p1, max_attempts)
        res["redraws"] += r
        if idx is None:
            break
        models, rel = seven_point(p0[idx], p1[idx])
        rec = note(idx, models, rel) if trace else None
        goods = [int(np.count_nonzero(errors(F, p0, p1) <= thr)) for F in models]
        for k, F in enumerate(models):
            mask = errors(F, p0, p1) <= thr
            good = goods[k]
            if good > max(best, MODEL_POINTS - 1):
                # the order of an iteration's models follows the null-space basis: it decides only between
                # two models of one iteration that tie at an accepted count
                res["order_dependent"] = goods.count(good) > 1  # (of the LAST acceptance: the result's)
                best, best_mask = good, mask
                res["F"] = F.copy()
                niters = update_num_iters(confidence, (n - good) / n, MODEL_POINTS, niters)
                if rec is not None:
                    rec["accepted"] = k
        if rec is not None:
            res["trace"].append(rec)
        it += 1
    res["hypotheses"] = it
    if best > 0:
        res["mask"] = best_mask.astype(np.uint8)
        res["n_inliers"] = best
    return res


def normalized(F):
    """F / ||F|| with the sign of its largest entry positive"""
    F = np.asarray(F, np.float64).reshape(9)
    F = F / np.linalg.norm(F)
    return F if F[np.argmax(np.abs(F))] > 0 else -F
