"""numpy restatement of the global descriptor search (relocalisation).  The reference has no such
stage -- its tracking gives up for good (src/map_builder.cc:218-225) -- so this file IS the contract:

  D[i][p] = 2 (1 - q_i . d_p)      lmap_ref.distance, the fixed summation order
  per keypoint i, p ascending with lmap::Best's rule and a constant key (strict <: a tie keeps the lowest p):
      best, arg, second (the second smallest value; 4.0 where nothing is below it; arg -1 without candidates)
  per local point p: kbest, the lowest i that attains min_i D[i][p] (-1 when n1 = 0)
  pass:   best < max_distance and best < max_ratio * second
  match:  pass and (mutual == 0 or kbest[arg] == i)
  the matches compacted in ascending keypoint order: keypoint, local index, id, position, keypoint (x, y)

A table is a dict ids [n], pos [n, 3], desc [n, 256] (lmap_ref's local map); features is [n1, 259]."""
import numpy as np

import lmap_ref as LR

MAX_DISTANCE, MAX_RATIO = 0.35, 0.6


def distances(features, lm):
    F = np.asarray(features, np.float64).reshape(-1, 259)
    desc = np.asarray(lm["desc"], np.float64).reshape(-1, 256)
    D = np.zeros((len(F), len(desc)))
    if len(desc):
        for i in range(len(F)):
            D[i] = LR.distance(F[i, 3:], desc)
    return D


def search(features, lm, max_distance=MAX_DISTANCE, max_ratio=MAX_RATIO, mutual=True, D=None):
    F = np.asarray(features, np.float64).reshape(-1, 259)
    D = distances(F, lm) if D is None else D
    n1, nl = D.shape
    # a value not below 4.0 is no candidate (Best starts from 4.0 and compares strictly)
    C = np.concatenate([np.where(D < 4.0, D, 4.0), np.full((n1, 2), 4.0)], axis=1)
    two = np.sort(C, axis=1)[:, :2]
    best, second = two[:, 0].copy(), two[:, 1].copy()
    arg = np.where(best < 4.0, np.argmin(C, axis=1), -1).astype(np.int32)  # argmin: the first of equal values
    kbest = (np.argmin(D, axis=0) if n1 else np.full(nl, -1)).astype(np.int32)
    passed = (arg >= 0) & (best < max_distance) & (best < max_ratio * second)
    match = np.full(n1, -1, np.int32)
    for i in np.flatnonzero(passed):
        if not mutual or kbest[arg[i]] == i:
            match[i] = arg[i]
    kp = np.flatnonzero(match >= 0).astype(np.int32)
    loc = match[kp]
    return dict(n_keypoints=n1, n_local=nl, n_pass=int(passed.sum()), n_matched=len(kp), arg=arg, best=best,
                second=second, match=match, kbest=kbest, match_kp=kp, match_local=loc,
                match_id=np.asarray(lm["ids"], np.int32)[loc],
                match_pos=np.asarray(lm["pos"], np.float64).reshape(-1, 3)[loc], match_xy=F[kp, 1:3])


def margins(features, lm, max_distance=MAX_DISTANCE, max_ratio=MAX_RATIO, D=None):
    """the smallest distance of any decision from its threshold: best to second per keypoint, the two smallest values
    per local point, |best - max_distance|, |best - max_ratio second|"""
    D = distances(features, lm) if D is None else D
    n1, nl = D.shape
    if n1 == 0 or nl == 0:
        return np.inf
    r = search(features, lm, max_distance, max_ratio, D=D)
    m = [np.min(r["second"] - r["best"]), np.min(np.abs(r["best"] - max_distance)),
         np.min(np.abs(r["best"] - max_ratio * r["second"]))]
    if n1 > 1:
        col = np.sort(D, axis=0)
        m.append(np.min(col[1] - col[0]))
    return float(min(m))
