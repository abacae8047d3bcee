"""Small local-BA windows for the call-frame tests (test_ba_pair_offsets_cpu.py, test_gpu_ba_frame.py): seeded
synthetic problems (real geometry, so the BA runs on them) cut to an exact landmark count and then bent into the
shapes the edge-pair lists and the final kernel can go wrong at."""
import numpy as np

from rspl_slam_amd import synthetic as SY
from rspl_slam_amd.ba_types import DenseProblem

KINDS = (("mono", 2), ("stereo", 3), ("mono_line", 4), ("stereo_line", 8))
# the handle every case fits (LocalBA(*CAPS)); the host-only hook is given the same capacities
CAPS = dict(max_poses=16, max_points=2048, max_lines=64, max_edges=32768)
MAX_LANDMARKS = CAPS["max_points"] + CAPS["max_lines"]


def rebuild(p, edges, pose_fixed=None, nq=None, nl=None):
    nq = p.points.shape[0] if nq is None else nq
    nl = p.lines.shape[0] if nl is None else nl
    return DenseProblem(cameras=p.cameras, pose_q=p.pose_q, pose_p=p.pose_p,
                        pose_fixed=p.pose_fixed if pose_fixed is None else pose_fixed, points=p.points[:nq],
                        lines=p.lines[:nl], cfg=p.cfg, iterations_first=p.iterations_first,
                        iterations_second=p.iterations_second, **edges)


def edges_of(p):
    return {k: {f: getattr(p, k)[f].copy() for f in ("pose", "lm", "cam", "obs")} for k, _ in KINDS}


def select(ed, kind, mask):
    ed[kind] = {f: a[mask] for f, a in ed[kind].items()}


def window(n_landmarks, n_opt, seed, n_lines=2, points=True):
    """n_landmarks landmarks (the last min(n_lines, ...) of them lines; points=False: lines only), n_opt optimised
    poses + one fixed, every pose observing"""
    n_poses = n_opt + 1
    nl = n_landmarks if not points else min(n_lines, n_landmarks - 1)
    nq = n_landmarks - nl
    p, _ = SY.ba_problem(n_poses=n_poses, n_points=2 * nq + 16, n_lines=4 * nl + 4, obs_per_point=n_poses, seed=seed,
                         pixel_sigma=0.8, outlier_frac=0.05)
    assert p.points.shape[0] >= nq and p.lines.shape[0] >= nl, "generator kept too few landmarks"
    ed = edges_of(p)
    for k in ("mono", "stereo"):
        select(ed, k, ed[k]["lm"] < nq)
    for k in ("mono_line", "stereo_line"):
        select(ed, k, ed[k]["lm"] < nl)
    return rebuild(p, ed, nq=nq, nl=nl)


def landmark_edges(p, g):
    """(kind, index) of the edges of landmark g (points first, then lines)"""
    nq = p.points.shape[0]
    kinds = ("mono", "stereo") if g < nq else ("mono_line", "stereo_line")
    lm = g if g < nq else g - nq
    return [(k, int(i)) for k in kinds for i in np.flatnonzero(getattr(p, k)["lm"] == lm)]


def with_edges(p, g, n, rng):
    """landmark g with exactly n edges: its own repeated (jittered observations: several edges on one pose)"""
    have = landmark_edges(p, g)
    assert have
    ed = edges_of(p)
    if len(have) > n:
        for k in {k for k, _ in have}:
            drop = [i for kk, i in have[n:] if kk == k]
            m = np.ones(ed[k]["lm"].shape[0], bool)
            m[drop] = False
            select(ed, k, m)
    for j in range(max(0, n - len(have))):
        k, i = have[j % len(have)]
        src = getattr(p, k)
        ed[k]["pose"] = np.append(ed[k]["pose"], src["pose"][i])
        ed[k]["lm"] = np.append(ed[k]["lm"], src["lm"][i])
        ed[k]["cam"] = np.append(ed[k]["cam"], src["cam"][i])
        ed[k]["obs"] = np.vstack([ed[k]["obs"], src["obs"][i] + rng.normal(0, 0.3, src["obs"][i].shape)])
    return rebuild(p, ed)


def without_landmark(p, g):
    """landmark g left without any edge (inactive)"""
    ed = edges_of(p)
    nq = p.points.shape[0]
    for k in (("mono", "stereo") if g < nq else ("mono_line", "stereo_line")):
        select(ed, k, ed[k]["lm"] != (g if g < nq else g - nq))
    return rebuild(p, ed)


def apart(p, pa, pb):
    """no landmark observed by both pose pa and pose pb: pb's edges leave pa's landmarks"""
    ed = edges_of(p)
    for kinds in (("mono", "stereo"), ("mono_line", "stereo_line")):
        seen = np.concatenate([ed[k]["lm"][ed[k]["pose"] == pa] for k in kinds])
        for k in kinds:
            select(ed, k, ~((ed[k]["pose"] == pb) & np.isin(ed[k]["lm"], seen)))
    return rebuild(p, ed)


def shuffled(p, rng):
    """the caller's edge order of every type permuted"""
    ed = edges_of(p)
    for k, _ in KINDS:
        select(ed, k, rng.permutation(ed[k]["lm"].shape[0]))
    return rebuild(p, ed)


def with_total_edges(p, n, rng):
    """exactly n edges in all (n >= 4: every type present when the window has all four), caller order shuffled"""
    ed = edges_of(p)
    total = sum(ed[k]["lm"].shape[0] for k, _ in KINDS)
    assert total >= n
    kinds = [k for k, _ in KINDS if ed[k]["lm"].shape[0]]
    keep = {k: (1 if n >= len(kinds) else 0) for k in kinds}
    if n < len(kinds):
        for k in kinds[:n]:
            keep[k] = 1
    left = n - sum(keep.values())
    while left:
        for k in kinds:
            if left and keep[k] < ed[k]["lm"].shape[0]:
                keep[k] += 1
                left -= 1
    for k in kinds:
        select(ed, k, np.sort(rng.permutation(ed[k]["lm"].shape[0])[:keep[k]]))
    return shuffled(rebuild(p, ed), rng)


def n_edges(p):
    return sum(p.n_edges(k) for k, _ in KINDS)


def structure_cases():
    """(name, problem) for the edge-pair list tests"""
    rng = np.random.default_rng(7)
    out = []
    for K in (1, 2, 10):
        for nL in (1, 63, 64, 65, 255, 256, 257):
            out.append((f"nL{nL}-K{K}", window(nL, K, seed=1000 * K + nL)))
    wide = window(300, 12, seed=5)  # 12 optimised poses, 2 landmark ranges: diagonal sub-chunks (dsub > 1)
    out.append(("wide-dsub", wide))
    base = window(130, 10, seed=11)
    out.append(("edges9", with_edges(base, 3, 9, rng)))
    out.append(("edges17", with_edges(with_edges(base, 70, 17, rng), 129, 9, rng)))  # (a point and a line landmark)
    out.append(("twice-on-a-pose", with_edges(window(65, 2, seed=12), 1, 5, rng)))
    out.append(("inactive", without_landmark(without_landmark(base, 0), 64)))
    fixed2 = base.pose_fixed.copy()
    fixed2[3] = 1  # a second fixed pose, with edges
    out.append(("fixed-pose-edges", rebuild(base, edges_of(base), pose_fixed=fixed2)))
    out.append(("empty-chunk", apart(window(257, 10, seed=13), 1, 10)))
    out.append(("lines-only", window(20, 4, seed=14, points=False)))
    out.append(("shuffled", shuffled(window(257, 10, seed=15), rng)))
    return out
