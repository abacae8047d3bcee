"""Generators of the local map tracking tests (tests/test_lmap_cpu.py, tests/test_gpu_lmap.py): frames and local maps
in tests/lmap_ref.py's format, each built so that the restatement reaches the decision the case is named after.
A case that is NOT built to sit on a boundary asserts here, on the CPU, that every decision margin of the
restatement (depth, image bounds, box sides, best against 0.35 and 0.6 * second) exceeds 1e-9; the boundary cases
use exactly representable values (identity pose, fx = fy = 256, depth 2) and assert that the restatement lands on
the boundary."""
import numpy as np

import lmap_ref as LR

W, H = 512, 384                                  # 64 / W = 48 / H = 0.125: the grid's scale is exact
CAM = (256.0, 256.0, 256.0, 192.0, 32.0)         # fx fy cx cy bf, powers of two around the centre
Z = 2.0
MARGIN = 1e-9


def same_bits(got, want):
    """two search results (dicts of status, best_idx, best, second) are equal, the doubles bit for bit"""
    for k in ("status", "best_idx"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("best", "second"):  # compared as integers
        np.testing.assert_array_equal(np.asarray(got[k]).view(np.int64), np.asarray(want[k]).view(np.int64), err_msg=k)


def unit(rng, n=None):
    v = rng.normal(size=(256,) if n is None else (n, 256))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def at_distance(d, dist, rng):
    """a unit descriptor at descriptor distance ~dist from the unit descriptor d (dist = 2 (1 - cos))"""
    e = rng.normal(size=256)
    e -= e.dot(d) * d
    e /= np.linalg.norm(e)
    c = 1.0 - dist / 2.0
    return c * d + np.sqrt(max(0.0, 1.0 - c * c)) * e


def pixel_point(u, v, z=Z, Twc=None, cam=CAM):
    """the world point that projects to (u, v) at depth z (exactly, for the identity pose and CAM)"""
    fx, fy, cx, cy, _ = cam
    pc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
    if Twc is None:
        return pc
    return Twc[:3, :3] @ pc + Twc[:3, 3]


class Scene:
    """one frame and one local map under construction"""

    def __init__(self, seed=0, Twc=None, cam=CAM, stereo=False, width=W, height=H):
        self.rng = np.random.default_rng(seed)
        self.Twc = np.eye(4) if Twc is None else np.asarray(Twc, np.float64)
        self.cam, self.stereo, self.width, self.height = cam, stereo, width, height
        self.kp, self.pts, self.expect = [], [], {}

    def keypoint(self, x, y, desc=None, ur=-1.0, pid=-1, xyz=(0.0, 0.0, 0.0)):
        self.kp.append((x, y, unit(self.rng) if desc is None else desc, ur, pid, xyz))
        return len(self.kp) - 1

    def point(self, pid, pos, desc=None, expect=None, idx=None):
        self.pts.append((pid, np.asarray(pos, np.float64), unit(self.rng) if desc is None else desc))
        if expect is not None:
            self.expect[len(self.pts) - 1] = (expect, idx)
        return len(self.pts) - 1

    def at(self, u, v, z=Z):
        return pixel_point(u, v, z, None if np.array_equal(self.Twc, np.eye(4)) else self.Twc, self.cam)

    def build(self, boundary=False):
        n1, n = len(self.kp), len(self.pts)
        F = np.zeros((n1, 259))
        ur, pid, xyz = np.full(n1, -1.0), np.full(n1, -1, np.int32), np.zeros((n1, 3))
        for i, (x, y, d, r, p, q) in enumerate(self.kp):
            F[i, 0], F[i, 1], F[i, 2], F[i, 3:] = 0.5, x, y, d
            ur[i], pid[i], xyz[i] = r, p, q
        fr = dict(features=F, u_right=ur if self.stereo else None, point_id=pid, point_xyz=xyz, Twc=self.Twc,
                  cam=self.cam, width=self.width, height=self.height)
        lm = dict(ids=np.array([p[0] for p in self.pts], np.int32),
                  pos=np.array([p[1] for p in self.pts], np.float64).reshape(-1, 3),
                  desc=np.array([p[2] for p in self.pts], np.float64).reshape(-1, 256))
        res = LR.search(fr, lm)
        for p, (st, idx) in self.expect.items():
            assert res["status"][p] == st, (p, res["status"][p], st)
            assert idx is None or res["best_idx"][p] == idx, (p, res["best_idx"][p], idx)
        if not boundary:
            m = LR.margins(fr, lm)
            assert m > MARGIN, f"a decision of this case sits {m} from its threshold"
        return fr, lm


def random_pose(rng):
    from rspl_slam_amd import synthetic as SY
    T = np.eye(4)
    T[:3, :3] = SY._rotvec_to_R(rng.normal(0, 0.1, 3))
    T[:3, 3] = rng.normal(0, 1.0, 3)
    return T


def random_scene(n_kp, n_local, seed, stereo=False, hold=0.1, cam=(458.654, 457.296, 367.215, 248.375, 50.0),
                 width=752, height=480):
    """n_kp keypoints on quarter pixels under a random pose, n_local local points: most of them project near a
    keypoint and carry a noisy copy of its descriptor, the rest anywhere (also behind the camera and off the
    image); `hold` of the keypoints hold a point already, some of them one of the local map's."""
    rng = np.random.default_rng(seed)
    s = Scene(seed + 1000, random_pose(rng), cam, stereo, width, height)
    for i in range(n_kp):
        x, y = np.round(rng.uniform(1, width - 1) * 4) / 4, np.round(rng.uniform(1, height - 1) * 4) / 4
        held = rng.uniform() < hold
        # a held keypoint holds either a point outside the local map or (every other one) local point `i % n_local`
        pid = (10000 + i if (i % 2 or n_local == 0) else 100 + i % n_local) if held else -1
        ur = x - rng.uniform(2, 40) if (stereo and rng.uniform() < 0.6) else -1.0
        s.keypoint(x, y, ur=ur, pid=pid, xyz=rng.normal(size=3))
    for p in range(n_local):
        k = rng.uniform()
        if n_kp and k < 0.75:
            i = int(rng.integers(n_kp))
            x, y, d, ur = s.kp[i][:4]
            z = rng.uniform(2, 10)
            if stereo and ur > 0 and rng.uniform() < 0.7:
                z = cam[4] / (x - ur)  # consistent with the keypoint's disparity
            pos = s.at(x + rng.uniform(-10, 10), y + rng.uniform(-10, 10), z)
            s.point(100 + p, pos, at_distance(d, rng.uniform(0.02, 0.5), rng))
        elif k < 0.85:
            s.point(100 + p, s.at(rng.uniform(0, width), rng.uniform(0, height), -rng.uniform(1, 5)))
        else:
            s.point(100 + p, s.at(rng.uniform(-200, width + 200), rng.uniform(-200, height + 200), rng.uniform(2, 10)))
    return s.build()


# ---- the designed cases: name -> (frame, local map, boundary) -------------------------------------------------
def geometry():
    s = Scene(1)
    d = unit(s.rng)
    k = s.keypoint(100.0, 100.0, at_distance(d, 0.1, s.rng))
    s.point(1, [0.1, 0.1, 0.0], expect=LR.BEHIND)                     # z exactly 0
    s.point(2, [0.1, 0.1, -3.0], expect=LR.BEHIND)
    s.point(3, s.at(0.0, 100.0), expect=LR.OFF_IMAGE)                 # u = 0
    s.point(4, s.at(float(W), 100.0), expect=LR.OFF_IMAGE)            # u = W
    s.point(5, s.at(100.0, 0.0), expect=LR.OFF_IMAGE)                 # v = 0
    s.point(6, s.at(100.0, float(H)), expect=LR.OFF_IMAGE)            # v = H
    s.point(7, s.at(0.5, 0.5), expect=LR.NO_CANDIDATE)                # just inside
    s.point(8, s.at(100.0 - 15.0, 100.0), d, expect=LR.NO_CANDIDATE)  # the keypoint at exactly u + 15: rejected
    s.point(9, s.at(100.0, 100.0 + 15.0), d, expect=LR.NO_CANDIDATE)  # ... at exactly v - 15
    s.point(10, s.at(100.0 - 14.75, 100.0 + 14.75), d, expect=LR.GOOD, idx=k)  # just inside both
    fr, lm = s.build(boundary=True)
    for p, (u, v) in {2: (0.0, 100.0), 3: (float(W), 100.0), 4: (100.0, 0.0), 5: (100.0, float(H)), 7: (85.0, 100.0),
                      8: (100.0, 115.0)}.items():
        st, pu, pv, _, _ = LR.project(fr["Twc"], fr["cam"], lm["pos"][p])
        assert (pu, pv) == (u, v), (p, pu, pv)  # the restatement lands on the boundary exactly
    assert LR.project(fr["Twc"], fr["cam"], lm["pos"][0])[4] == 0.0
    return fr, lm


def stereo_gate(stereo=True):
    """with u_right: xr > 0 against stereo and mono (-1) keypoints, and xr <= 0; without: the term is skipped"""
    s = Scene(2, stereo=stereo)
    d = [unit(s.rng) for _ in range(4)]
    # xr = u - bf / z = u - 16 at depth 2
    a = s.keypoint(200.0, 100.0, at_distance(d[0], 0.1, s.rng), ur=186.0)   # dxr = 2: passes
    b = s.keypoint(200.0, 200.0, at_distance(d[1], 0.1, s.rng), ur=150.0)   # dxr = -34: fails with u_right
    c = s.keypoint(200.0, 300.0, at_distance(d[2], 0.1, s.rng), ur=-1.0)    # mono: dxr = -185 fails with u_right
    e = s.keypoint(10.0, 50.0, at_distance(d[3], 0.1, s.rng), ur=-1.0)      # xr = 10 - 16 <= 0: dxr = 0 passes
    s.point(1, s.at(200.0, 100.0), d[0], expect=LR.GOOD, idx=a)
    s.point(2, s.at(200.0, 200.0), d[1], expect=LR.NO_CANDIDATE if stereo else LR.GOOD, idx=None if stereo else b)
    s.point(3, s.at(200.0, 300.0), d[2], expect=LR.NO_CANDIDATE if stereo else LR.GOOD, idx=None if stereo else c)
    s.point(4, s.at(10.0, 50.0), d[3], expect=LR.GOOD, idx=e)
    return s.build()


def filters():
    s = Scene(3)
    d = [unit(s.rng) for _ in range(3)]
    s.keypoint(100.0, 100.0, at_distance(d[0], 0.05, s.rng), pid=77, xyz=(1.0, 2.0, 3.0))  # occupied: skipped
    k1 = s.keypoint(104.0, 100.0, at_distance(d[0], 0.2, s.rng))
    s.keypoint(300.0, 100.0, at_distance(d[1], 0.05, s.rng), pid=5, xyz=(0.5, 0.5, 4.0))   # holds local point 5
    k3 = s.keypoint(300.0, 300.0, at_distance(d[2], 0.1, s.rng))
    s.point(1, s.at(100.0, 100.0), d[0], expect=LR.GOOD, idx=k1)      # the better, occupied keypoint is not visited
    s.point(5, s.at(300.0, 104.0), d[1], expect=LR.NOT_SELECTED)      # the frame already holds it
    s.point(0, s.at(300.0, 300.0), d[2], expect=LR.GOOD, idx=k3)      # a point whose id is 0
    return s.build()


def selection():
    s = Scene(4)
    d = [unit(s.rng) for _ in range(6)]
    k0 = s.keypoint(40.0, 40.0, at_distance(d[0], 0.1, s.rng))
    s.point(1, s.at(40.0, 40.0), d[0], expect=LR.GOOD, idx=k0)        # one candidate: second stays 4.0
    s.keypoint(140.0, 40.0, at_distance(d[1], 0.35 + 1e-6, s.rng))
    s.point(2, s.at(140.0, 40.0), d[1], expect=LR.FAILED)             # best just above 0.35
    k2 = s.keypoint(240.0, 40.0, at_distance(d[2], 0.35 - 1e-6, s.rng))
    s.point(3, s.at(240.0, 40.0), d[2], expect=LR.GOOD, idx=k2)       # ... just below
    k3 = s.keypoint(40.0, 140.0, at_distance(d[3], 0.12, s.rng))
    s.keypoint(44.0, 140.0, at_distance(d[3], 0.12 / 0.6 - 1e-6, s.rng))
    s.point(4, s.at(42.0, 140.0), d[3], expect=LR.FAILED, idx=k3)     # best just above 0.6 * second
    k5 = s.keypoint(140.0, 140.0, at_distance(d[4], 0.12, s.rng))
    s.keypoint(144.0, 140.0, at_distance(d[4], 0.12 / 0.6 + 1e-6, s.rng))
    s.point(5, s.at(142.0, 140.0), d[4], expect=LR.GOOD, idx=k5)      # ... just below
    # 70 keypoints in one box: more than a ballot's 64 candidates, the best one late
    cl = [s.keypoint(300.0 + (i % 10), 250.0 + i // 10, at_distance(d[5], 0.3 + 0.002 * i, s.rng)) for i in range(69)]
    kb = s.keypoint(305.0, 257.0, at_distance(d[5], 0.1, s.rng))
    s.point(6, s.at(304.0, 253.0), d[5], expect=LR.GOOD, idx=kb)
    fr, lm = s.build()
    res = LR.search(fr, lm)
    assert res["second"][0] == 4.0 and len(LR.neighbors_brute(fr, 304.0, 253.0, 0.0)) == 70 and kb == cl[-1] + 1
    return fr, lm


def ties():
    s = Scene(5)
    d = [unit(s.rng) for _ in range(2)]
    same = at_distance(d[0], 0.1, s.rng)
    # tie 1: identical descriptors; index 1 sits in the lower gx (cell width 8 px), so the grid walk meets it first
    s.keypoint(110.0, 100.0, same)           # gx = round(13.75) = 14
    k1 = s.keypoint(98.0, 100.0, same)       # gx = round(12.25) = 12
    s.point(1, s.at(104.0, 100.0), d[0], expect=LR.FAILED, idx=k1)    # best == second: the ratio test fails, idx = 1
    # tie 2: both in one cell: the lower index wins
    same2 = at_distance(d[1], 0.1, s.rng)
    k2 = s.keypoint(301.0, 200.0, same2)     # gx = round(37.625) = 38
    s.keypoint(303.0, 200.0, same2)          # gx = round(37.875) = 38
    s.point(2, s.at(302.0, 200.0), d[1], expect=LR.FAILED, idx=k2)
    fr, lm = s.build(boundary=True)
    assert LR.cell(110.0, 100.0, W, H)[0] > LR.cell(98.0, 100.0, W, H)[0]
    assert LR.cell(301.0, 200.0, W, H) == LR.cell(303.0, 200.0, W, H)
    res = LR.search(fr, lm)
    assert res["best"][0] == res["second"][0] and res["best"][1] == res["second"][1]
    return fr, lm


def merge_claims():
    """two and three points claim one keypoint (the last in list order wins); the good list is in local order"""
    s = Scene(6)
    d = [unit(s.rng) for _ in range(3)]
    ka = s.keypoint(100.0, 100.0, d[0])
    kb = s.keypoint(300.0, 100.0, d[1])
    kc = s.keypoint(300.0, 300.0, d[2])
    s.point(11, s.at(300.0, 301.0), at_distance(d[2], 0.05, s.rng), expect=LR.GOOD, idx=kc)
    s.point(12, s.at(101.0, 100.0), at_distance(d[0], 0.05, s.rng), expect=LR.GOOD, idx=ka)
    s.point(13, s.at(301.0, 100.0), at_distance(d[1], 0.05, s.rng), expect=LR.GOOD, idx=kb)
    s.point(14, s.at(100.0, 101.0), at_distance(d[0], 0.07, s.rng), expect=LR.GOOD, idx=ka)
    s.point(15, s.at(300.0, 101.0), at_distance(d[1], 0.07, s.rng), expect=LR.GOOD, idx=kb)
    s.point(16, s.at(99.0, 100.0), at_distance(d[0], 0.02, s.rng), expect=LR.GOOD, idx=ka)
    fr, lm = s.build()
    kp, pt = LR.good_list(LR.search(fr, lm))
    assoc, winner = LR.merge(fr, lm, kp, pt)
    assert list(pt) == [0, 1, 2, 3, 4, 5] and list(assoc) == [16, 15, 11] and list(winner) == [5, 4, 0]
    return fr, lm


DESIGNED = dict(geometry=geometry, stereo=stereo_gate, mono=lambda: stereo_gate(False), filters=filters,
                selection=selection, ties=ties, merge=merge_claims)
# (keypoints, local points): the chunk / ballot boundaries against the partial last block of four waves
SIZES = [(0, 5), (1, 1), (63, 4), (64, 5), (65, 65), (130, 65), (130, 0), (64, 1), (130, 4)]


def chain_scene(seed=7, n_kp=250, n_own=6, n_local=200):
    """A noise-free frame at a known pose that holds `n_own` points of its own -- too few for the tracking step --
    and a local map of which `n_local` points project exactly onto free keypoints, with descriptors near theirs.
    -> (frame, local map, ground truth T_wc, last T_wc)"""
    from rspl_slam_amd import synthetic as SY
    rng = np.random.default_rng(seed)
    cam, width, height = (458.654, 457.296, 367.215, 248.375, 50.0), 752, 480
    gt = random_pose(rng)
    s = Scene(seed + 1, gt, cam, False, width, height)
    # keypoints on a jittered lattice, more than 2 r apart: one candidate per point
    xs, ys = np.meshgrid(np.arange(20, width - 20, 34.0), np.arange(20, height - 20, 34.0))
    cells = rng.permutation(len(xs.ravel()))[:n_kp]
    for c in cells:
        s.keypoint(xs.ravel()[c] + rng.uniform(-1, 1), ys.ravel()[c] + rng.uniform(-1, 1))
    order = rng.permutation(n_kp)
    for j, i in enumerate(order[:n_own]):
        x, y, d = s.kp[i][:3]
        s.kp[i] = (x, y, d, -1.0, 5000 + j, tuple(s.at(x, y, rng.uniform(2, 15))))
    for j, i in enumerate(order[n_own:n_own + n_local]):
        x, y, d = s.kp[i][:3]
        s.point(200 + j, s.at(x, y, rng.uniform(2, 15)), at_distance(d, rng.uniform(0.02, 0.2), rng), expect=LR.GOOD, idx=i)
    for j in range(20):  # and some that land nowhere near a keypoint or outside
        s.point(900 + j, s.at(rng.uniform(-300, width + 300), rng.uniform(-300, height + 300), rng.uniform(2, 15)))
    fr, lm = s.build()
    # the search projects with a pose a little off the truth (the last frame's), as tracking would
    last = gt.copy()
    last[:3, :3] = SY._rotvec_to_R(rng.normal(0, 0.002, 3)) @ gt[:3, :3]
    last[:3, 3] += rng.normal(0, 0.01, 3)
    fr = dict(fr, Twc=last)
    assert LR.margins(fr, lm) > MARGIN
    return fr, lm, gt, last


def batch_scenes(seed=11, n_local=65, counts=(130, 63, 1), stereo=(False, True, False)):
    """one local map seen by len(counts) frames with different poses, keypoint counts and u_right arrays
    -> ([frame], local map)"""
    from rspl_slam_amd import synthetic as SY
    rng = np.random.default_rng(seed)
    cam, width, height = (458.654, 457.296, 367.215, 248.375, 50.0), 752, 480
    base = random_pose(rng)
    pos = np.array([pixel_point(rng.uniform(-100, width + 100), rng.uniform(-100, height + 100), rng.uniform(2, 12),
                                base, cam) for _ in range(n_local)])
    lm = dict(ids=np.arange(300, 300 + n_local, dtype=np.int32), pos=pos, desc=unit(rng, n_local))
    frames = []
    for n_kp, st in zip(counts, stereo):
        T = base.copy()
        T[:3, :3] = SY._rotvec_to_R(rng.normal(0, 0.03, 3)) @ base[:3, :3]
        T[:3, 3] += rng.normal(0, 0.2, 3)
        s = Scene(seed + n_kp, T, cam, st, width, height)
        vis = [p for p in range(n_local) if LR.project(T, cam, pos[p])[0] == LR.GOOD and
               LR.in_image(*LR.project(T, cam, pos[p])[1:3], width, height)]
        for i in range(n_kp):
            if i < len(vis) and i % 4 != 3:  # near a local point's projection, with a descriptor near its own
                _, u, v, xr, _ = LR.project(T, cam, pos[vis[i]])
                x, y = np.round((u + rng.uniform(-8, 8)) * 4) / 4, np.round((v + rng.uniform(-8, 8)) * 4) / 4
                ur = xr + rng.uniform(-5, 5) if (st and xr > 1 and i % 3) else -1.0
                s.keypoint(x, y, at_distance(lm["desc"][vis[i]], rng.uniform(0.02, 0.5), rng), ur=ur,
                           pid=int(lm["ids"][vis[i]]) if i % 7 == 5 else -1, xyz=pos[vis[i]])
            else:
                s.keypoint(np.round(rng.uniform(1, width - 1) * 4) / 4, np.round(rng.uniform(1, height - 1) * 4) / 4)
        s.pts = [(int(lm["ids"][p]), pos[p], lm["desc"][p]) for p in range(n_local)]
        frames.append(s.build()[0])
    return frames, lm
