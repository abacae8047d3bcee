"""CPU-side checks of local map tracking (rspl_lmap_*, rspl_map_reference_keyframe, rspl_map_local_mappoints): the
boundary is declared and bound; the numpy restatement (tests/lmap_ref.py) is checked against itself -- the grid walk
against the plain box, the tie rule against the walk's first-visited winner, the fixed-order distance against
np.dot; the library's host entry points equal the restatement -- rspl_lmap_debug_search_host bit for bit on every
case the GPU tests run, the two map functions on hand-built graphs; and the bank / local-table bookkeeping of a
host-only handle reports its errors.  No GPU needed.

Parity is with this project's restatement: the reference never calls this code, and it cannot be built here.
One listed case has no native counterpart: the map's API cannot record an observer it does not know
(rspl_map_add_point_observation refuses the frame), so that branch is checked on the restatement only."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import lmap_cases as LC
import lmap_ref as LR

ROOT = pathlib.Path(__file__).resolve().parents[1]
FUNCS = ("rspl_lmap_create", "rspl_lmap_destroy", "rspl_lmap_store", "rspl_lmap_store_host", "rspl_lmap_bank_size",
         "rspl_lmap_set_local", "rspl_lmap_enqueue", "rspl_lmap_fetch", "rspl_lmap_debug_points",
         "rspl_lmap_track_enqueue", "rspl_lmap_debug_search_host", "rspl_map_reference_keyframe",
         "rspl_map_local_mappoints")


@pytest.fixture(scope="module")
def pkg():
    import rspl_loader
    return rspl_loader.load()


# 1: the boundary -----------------------------------------------------------------------------------------------
def test_header_declares_lmap_api_and_keeps_abi_2():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    for n in FUNCS:
        assert n in names
    for s in ("rspl_lmap_config", "rspl_lmap_frame", "rspl_lmap_result", "rspl_lmap_host_problem"):
        assert re.search(r"}\s*%s;" % s, hdr), s
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct changed


def test_capi_binds_lmap_api(pkg):
    lib = pkg.capi.load()
    for n in FUNCS:
        assert n in pkg.capi.EXPORTS and hasattr(lib, n)
    assert len(lib.rspl_lmap_track_enqueue.argtypes) == 6
    assert [f[0] for f in pkg.capi.LmapConfig._fields_] == ["max_bank_points", "max_local_points", "max_keypoints",
                                                            "max_batch", "device", "radius", "max_distance", "max_ratio"]
    from rspl_slam_amd import api
    assert [api.LMAP_NOT_SELECTED, api.LMAP_BEHIND, api.LMAP_OFF_IMAGE, api.LMAP_NO_CANDIDATE, api.LMAP_FAILED,
            api.LMAP_GOOD] == [LR.NOT_SELECTED, LR.BEHIND, LR.OFF_IMAGE, LR.NO_CANDIDATE, LR.FAILED, LR.GOOD]


# 2: the restatement against itself -----------------------------------------------------------------------------
def _frame(xy, W=LC.W, H=LC.H, held=()):
    F = np.zeros((len(xy), 259))
    F[:, 1:3] = xy
    pid = np.full(len(xy), -1, np.int32)
    pid[list(held)] = 1
    return dict(features=F, u_right=None, point_id=pid, point_xyz=np.zeros((len(xy), 3)), Twc=np.eye(4), cam=LC.CAM,
                width=W, height=H)


def test_round_is_half_away_from_zero():
    assert [LR.c_round(t) for t in (0.5, 1.5, 2.5, -0.5, 0.49999999999999994, 2.4999999999999996)] == [1, 2, 3, -1, 0, 2]
    # cell width 8, height 8: x * 0.125 exactly at .5; x near W rounds to 64 and is clamped
    assert LR.cell(4.0, 4.0, LC.W, LC.H) == (1, 1) and LR.cell(12.0, 20.0, LC.W, LC.H) == (2, 3)
    assert LR.cell(3.999, 3.999, LC.W, LC.H) == (0, 0)
    assert LR.cell(509.0, 381.0, LC.W, LC.H) == (63, 47) and LR.cell(511.75, 383.75, LC.W, LC.H) == (63, 47)


@pytest.mark.parametrize("seed", range(6))
def test_walk_candidate_set_equals_the_box(seed):
    rng = np.random.default_rng(seed)
    n = 400
    xy = np.stack([rng.uniform(0, LC.W, n), rng.uniform(0, LC.H, n)], 1)
    xy[:80] = np.round(xy[:80] / 8) * 8 + 4.0                    # on cell-rounding boundaries: x / 8 exactly at .5
    xy[80:120, 0] = rng.uniform(LC.W - 4, LC.W, 40)              # round gives 64: clamped to the last column
    xy[120:140, 1] = rng.uniform(LC.H - 4, LC.H, 20)
    xy = np.clip(xy, 0, [LC.W, LC.H])
    fr = _frame(xy, held=rng.choice(n, 40, replace=False))
    grid = LR.build_grid(fr)
    assert sum(len(v) for v in grid.values()) == n and max(k[0] for k in grid) == 63 and max(k[1] for k in grid) == 47
    hits = 0
    for _ in range(300):
        u, v = rng.uniform(0, LC.W), rng.uniform(0, LC.H)
        if _ % 3 == 0:  # projections at the image's edges and on keypoints' box sides
            u, v = rng.choice([0.25, LC.W - 0.25, u]), rng.choice([0.25, LC.H - 0.25, v])
        if _ % 5 == 0:
            j = rng.integers(n)
            u, v = float(np.float32(xy[j, 0])) - 15.0, float(np.float32(xy[j, 1])) + 14.5
        walk = LR.neighbors_walk(fr, grid, u, v, 0.0)
        assert sorted(walk) == LR.neighbors_brute(fr, u, v, 0.0)
        hits += len(walk)
    assert hits > 300


def test_tie_rule_is_the_walks_first_visited_winner():
    fr, lm = LC.ties()
    a, b = LR.search(fr, lm), LR.search(fr, lm, tie_rule=True)
    assert list(a["best_idx"]) == [1, 2]  # cell order beats index order; inside a cell the lower index
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # many exact ties: 30 keypoints share 3 descriptors around one projection
    rng = np.random.default_rng(0)
    for trial in range(20):
        s = LC.Scene(100 + trial)
        d = LC.unit(rng)
        shared = [LC.at_distance(d, x, rng) for x in (0.1, 0.1001, 0.3)]
        for i in range(30):
            s.keypoint(200.0 + rng.integers(-14, 15), 150.0 + rng.integers(-14, 15), shared[rng.integers(3)])
        s.point(1, s.at(200.0, 150.0), d)
        fr, lm = s.build(boundary=True)
        a, b = LR.search(fr, lm), LR.search(fr, lm, tie_rule=True)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_fixed_order_distance_equals_the_dot_product():
    rng = np.random.default_rng(1)
    a, B = LC.unit(rng), LC.unit(rng, 50)
    d = LR.distance(a, B)
    assert np.abs(d - 2 * (1 - B @ a)).max() < 1e-13
    assert LR.distance(a, B[3]) == d[3] and LR.distance(a, a) == pytest.approx(0.0, abs=1e-15)


# 3: rspl_lmap_debug_search_host against the restatement, bit for bit -------------------------------------------
def all_cases():
    out = [(k, f) for k, f in LC.DESIGNED.items()]
    for nk, nl in LC.SIZES:
        for st in (False, True):
            out.append((f"size_{nk}_{nl}_{'stereo' if st else 'mono'}",
                        lambda nk=nk, nl=nl, st=st: LC.random_scene(nk, nl, seed=100 * nk + nl, stereo=st)))
    out.append(("size_130_600", lambda: LC.random_scene(130, 600, seed=13600)))
    for b in range(3):
        out.append((f"batch_{b}", lambda b=b: (LC.batch_scenes()[0][b], LC.batch_scenes()[1])))
    out.append(("chain", lambda: LC.chain_scene()[:2]))
    return out


@pytest.mark.parametrize("name,build", all_cases(), ids=[c[0] for c in all_cases()])
def test_search_host_equals_ref_bitwise(pkg, name, build):
    fr, lm = build()
    want = LR.search(fr, lm)
    got = pkg.lmap_search_host(fr["features"], fr["point_id"], lm["ids"], lm["pos"], lm["desc"], fr["Twc"], fr["cam"],
                               fr["width"], fr["height"], u_right=fr["u_right"])
    LC.same_bits(got, want)
    np.testing.assert_array_equal(want["status"], LR.search(fr, lm, tie_rule=True)["status"])


# 4: local map selection on hand-built graphs ------------------------------------------------------------------
def _build_map(pkg, frames, points, obs, update):
    """the native map and lmap_ref's graph from one description; the graph's connections are read back from the
    native map (Map::UpdateFrameConnection is checked by tests/test_map.py)"""
    m = pkg.mapping.Map(LC.CAM)
    for f, n in frames.items():
        m.InsertKeyframe(f, float(f), np.eye(4), np.zeros((n, 3)))
    for i, (t, p) in points.items():
        m.InsertMappoint(i, p, t)
    g = dict(frames={f: dict(slots=[-1] * n, conn={}) for f, n in frames.items()},
             points={i: dict(type=t, obs={}, p=p) for i, (t, p) in points.items()})
    for i, f, k in obs:
        m.AddPointObservation(i, f, k)
        g["frames"][f]["slots"][k] = i
        g["points"][i]["obs"][f] = k
    for f in update:
        m.UpdateFrameConnection(f)
    for f in frames:
        g["frames"][f]["conn"] = {i: w for w, i in m.GetOrderedConnections(f)}
    return m, g


def _graph(pkg):
    # Frame 1 (the reference keyframe) shares 16 non-bad points with frames 2 and 4 and 20 with frame 3; frame 6
    # shares nothing with anybody.  Points 0..16 are seen by 1, 2 and 3 (two local keyframes: first occurrence),
    # 17..20 by 1 and 3, 21..36 by 1 and 4; point 5 is bad, point 21 untriangulated; frame 2 also holds points
    # 100..103 of its own in its first slots; frame 5 (the current frame) sees points 0..5 and 21..26.
    frames = {1: 60, 2: 30, 3: 30, 4: 30, 5: 30, 6: 4}
    P = {i: (1, [0.1 * i, 1.0, 2.0 + i]) for i in list(range(37)) + [100, 101, 102, 103, 200]}
    P[5] = (2, P[5][1])
    P[21] = (0, P[21][1])
    obs = [(i, 1, i) for i in range(37)] + [(i, 2, 29 - i) for i in range(17)] + [(i, 3, i) for i in range(21)]
    obs += [(i, 4, i - 21) for i in range(21, 37)] + [(100 + k, 2, k) for k in range(4)]
    obs += [(i, 5, k) for k, i in enumerate(list(range(6)) + list(range(21, 27)))] + [(200, 6, 0)]
    return _build_map(pkg, frames, P, obs, update=[1])


def test_local_mappoints_equal_ref(pkg):
    m, g = _graph(pkg)
    assert m.GetOrderedConnections(1) == [(16, 2), (16, 4), (20, 3)]  # the tie 2 / 4 in id order, then the heavier
    want_ids, want_pos = LR.local_mappoints(g, 1)
    ids, pos = m.LocalMappoints(1)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(pos, want_pos)
    # frame 2's slots in keypoint order (its own points, then 16 .. 0 without the bad point 5), frame 4's without
    # the untriangulated 21, of frame 3's only what frame 2 did not show already
    assert list(ids) == [100, 101, 102, 103] + [i for i in range(16, -1, -1) if i != 5] + list(range(22, 37)) + \
        [17, 18, 19, 20]
    # a reference keyframe without connections; an unknown one
    ids, pos = m.LocalMappoints(6)
    assert len(ids) == 0 and pos.shape == (0, 3) and len(LR.local_mappoints(g, 6)[0]) == 0
    with pytest.raises(pkg.capi.RsplError, match="unknown frame 77"):
        m.LocalMappoints(77)
    # cap too small: an error, the count reported, nothing written
    n, buf = C.c_int(), np.full(10, -7, np.int32)
    rc = pkg.capi.load().rspl_map_local_mappoints(m._h, 1, buf.ctypes.data, None, 10, C.byref(n))
    assert rc == -4 and n.value == len(want_ids) == 39 and (buf == -7).all()
    with pytest.raises(pkg.capi.RsplError, match="capacity 10"):
        m.LocalMappoints(1, cap=10)
    assert len(m.LocalMappoints(1, cap=39)[0]) == 39


def test_reference_keyframe_equals_ref(pkg):
    m, g = _graph(pkg)
    cur = np.array(g["frames"][5]["slots"], np.int32)
    # votes (bad point 5 skipped, untriangulated 21 counted, the current frame 5 itself skipped):
    # frame 1: 11, frame 2: 5, frame 3: 5, frame 4: 6
    assert LR.reference_keyframe(g, 5, cur, 3) == (1, True)
    assert m.ReferenceKeyframe(5, cur, 3) == (1, True)
    assert m.ReferenceKeyframe(5, cur, 1) == LR.reference_keyframe(g, 5, cur, 1) == (1, False)
    # a tie in the counts: seen from frame 1, points 0..9 give frames 2 and 3 nine votes each (frame 5: five)
    # -> the lowest id.  (4242: an id the map does not know is skipped)
    few = np.array([i for i in range(10)] + [-1, 4242], np.int32)
    assert m.ReferenceKeyframe(1, few, 4) == LR.reference_keyframe(g, 1, few, 4) == (2, True)
    # an observer the map does not know (restatement only, see the module docstring): frame 1 taken out of it
    g1 = dict(g, frames={f: v for f, v in g["frames"].items() if f != 1})
    assert LR.reference_keyframe(g1, 5, few, 4) == (2, True)
    # nobody counted: the reference keyframe stays
    none = np.array([-1, 5, 4242], np.int32)
    assert m.ReferenceKeyframe(5, none, 3) == LR.reference_keyframe(g, 5, none, 3) == (3, False)
    assert m.ReferenceKeyframe(5, np.zeros(0, np.int32), 3) == (3, False)


# 5: bank and local table of a host-only handle -----------------------------------------------------------------
def test_bank_and_local_table_errors(pkg):
    rng = np.random.default_rng(2)
    lm = pkg.LocalMap(max_bank_points=4, max_local_points=3, max_keypoints=8, device=-1)
    lm.store_host([], np.zeros((0, 256)))                      # n = 0
    lm.set_local([], np.zeros((0, 3)))
    assert lm.bank_size() == 0
    lm.store_host([7, 9, 11], LC.unit(rng, 3))
    lm.store_host([9], LC.unit(rng, 1))                        # overwrite: no new row
    assert lm.bank_size() == 3
    with pytest.raises(pkg.capi.RsplError, match=r"rc=-4.*do not fit"):
        lm.store_host([11, 20, 21], LC.unit(rng, 3))           # a full bank is an error, not an eviction ...
    assert lm.bank_size() == 3                                 # ... and nothing of the call was stored
    lm.store_host([20, 20], LC.unit(rng, 2))                   # one id twice in a call takes one row
    assert lm.bank_size() == 4
    lm.set_local([9, 7], np.ones((2, 3)))
    with pytest.raises(pkg.capi.RsplError, match=r"rc=-1.*map point 21 has no descriptor"):
        lm.set_local([9, 21], np.ones((2, 3)))                 # unknown id, named
    assert lm.n_local == 2                                     # the local map is unchanged
    with pytest.raises(pkg.capi.RsplError, match="outside"):
        lm.set_local([7, 9, 11, 20], np.ones((4, 3)))          # more than max_local_points
    with pytest.raises(pkg.capi.RsplError, match="host-only"):
        lm.enqueue([])
    with pytest.raises(pkg.capi.RsplError, match="host-only"):
        lm.store([1], [0], 8)
    with pytest.raises(ValueError):
        pkg.LocalMap(max_keypoints=0, device=-1)
    h = C.c_void_p()
    cfg = pkg.capi.LmapConfig(4, 3, 8, 0, 0, 15.0, 0.35, 0.6)   # max_batch 0: refused before a device is touched
    assert pkg.capi.load().rspl_lmap_create(C.byref(cfg), C.byref(h)) == -1 and not h.value


def test_merge_ignores_a_claim_on_a_held_keypoint():
    """TrackLocalMap's loop (map_builder.cc:763-768) checks the slot again although the search's filter never
    proposes a keypoint that holds a point, so no search result can carry such a claim: the branch is checked on the
    restatement, with a hand-made list"""
    fr, lm = LC.filters()
    assert fr["point_id"][0] == 77
    assoc, winner = LR.merge(fr, lm, good_kp=[0, 1, 1], good_point=[2, 0, 2])
    assert list(assoc) == [77, 0, 5, -1] and list(winner) == [-1, 2, -1, -1]  # kept; the last of two claims


def test_host_check_program():
    """tests/c/lmap_check.cpp: the handle's bookkeeping and the host search from C++, linked with the library's own
    objects (tests/c/lmap_check.mk; `lmap_check_san` there is the same program under ASan + UBSan)"""
    import subprocess
    subprocess.run(["make", "-C", str(ROOT / "tests" / "c"), "-f", "lmap_check.mk", "lmap_check"], check=True,
                   capture_output=True)
    r = subprocess.run([str(ROOT / "tests" / "c" / "build" / "lmap_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "lmap_check: ok" in r.stdout, r.stdout + r.stderr


def test_track_local_map_gate():
    assert LR.track_local_map_gate(2, 50, 10, 10) == -1    # fewer than 3 good projections
    assert LR.track_local_map_gate(3, 10, 10, 5) == -1     # n_inliers <= min_num_match
    assert LR.track_local_map_gate(3, 20, 10, 20) == -1    # n_inliers <= num_inlier_thr
    assert LR.track_local_map_gate(3, 21, 10, 20) == 21
