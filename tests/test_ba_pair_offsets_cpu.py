"""Segment offsets of the Schur chunks' edge-pair lists as the local BA's host staging counts them
(ba::pair_offsets through rspl_ba_debug_pair_offsets, csrc/ba_stage.cpp).  Host only -- no device.

The fused first pass fills the lists on the device against these offsets, so they must be exactly what the device's
own count gives: per chunk (a pose pair a <= b and a landmark range of rspl_ba_debug_chunk_geometry) the sum over the
range's landmarks of (edges on reduced pose a) x (edges on reduced pose b).  Counted here in numpy straight from the
problem's edge arrays -- no staging, no CSR."""
import ctypes as C

import numpy as np
import pytest

from rspl_slam_amd import capi

import ba_frame_cases as BC

CASES = BC.structure_cases()


def _reduced_poses(p):
    has = np.zeros(p.pose_q.shape[0], bool)
    for k, _ in BC.KINDS:
        has[getattr(p, k)["pose"]] = True
    opt = has & (p.pose_fixed == 0)
    return np.where(opt, np.cumsum(opt) - 1, -1), int(opt.sum())


def _expected(p, max_landmarks, max_poses):
    nq, nL = p.points.shape[0], p.points.shape[0] + p.lines.shape[0]
    pidx, K = _reduced_poses(p)
    cnt = np.zeros((nL, max(K, 1)), np.int64)  # edges of landmark g on reduced pose a
    for t, (k, _) in enumerate(BC.KINDS):
        d = getattr(p, k)
        g = d["lm"].astype(np.int64) + (nq if t >= 2 else 0)
        a = pidx[d["pose"]]
        np.add.at(cnt, (g[a >= 0], a[a >= 0]), 1)
    pl = capi.BaChunkPlan()
    assert capi.load().rspl_ba_debug_chunk_plan(nL, K, max_landmarks, max_poses, C.byref(pl)) == 0
    chunks = np.full((max(pl.chunks, 1), 6), -9, np.int32)
    order = np.full(max(pl.grid, 1), -9, np.int32)
    assert capi.load().rspl_ba_debug_chunk_geometry(nL, K, max_landmarks, max_poses, chunks.ctypes.data,
                                                    order.ctypes.data) == 0
    pairs = [(a, b) for a in range(K) for b in range(a, K)]
    n = np.zeros(pl.chunks, np.int64)
    for c in range(pl.chunks):
        pr, g0, g1 = (int(v) for v in chunks[c, :3])
        a, b = pairs[pr]
        n[c] = int((cnt[g0:g1, a] * cnt[g0:g1, b]).sum())
    return np.concatenate([[0], np.cumsum(n)]), pl, cnt


def _staged(p, max_landmarks, max_poses, cap):
    off = np.full(cap, -7, np.int32)
    nc = C.c_int(-1)
    P = p.to_ctypes()
    rc = capi.load().rspl_ba_debug_pair_offsets(C.byref(P), max_landmarks, max_poses, off.ctypes.data, cap,
                                                C.byref(nc))
    return rc, off, nc.value


def test_exports_declared():
    import pathlib
    hdr = (pathlib.Path(__file__).resolve().parents[1] / "include" / "rspl.h").read_text()
    lib = capi.load()
    for n in ("rspl_ba_debug_pair_offsets", "rspl_ba_debug_pairs", "rspl_ba_debug_final"):
        assert n in hdr and n in capi.EXPORTS and hasattr(lib, n)
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct or call changed


@pytest.mark.parametrize("name,p", CASES, ids=[n for n, _ in CASES])
def test_pair_offsets_match_numpy(name, p):
    want, pl, cnt = _expected(p, BC.MAX_LANDMARKS, BC.CAPS["max_poses"])
    rc, off, nc = _staged(p, BC.MAX_LANDMARKS, BC.CAPS["max_poses"], pl.chunks + 1)
    assert rc == 0, capi.load().rspl_last_error()
    assert nc == pl.chunks
    np.testing.assert_array_equal(off[:nc + 1], want)


def test_cases_have_the_shapes_they_claim():
    """the windows above really hold what the list code branches on"""
    cases = dict(CASES)
    nL = lambda p: p.points.shape[0] + p.lines.shape[0]  # noqa: E731
    deg = lambda p, g: len(BC.landmark_edges(p, g))      # noqa: E731
    for n in (1, 63, 64, 65, 255, 256, 257):
        for K in (1, 2, 10):
            assert nL(cases[f"nL{n}-K{K}"]) == n
    for K in (1, 2, 10):  # (a single landmark is not seen by every pose)
        assert _reduced_poses(cases[f"nL257-K{K}"])[1] == K
    _, pl, _ = _expected(cases["wide-dsub"], BC.MAX_LANDMARKS, BC.CAPS["max_poses"])
    assert pl.dsub > 1 and pl.nchk >= 2
    assert deg(cases["edges9"], 3) == 9
    assert deg(cases["edges17"], 70) == 17 and deg(cases["edges17"], 129) == 9
    assert cases["edges17"].points.shape[0] <= 129  # (landmark 129 is a line)
    _, _, cnt = _expected(cases["twice-on-a-pose"], BC.MAX_LANDMARKS, BC.CAPS["max_poses"])
    assert cnt[1].max() >= 2
    assert deg(cases["inactive"], 0) == 0 and deg(cases["inactive"], 64) == 0
    p = cases["fixed-pose-edges"]
    assert p.pose_fixed.sum() == 2 and all((getattr(p, k)["pose"] == 3).any() for k in ("mono", "stereo"))
    want, pl, _ = _expected(cases["empty-chunk"], BC.MAX_LANDMARKS, BC.CAPS["max_poses"])
    assert (np.diff(want) == 0).any() and (np.diff(want) > 0).any()
    assert cases["lines-only"].points.shape[0] == 0 and BC.n_edges(cases["lines-only"]) > 0


def test_pair_offsets_rejects_bad_arguments():
    p = dict(CASES)["nL65-K2"]
    want, pl, _ = _expected(p, BC.MAX_LANDMARKS, BC.CAPS["max_poses"])
    assert _staged(p, BC.MAX_LANDMARKS, BC.CAPS["max_poses"], pl.chunks)[0] == -1      # one offset short
    assert _staged(p, 10, BC.CAPS["max_poses"], pl.chunks + 1)[0] == -1                # window beyond the handle
    nc = C.c_int()
    assert capi.load().rspl_ba_debug_pair_offsets(None, 10, 10, None, 0, C.byref(nc)) == -1
