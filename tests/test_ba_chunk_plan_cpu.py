"""Schur chunk geometry of the local BA (ba::chunk_plan, chunk_geo and the launch order chunk_at, through
rspl_ba_debug_chunk_plan / rspl_ba_debug_chunk_geometry).  Host only -- no device.

For every window: each pose pair's chunks tile [0, nL) once in increasing landmark order, a pair's chunks are
contiguous, the chunks fit the handle's buffers, and the launch order visits every chunk once.  Windows of 8 or more
landmark ranges: every chunk of range lb on XCD lb % 8 (where update_errors' workgroups of that range look for its
records), the diagonal pose pairs' chunks on each XCD's lowest workgroup ids, idle slots last; plain chunk order
below 8 ranges.  The plan itself (ranges, diagonal sub-chunks of wide windows) is the formula run_call had inline
before chunk_plan: restated here, for every window."""
import ctypes as C

import numpy as np
import pytest

from rspl_slam_amd import capi

KS = (1, 2, 9, 10, 11, 29)
C3_NL, C3_K = 3938, 9
K_WAVE = 10          # wave_path(K): the single-wave solve's windows
LM_CHUNK = 256       # kLmChunk
CHUNK_WAVES = 1024   # kChunkWaves


def _plan(nL, K, maxL=None, maxK=None):
    pl = capi.BaChunkPlan()
    rc = capi.load().rspl_ba_debug_chunk_plan(nL, K, nL if maxL is None else maxL, K if maxK is None else maxK,
                                              C.byref(pl))
    assert rc == 0
    return pl


def _geometry(nL, K, maxL=None, maxK=None):
    pl = _plan(nL, K, maxL, maxK)
    chunks = np.full((max(pl.chunks, 1), 6), -9, np.int32)
    order = np.full(max(pl.grid, 1), -9, np.int32)
    rc = capi.load().rspl_ba_debug_chunk_geometry(nL, K, nL if maxL is None else maxL, K if maxK is None else maxK,
                                                  chunks.ctypes.data, order.ctypes.data)
    assert rc == 0
    return pl, chunks[:pl.chunks], order[:pl.grid]


def _before(nL, K, slots):
    """the geometry before the balanced plan: ranges of 256 landmarks while the chunk waves fit one dispatch round,
    fewer and wider ones beyond; 8 diagonal sub-chunks on wide windows of fewer than 8 ranges"""
    npairs = K * (K + 1) // 2
    nchk = max(1, min((nL + LM_CHUNK - 1) // LM_CHUNK, CHUNK_WAVES // max(npairs, 1)))
    lmchunk = max(LM_CHUNK, ((nL + nchk - 1) // nchk + 63) // 64 * 64)
    nchk = max((nL + lmchunk - 1) // lmchunk, 1)
    dsub, lmsub = 1, lmchunk
    if not (0 < K <= K_WAVE) and nchk < 8 and nchk * (npairs + 7 * K) <= slots:
        dsub, lmsub = 8, ((lmchunk + 7) // 8 + 63) // 64 * 64
    return nchk, lmchunk, dsub, lmsub


def _sizes():
    lc = _plan(C3_NL, C3_K).lmchunk
    ns = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 2049, 7 * lc, 7 * lc + 1, 8 * lc - 1, 8 * lc, 8 * lc + 1,
          3000, C3_NL, C3_NL + 1, 4096, 4100}
    return sorted(ns)


def test_exports_declared():
    hdr = (capi.PKG.parent / "include" / "rspl.h").read_text()
    lib = capi.load()
    for n in ("rspl_ba_debug_chunk_plan", "rspl_ba_debug_chunk_geometry"):
        assert n in hdr and n in capi.EXPORTS and hasattr(lib, n)
    pl = capi.BaChunkPlan()
    assert lib.rspl_ba_debug_chunk_plan(10, 2, 5, 2, C.byref(pl)) == -1   # window beyond the handle
    assert lib.rspl_ba_debug_chunk_plan(10, 2, 10, 2, None) == -1
    assert lib.rspl_ba_debug_chunk_plan(-1, 2, 10, 2, C.byref(pl)) == -1


def test_c3_plan():
    pl = _plan(C3_NL, C3_K, 6200, 16)  # the benchmark's handle
    assert (pl.nchk, pl.lmchunk, pl.dsub, pl.lmsub) == (16, 256, 1, 256)
    assert pl.chunks == pl.grid == 45 * 16  # no idle slot
    assert pl.ue_bpr == 8  # the update workgroups follow the chunks' XCDs


@pytest.mark.parametrize("K", KS)
def test_chunk_geometry(K):
    npairs = K * (K + 1) // 2
    pairs = [(a, b) for a in range(K) for b in range(a, K)]
    for nL in _sizes():
        for maxL, maxK in ((nL, K), (nL + 300, max(K, 12))):
            pl, ch, order = _geometry(nL, K, maxL, maxK)
            tag = f"K={K} nL={nL} handle=({maxL},{maxK}) plan=({pl.nchk},{pl.lmchunk},{pl.dsub},{pl.lmsub})"
            # ---- the plan ----
            assert (pl.nchk, pl.lmchunk, pl.dsub, pl.lmsub) == _before(nL, K, pl.slots), tag
            assert pl.slots == maxK * (maxK + 1) // 2 * max((maxL + LM_CHUNK - 1) // LM_CHUNK, 1), tag
            assert pl.dsub == 1 or (K > K_WAVE and pl.nchk < 8), tag
            assert pl.nchk * pl.lmchunk >= nL and (pl.nchk - 1) * pl.lmchunk < nL, tag
            assert pl.dsub * pl.lmsub >= pl.lmchunk, tag
            assert pl.chunks == pl.nchk * (npairs + (pl.dsub - 1) * K), tag
            assert pl.chunks <= pl.slots, tag
            # ---- every pose pair's chunks: contiguous, tiling [0, nL) once in landmark order ----
            c = 0
            for pr, (a, b) in enumerate(pairs):
                n = pl.nchk * (pl.dsub if a == b else 1)
                rows = ch[c:c + n]
                assert (rows[:, 0] == pr).all() and (rows[:, 3] == c).all() and (rows[:, 4] == c + n).all(), tag
                g0, g1, gend = rows[:, 1], rows[:, 2], rows[:, 5]
                live = g1 > g0
                assert g0[0] == 0 and live[0], tag
                assert (g1[live][:-1] == g0[live][1:]).all() and g1[live][-1] == nL, tag  # no gap, no overlap
                assert (g1[~live] == g0[~live]).all() and ((g0 >= nL) | (g0 >= gend))[~live].all(), tag  # (empty: past the end)
                assert (g1 == np.minimum(gend, nL))[live].all(), tag
                c += n
            assert c == pl.chunks, tag
            # ---- the launch order ----
            assert (order >= -1).all(), tag  # (-2: the order's geometry of a chunk differs from chunk_geo's)
            seen = order[order >= 0]
            assert np.array_equal(np.sort(seen), np.arange(pl.chunks)), tag
            if pl.nchk < 8:
                assert pl.grid == pl.chunks and np.array_equal(order, np.arange(pl.chunks)), tag
                continue
            vb = np.flatnonzero(order >= 0)
            lb = ch[order[vb], 1] // pl.lmchunk
            assert (vb % 8 == lb % 8).all(), tag
            assert pl.grid == 8 * ((pl.nchk + 7) // 8) * npairs, tag
            assert pl.ue_bpr * 32 == pl.lmchunk, tag  # (32 landmarks per update workgroup)
            diag = np.array([a == b for a, b in pairs])[ch[order[vb], 0]]
            for x in range(8):  # per XCD: the diagonal pairs' chunks before every off-diagonal one
                d = diag[vb % 8 == x]
                first_off = len(d) if d.all() else int(np.argmin(d))
                assert not d[first_off:].any(), tag
                idle = order[x::8] < 0  # its idle slots: after all of its chunks
                assert not idle[:len(d)].any(), tag


@pytest.mark.parametrize("K", (2, 9, 29))
def test_points_only_flag_with_lines_inside_a_chunk(K):
    """points + lines with the border inside a chunk (K = 29: inside a diagonal sub-chunk): a chunk takes the 3-dim
    loops only when its nominal end is within the points"""
    pl = _plan(3000, K)
    assert pl.dsub == (8 if K == 29 else 1)
    nq = 2 * pl.lmchunk + pl.lmsub + 7  # inside the (sub-)chunk that starts at 2 lmchunk + lmsub
    nL = nq + 60
    pl, ch, _ = _geometry(nL, K)
    pts = ch[:, 5] <= nq
    assert (ch[pts, 2] <= nq).all()
    holds = (ch[:, 1] <= nq) & (nq < ch[:, 2])
    assert holds.sum() == K * (K + 1) // 2 and not pts[holds].any()
    assert pts.any() and (~pts).any()
