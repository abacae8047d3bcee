"""The cases of tests/sp_select_cases.py, proved on the reference alone (oracle.simple_nms + post.sp_postprocess):
every image has the candidate count it is meant to have, that count stands in the meant relation to k and 16384
(topk_kernel's branch), the cut falls inside a tie group where the case says so, and the threshold, border, seam
and edge pixels are kept or dropped as listed.  This is what keeps test_gpu_sp_select.py from comparing the wrong
regime; it needs no GPU.  Also: the boundary is declared and bound, rspl_sp_create refuses max_keypoints outside
[-1, 16384] before a device is touched, and the descriptor tolerance is the reference's own error."""
import pathlib
import re

import numpy as np
import pytest

import post
import sp_select_cases as SC

ROOT = pathlib.Path(__file__).resolve().parents[1]
CASES = SC.cases()


def _pkg():
    import rspl_loader
    return rspl_loader.load()


def test_hook_is_declared_and_bound():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    assert "rspl_sp_debug_select" in set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    capi = _pkg().capi
    lib = capi.load()
    assert "rspl_sp_debug_select" in capi.EXPORTS and hasattr(lib, "rspl_sp_debug_select")
    assert len(lib.rspl_sp_debug_select.argtypes) == 10
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct changed


def test_lds_cap_is_the_library_constant():
    src = (ROOT / "rspl-slam_amd" / "csrc" / "sp.cpp").read_text()
    assert re.search(r"kCandCap\s*=\s*%d\b" % SC.LDS_CAP, src)


@pytest.mark.parametrize("k", [-2, -100, SC.LDS_CAP + 1])
def test_create_refuses_max_keypoints_outside_the_contract(weight_blobs, k):
    """-1 keeps all, 0 yields none, [1, 16384] is the top-k; anything else is RSPL_E_ARG before a device is touched
    (no launch: this machine may have no device at all)"""
    pkg = _pkg()
    sp = pkg.SuperPoint(pkg.SuperPointConfig(max_keypoints=k, weights=weight_blobs[0], max_height=40, max_width=56,
                                             max_batch=1))
    assert not sp.build()
    assert "max_keypoints" in sp.error


def test_regime_function_at_its_boundaries():
    C = SC.LDS_CAP
    assert SC.regime(88, -1) == "keep_all" and SC.regime(C, -1) == "keep_all" and SC.regime(C + 1, -1) == "overflow"
    assert SC.regime(88, 100) == "scan" and SC.regime(88, 88) == "scan" and SC.regime(0, 43) == "scan"
    assert SC.regime(88, 87) == "whole_sort" and SC.regime(88, 44) == "whole_sort" and SC.regime(88, 43) == "select"
    assert SC.regime(89, 44) == "select" and SC.regime(C, C // 2) == "whole_sort" and SC.regime(C, C // 2 - 1) == "select"
    assert SC.regime(C + 1, C) == "select" and SC.regime(C + 1, C + 1) == "overflow"
    assert SC.regime(88, 0) == "none" and SC.regime(0, 0) == "none"
    assert SC.expected_count(88, 43) == 43 and SC.expected_count(88, -1) == 88 and SC.expected_count(88, 0) == 0
    assert SC.expected_count(3, 43) == 3 and SC.expected_count(C + 1, -1) == 0


def test_every_regime_and_boundary_is_covered():
    seen = {r for c in CASES.values() for r in c.regime}
    assert seen == {"none", "keep_all", "overflow", "scan", "whole_sort", "select"}
    nk = {(n, c.k) for c in CASES.values() for n in c.n}
    # n = k, k+1, 2k, 2k+2 on the lattice; 16384 exactly full, at 2k and just beyond; beyond the LDS sort
    for want in ((88, 88), (88, 87), (88, 44), (88, 43), (SC.LDS_CAP, -1), (SC.LDS_CAP, 8192), (SC.LDS_CAP, 8191)):
        assert want in nk, want
    assert any(n > SC.LDS_CAP and c.k == SC.LDS_CAP for c in CASES.values() for n in c.n)
    assert max(c.shape[1] * c.shape[2] for c in CASES.values()) == 136 * 144


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_lands_in_its_regime(name):
    c = CASES[name]
    B, H, W = c.shape
    assert H % 8 == 0 and W % 8 == 0 and c.desc.shape == (B, 256, H // 8, W // 8)
    np.testing.assert_allclose(np.sqrt((c.desc.astype(np.float64) ** 2).sum(axis=1)), 1.0, atol=1e-6)
    allc = SC.keep_all_reference(c)
    ref = SC.reference(c)
    for b in range(B):
        A = allc[b]
        n = A.shape[1]
        assert n == c.n[b], (name, b, n)
        assert SC.regime(n, c.k) == c.regime[b], (name, b, n, c.k)
        assert ref[b].shape == (259, SC.expected_count(n, c.k))
        # keep-all order is the row-major scan, and no pixel appears twice
        flat = (A[2] * W + A[1]).astype(np.int64)
        assert np.all(np.diff(flat) > 0)
        # every candidate is above the threshold in double and inside the border
        assert np.all(A[0] > c.threshold)
        assert np.all((A[1] >= c.border) & (A[1] < W - c.border) & (A[2] >= c.border) & (A[2] < H - c.border))
        # at x = W-1 or y = H-1 (reachable with border 0 only: the seam case's last column and row) the reference's
        # four weights are all zero and its descriptor is 0/0; everywhere else every value is finite
        edge = (A[1] == W - 1) | (A[2] == H - 1)
        assert np.all(np.isfinite(A[:, ~edge])) and np.all(np.isnan(A[3:, edge])) and np.all(np.isfinite(A[:3]))
        assert edge.any() == name.startswith("e_seams")
        have = set(zip(A[2].astype(int).tolist(), A[1].astype(int).tolist()))
        for bb, y, x in c.kept:
            assert bb != b or (y, x) in have, (name, "kept", bb, y, x)
        for bb, y, x in c.dropped:
            assert bb != b or (y, x) not in have, (name, "dropped", bb, y, x)
        if c.regime[b] in ("whole_sort", "select"):
            G = ref[b]
            order = np.lexsort((flat, -A[0]))       # score descending, then flat index ascending
            np.testing.assert_array_equal(G[:3], A[:3, order[:c.k]])
            tie = A[0, order[c.k - 1]] == A[0, order[c.k]]
            assert bool(tie) == c.tie_cut, (name, b)
    assert all(bb < B for bb, _, _ in c.kept + c.dropped)


def test_low_byte_case_differs_in_the_last_score_byte_only():
    A = SC.keep_all_reference(CASES["b2_low_byte_k43"])[0]
    bits = A[0].astype(np.float32).view(np.uint32)
    assert np.unique(bits).size == 88 and np.unique(bits >> 8).size == 1


def test_three_value_case_has_three_groups_around_both_cuts():
    A = SC.keep_all_reference(CASES["b1_three_values_k43"])[0]
    v, cnt = np.unique(A[0], return_counts=True)
    assert v.size == 3 and cnt[::-1].tolist() == [30, 25, 33]   # cumulative 30, 55, 88: cuts 43 and 60 inside groups
    assert np.unique(SC.keep_all_reference(CASES["b3_all_equal_k43"])[0][0]).size == 1


def test_threshold_neighbours():
    assert float(SC.T0) > SC.THRESHOLD and not float(SC.T_DN) > SC.THRESHOLD and float(SC.T_UP) > SC.THRESHOLD
    assert SC.T_DN < SC.T0 < SC.T_UP and SC.T0 == np.float32(0.004)
    assert not SC.T_DN > np.float32(SC.THRESHOLD) and not SC.T0 > np.float32(SC.THRESHOLD)  # a float compare drops T0
    c = CASES["c_threshold_edge"]
    A = SC.keep_all_reference(c)[0]
    assert (A[0] == float(SC.T0)).sum() == 3 and (A[0] == float(SC.T_UP)).sum() == 3 and (A[0] == float(SC.T_DN)).sum() == 0
    assert (SC.nms_maps(c)[0] == SC.T_DN).sum() == 3      # the NMS keeps them; only the threshold drops them


def test_seam_case_geometry():
    c = CASES["e_seams_k400"]
    assert c.shape == (2, 72, 136)      # 3 x 3 tiles of 64 x 32 per image, the last 8 wide and 8 high
    xs = {x for b in range(2) for _, x in SC.E_SPECIAL[b]}
    ys = {y for b in range(2) for y, _ in SC.E_SPECIAL[b]}
    assert set(SC.SEAM_X) <= xs and set(SC.SEAM_Y) <= ys
    A0 = SC.keep_all_reference(c)[0]
    y0, y1, x0, x1 = SC.PLATEAU
    inside = (A0[2] >= y0) & (A0[2] < y1) & (A0[1] >= x0) & (A0[1] < x1)
    assert inside.sum() == 144 and np.all(A0[0, inside] == float(np.float32(0.3)))
    assert not np.array_equal(c.scores[0], c.scores[1])


def test_edge_tap_case_extrapolates():
    """keypoints at x = 0 / y = 0 (and x = 2 / y = 2) lie left of / above the first cell centre: the nw tap is
    clamped and the weights leave [0, 1]"""
    c = CASES["h_edge_taps"]
    A = SC.keep_all_reference(c)[0]
    assert {(0, 0), (0, 12), (12, 0)} <= set(zip(A[1].astype(int).tolist(), A[2].astype(int).tolist()))
    h, w = c.shape[1] // 8, c.shape[2] // 8
    for x in (0.0, 2.0):
        ix = ((x - 4 + 0.5) / (w * 8 - 4 - 0.5) * 2 - 1 + 1) / 2 * (w - 1)
        assert ix < 0


def _sample_pairwise(xs, ys, desc):
    """post.sample_descriptors with the norm summed by np.sum (pairwise) instead of sequentially"""
    out = post.sample_descriptors(xs, ys, desc)
    raw = _raw_blend(xs, ys, desc)
    ss = np.sum(raw * raw, axis=1)
    return out, (1.0 / np.sqrt(ss))[:, None] * raw


def _raw_blend(xs, ys, desc, s=8):
    """the blend of post.sample_descriptors before normalize_descriptors, in the same operation order"""
    dim, h, w = desc.shape
    x, y = xs.astype(np.float64), ys.astype(np.float64)
    gx = (x - s // 2 + 0.5) / (w * s - s // 2 - 0.5) * 2 - 1
    gy = (y - s // 2 + 0.5) / (h * s - s // 2 - 0.5) * 2 - 1
    ix, iy = ((gx + 1) / 2) * (w - 1), ((gy + 1) / 2) * (h - 1)
    clip = lambda v, m: np.minimum(np.maximum(v, 0), m - 1)
    ix_nw, iy_nw = clip(np.floor(ix).astype(np.int64), w), clip(np.floor(iy).astype(np.int64), h)
    ix_ne, iy_ne = clip(ix_nw + 1, w), clip(iy_nw, h)
    ix_sw, iy_sw = clip(ix_nw, w), clip(iy_nw + 1, h)
    ix_se, iy_se = clip(ix_nw + 1, w), clip(iy_nw + 1, h)
    nw, ne = (ix_se - ix) * (iy_se - iy), (ix - ix_sw) * (iy_sw - iy)
    sw, se = (ix_ne - ix) * (iy - iy_ne), (ix - ix_nw) * (iy - iy_nw)
    d = desc.astype(np.float64)
    out = (d[:, iy_nw, ix_nw] * nw + d[:, iy_ne, ix_ne] * ne) + d[:, iy_sw, ix_sw] * sw
    return (out + d[:, iy_se, ix_se] * se).T.copy()


def test_descriptor_tolerance_is_the_references_own_error():
    """Both sides blend and normalise in fp64 from the same fp32 map and differ only in summation order.  The
    tolerance of the GPU test is 8 x the largest difference between post.sample_descriptors as written
    (sequential norm) and the same with a pairwise norm, over every candidate of every case, floored at 4 double
    ulps at 1.0.  Measured here: 1.943e-16, so the tolerance is 1.56e-15 (the floor is 8.9e-16)."""
    worst = 0.0
    done = set()
    for c in CASES.values():
        if (c.map_id, c.border) in done:
            continue
        done.add((c.map_id, c.border))
        for b, A in enumerate(SC.keep_all_reference(c)):
            if not A.shape[1]:
                continue
            xs, ys = A[1].astype(np.int64), A[2].astype(np.int64)
            with np.errstate(divide="ignore", invalid="ignore"):    # 0/0 at x = W-1 or y = H-1 (the seam case)
                seq, pair = _sample_pairwise(xs, ys, c.desc[b])
            np.testing.assert_array_equal(seq, A[3:].T)     # the restated blend is the reference's, bit for bit
            raw = _raw_blend(xs, ys, c.desc[b])
            ss = np.cumsum(raw * raw, axis=1)[:, -1]
            with np.errstate(divide="ignore", invalid="ignore"):
                np.testing.assert_array_equal((1.0 / np.sqrt(ss))[:, None] * raw, seq)
            worst = max(worst, float(np.nanmax(np.abs(seq - pair))))
    print(f"SP_SELECT norm-order difference {worst:.3e}, tolerance {SC.DESC_TOL:.3e}")
    assert 0.0 < worst <= SC.NORM_ORDER_DIFF
    assert SC.DESC_TOL == max(8 * SC.NORM_ORDER_DIFF, 4 * np.finfo(np.float64).eps)
