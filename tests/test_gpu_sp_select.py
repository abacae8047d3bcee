"""The SuperPoint tail on score maps the test builds: nms_kernel's candidate extraction (threshold in double,
borders, ballot-and-scan slot reservation), every branch of topk_kernel, and the fp32 sample_kernel, launched by
rspl_sp_debug_select through the function rspl_sp_infer_device itself calls (select_and_sample in sp.cpp).

Reference: oracle.simple_nms, then post.sp_postprocess.  The cases, and the proof that each lands in the regime it
names, are in sp_select_cases.py / test_sp_select_cpu.py.

Asserted per image:
  * cand_counts = the reference's n, counts = min(n, k) (0 for k = 0 and for keep-all beyond 16384 candidates);
  * features[:, 0:3] (score, x, y) EQUAL to the reference's, in the reference's order -- these inputs are ours, so
    none of compare_features' near-tie allowances apply;
  * descriptors within DESC_TOL of the reference's: both sides compute in fp64 from the same fp32 map and differ in
    summation order only.  The tolerance is 8 x the reference's own norm-order difference, measured on the CPU over
    all cases as 1.943e-16 (test_sp_select_cpu.test_descriptor_tolerance_is_the_references_own_error), that is
    1.56e-15; a dropped or swapped tap moves a component by about 1e-2.  Where the reference's descriptor is 0/0 (a
    keypoint at x = W-1 or y = H-1, border 0: all four weights are zero) the device's must be NaN as well;
  * every feature row at or beyond an image's count keeps the test's fill pattern.
One SP_SELECT_PARITY JSON line is printed per case (collected in profiles/sp_select_parity.json)."""
import json

import numpy as np
import pytest

import sp_select_cases as SC

pytestmark = pytest.mark.gpu
CASES = SC.cases()


@pytest.fixture(scope="module")
def pkg():
    import rspl_loader
    return rspl_loader.load()


def _handle(pkg, w, c, k=None, precision=None):
    B, H, W = c.shape
    cfg = pkg.SuperPointConfig(max_keypoints=c.k if k is None else k, keypoint_threshold=c.threshold,
                               remove_borders=c.border, weights=w, max_height=H, max_width=W, max_batch=B)
    if precision is not None:
        cfg.precision = precision
    sp = pkg.SuperPoint(cfg)
    assert sp.build(), sp.error
    return sp


def _compare(c, F, cnt, cand, images=None):
    """figures first (one JSON line), then the assertions"""
    B = c.shape[0]
    allc, ref = SC.keep_all_reference(c), SC.reference(c)
    images = range(B) if images is None else images
    rows = []
    for j, b in enumerate(images):
        n, G = allc[b].shape[1], ref[b]
        got = F[j, :max(0, int(cnt[j]))].T
        same_shape = got.shape == G.shape
        head_equal = same_shape and np.array_equal(got[:3], G[:3])
        nan_equal = same_shape and np.array_equal(np.isnan(got[3:]), np.isnan(G[3:]))
        diff = float(np.nanmax(np.abs(got[3:] - G[3:]))) if same_shape and G.size and not np.all(np.isnan(G[3:])) else 0.0
        untouched = bool(np.all(F[j, max(0, int(cnt[j])):] == SC.FILL))
        rows.append(dict(image=int(b), n_ref=int(n), cand=int(cand[j]), count=int(cnt[j]),
                         count_ref=int(SC.expected_count(n, c.k)), regime=c.regime[b], head_equal=bool(head_equal),
                         nan_equal=bool(nan_equal), desc_max_abs_diff=diff, untouched_beyond_count=untouched))
    print("SP_SELECT_PARITY " + json.dumps(dict(case=c.name, k=c.k, border=c.border, shape=list(c.shape),
                                                tol=SC.DESC_TOL, images=rows)))
    for j, b in enumerate(images):
        n, G = allc[b].shape[1], ref[b]
        assert cand[j] == n, (c.name, b)
        assert cnt[j] == SC.expected_count(n, c.k) == G.shape[1], (c.name, b)
        got = F[j, :cnt[j]].T
        np.testing.assert_array_equal(got[:3], G[:3], err_msg=f"{c.name} image {b}: score, x, y and order")
        np.testing.assert_array_equal(np.isnan(got[3:]), np.isnan(G[3:]), err_msg=f"{c.name} image {b}: 0/0 descriptors")
        np.testing.assert_allclose(got[3:], G[3:], rtol=0, atol=SC.DESC_TOL, err_msg=f"{c.name} image {b}: descriptors")
        assert np.all(F[j, cnt[j]:] == SC.FILL), f"{c.name} image {b}: a row beyond the count was written"


@pytest.mark.parametrize("name", sorted(CASES))
def test_select_and_sample_equal_the_reference(pkg, weight_blobs, name):
    c = CASES[name]
    sp = _handle(pkg, weight_blobs[0], c)
    F, cnt, cand = sp.debug_select(c.scores, c.desc, fill=SC.FILL)
    assert F.shape == (c.shape[0], 16384 if c.k == -1 else max(c.k, 1), 259)
    _compare(c, F, cnt, cand)


def test_mixed_batch_equals_single_image_runs(pkg, weight_blobs):
    """B = 3 in one call (no candidate | select | n < k): each image bit for bit what its own single-image call
    gives on the same handle, counts (0, 43, 3)"""
    c = CASES["g_mixed_batch"]
    sp = _handle(pkg, weight_blobs[0], c)
    F, cnt, cand = sp.debug_select(c.scores, c.desc, fill=SC.FILL)
    assert cnt.tolist() == [0, 43, 3] and cand.tolist() == [0, 88, 3]
    for b in range(3):
        F1, cnt1, cand1 = sp.debug_select(c.scores[b:b + 1], c.desc[b:b + 1], fill=SC.FILL)
        assert cnt1[0] == cnt[b] and cand1[0] == cand[b]
        assert F1[0].tobytes() == F[b].tobytes(), f"image {b}: the batched call differs from the single-image call"
        _compare(c, F1, cnt1, cand1, images=[b])


def test_zero_keypoints_is_zero_keypoints(pkg, weight_blobs):
    """max_keypoints = 0 yields no keypoints (the reference's k < n sort-and-resize): 88 candidates, count 0, no
    feature slot written -- it is not keep-all"""
    c = CASES["a_k0"]
    sp = _handle(pkg, weight_blobs[0], c)
    F, cnt, cand = sp.debug_select(c.scores, c.desc, fill=SC.FILL)
    assert cnt.tolist() == [0] and cand.tolist() == [88]
    assert F.shape == (1, 1, 259) and np.all(F == SC.FILL)


@pytest.mark.parametrize("k", [-2, SC.LDS_CAP + 1])
def test_create_refuses_max_keypoints_outside_the_contract(pkg, weight_blobs, k):
    """below -1 and above kCandCap (a drift of LDS_CAP against the library would show here)"""
    sp = pkg.SuperPoint(pkg.SuperPointConfig(max_keypoints=k, weights=weight_blobs[0], max_height=40, max_width=56,
                                             max_batch=1))
    assert not sp.build() and "max_keypoints" in sp.error
    ok = pkg.SuperPoint(pkg.SuperPointConfig(max_keypoints=SC.LDS_CAP, weights=weight_blobs[0], max_height=40,
                                             max_width=56, max_batch=1))
    assert ok.build(), ok.error


def test_hook_refuses_what_it_cannot_run(pkg, weight_blobs):
    c = CASES["a_k43"]
    sp = _handle(pkg, weight_blobs[0], c, precision=pkg.capi.RSPL_PREC_FP16)
    with pytest.raises(pkg.capi.RsplError, match="RSPL_PREC_FP32"):
        sp.debug_select(c.scores, c.desc)
    sp = _handle(pkg, weight_blobs[0], c)
    with pytest.raises(pkg.capi.RsplError, match="multiples of 8"):      # beyond the arena
        sp.debug_select(np.zeros((1, 48, 56), np.float32), np.zeros((1, 256, 6, 7), np.float32))
    with pytest.raises(pkg.capi.RsplError, match="batch"):
        sp.debug_select(np.zeros((2, 40, 56), np.float32), np.zeros((2, 256, 5, 7), np.float32))
    sp.debug_select(c.scores, c.desc)
    with pytest.raises(pkg.capi.RsplError):      # the hook overwrote the last inference's maps: last_B = 0
        sp.debug_maps(0, 40, 56)
