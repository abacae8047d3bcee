"""GPU: the RSPL_PREC_FP16 front end (the benchmark's configuration) kernel by kernel.

1. Bitwise invariance (no hooks): the batched device paths of SuperPoint (B = 2) and SuperGlue (B = 2, 3, 5: the XCD
   placements xps = 2, 1 and the 2-D grid; nmax 96 and 72; normalize off / on; post stream) give the bytes of the
   max_batch = 1 host path, also right after a call with a larger image / larger counts on the same handle.
2. One stage at a time (rspl_sp_debug_layer, rspl_sg_debug_layers) against the fp64-accumulated restatement of the
   same operation on the same fp16 operands (oracle/fp16_emu.py) at the smallest shapes that reach every tile edge,
   batch boundary and grid-placement branch.  Tolerances and their derivation: tests/fp16_cases.py (GAMMA0 = 2 for the
   3x3 convolutions, 4 for conv1a and the 1x1 heads, GAMMA = 4 GAMMA0; SuperGlue 4 x the restatement's own spread).

Worst |gpu - ref| / bound measured on an MI355X (each test prints its own):
    conv1 0.47 / 0.80 / 0.89 (8 x 8, 24 x 40, 136 x 264: the allowance for conv1a's intermediate rounding dominates;
    flip share 0.10-0.16 %)      conv2a .. convPD 0.48-0.50 at every shape (i.e. the fp16 rounding itself; flip
    share 0-0.06 %)              det_head 0.02 (P = 1), 0.07 (P = 561)          taps 0.013
    SuperGlue layers: X 0.22-0.27, next q 0.25-0.33 of 4 x spread (spreads X 7e-5 .. 1.4e-4 S, q 5e-5 .. 8e-5 S)
The bitwise checks of part 1 hold as they stand.
"""
import numpy as np
import pytest

import fp16_cases as C
import fp16_emu as E
import post

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import rspl_loader
    return rspl_loader.load()


@pytest.fixture(scope="module")
def sp_w(pkg, weight_blobs):
    return pkg.weights.read_blob(weight_blobs[0])


@pytest.fixture(scope="module")
def sg_w(pkg, weight_blobs):
    return pkg.weights.read_blob(weight_blobs[1])


def _bytes_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


# --------------------------------------------------------------------------------------------------------------
# 1. bitwise invariance
# --------------------------------------------------------------------------------------------------------------
SP_K = 128


def _sp16(pkg, w, H, W, B, k=SP_K):
    sp = pkg.SuperPoint(pkg.SuperPointConfig(max_keypoints=k, weights=w, max_height=H, max_width=W, max_batch=B,
                                             precision=pkg.capi.RSPL_PREC_FP16))
    assert sp.build(), sp.error
    return sp


def test_sp_fp16_batched_equals_single_bitwise(pkg, weight_blobs):
    """infer_device with B = 2 on two different images equals infer of each image on a max_batch = 1 handle of the
    same limits, byte for byte, at 136 x 264 (the handle's maximum) and then at 64 x 96 on the same handle: nothing
    of the larger call's activations may leak through the smaller call's halos."""
    from rspl_slam_amd import capi
    from rspl_slam_amd import synthetic as SY
    HM, WM = 136, 264
    sp2 = _sp16(pkg, weight_blobs[0], HM, WM, 2)
    st = capi.Stream()
    feats, counts = capi.DeviceBuffer(2 * SP_K * 259 * 8), capi.DeviceBuffer(8)
    for H, W in ((HM, WM), (64, 96)):
        imgs = [SY.textured_image(H, W, seed=70 + H + i, n_blobs=12 + 5 * i) for i in range(2)]
        dimg = capi.DeviceBuffer(2 * H * W).upload(np.stack(imgs))
        feats.upload(np.full((2, SP_K, 259), -7.0))
        sp2.infer_device(dimg.ptr, 2, H, W, W, H * W, feats.ptr, SP_K, counts.ptr, st.handle)
        st.synchronize()
        F, cnt = feats.download((2, SP_K, 259), np.float64), counts.download((2,), np.int32)
        for b, img in enumerate(imgs):
            sp1 = _sp16(pkg, weight_blobs[0], HM, WM, 1)  # fresh: its arena has seen no other image
            ok, G = sp1.infer(img)
            assert ok, sp1.error
            assert G.shape[1] > 8, "the image must yield keypoints"
            assert cnt[b] == G.shape[1], (H, W, b, cnt[b], G.shape[1])
            _bytes_equal(F[b, :cnt[b]], np.ascontiguousarray(G.T), f"{H}x{W} image {b}")


def _sg16(pkg, w, nmax, B):
    sg = pkg.SuperGlue(pkg.SuperGlueConfig(weights=w, max_keypoints=nmax, max_batch=B,
                                           precision=pkg.capi.RSPL_PREC_FP16))
    assert sg.build(), sg.error
    return sg


def _sg_features(n0, n1, seed):
    from rspl_slam_amd import synthetic as SY
    if n0 == 0 or n1 == 0:
        F, _, _ = SY.sg_problem(max(n0, n1, 1), max(n0, n1, 1), 0, seed)
        return (np.zeros((259, 0)), F[:, :n1]) if n0 == 0 else (F[:, :n0], np.zeros((259, 0)))
    F0, F1, _ = SY.sg_problem(n0, n1, min(n0, n1) // 2, seed)
    return F0, F1


def _sg_device(sg, pairs, nmax, normalize, post_stream=False):
    """one batched device call; returns idx0, idx1 [B, nmax] and ms0, ms1"""
    from rspl_slam_amd import capi
    B = len(pairs)
    f0, f1 = np.zeros((B, nmax, 259)), np.zeros((B, nmax, 259))
    n0, n1 = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for p, (F0, F1) in enumerate(pairs):
        f0[p, :F0.shape[1]], f1[p, :F1.shape[1]] = F0.T, F1.T
        n0[p], n1[p] = F0.shape[1], F1.shape[1]
    st, pst = capi.Stream(), capi.Stream()
    bufs = {k: capi.DeviceBuffer(v.nbytes).upload(v) for k, v in dict(f0=f0, f1=f1, n0=n0, n1=n1).items()}
    out = {k: capi.DeviceBuffer(B * nmax * sz) for k, sz in dict(i0=4, i1=4, m0=8, m1=8).items()}
    sg.infer_device(B, bufs["f0"].ptr, bufs["n0"].ptr, bufs["f1"].ptr, bufs["n1"].ptr, nmax, normalize,
                    out["i0"].ptr, out["i1"].ptr, out["m0"].ptr, out["m1"].ptr, st.handle,
                    post_stream=pst.handle if post_stream else None)
    capi.synchronize()
    ok, flags = sg.status()
    assert ok, hex(flags)
    return (out["i0"].download((B, nmax), np.int32), out["i1"].download((B, nmax), np.int32),
            out["m0"].download((B, nmax), np.float64), out["m1"].download((B, nmax), np.float64))


def _sg_prime(sg, F0, F1):
    """rspl_sg_debug_scores copies (n0 + 1) x (n1 + 1) of the last HOST call's counts: make them this pair's"""
    ok, *_ = sg.infer(F0, F1)
    assert ok, sg.error


SG_MIX = {2: [(96, 95), (8, 0)], 3: [(33, 5), (1, 7), (0, 8)], 5: [(96, 95), (33, 5), (1, 7), (64, 64), (32, 31)]}


def _sg_bitwise(pkg, w, nmax, B, normalize, post_stream, mix):
    pairs = [_sg_features(a, b, seed=500 + 10 * a + b) for a, b in mix]
    if not normalize:  # the host path takes normalised keypoints
        pairs = [tuple(post.normalize_keypoints(F, 752, 480) if F.shape[1] else F for F in pr) for pr in pairs]
    sg1, sgB = _sg16(pkg, w, nmax, 1), _sg16(pkg, w, nmax, B)
    # a call with larger counts first: rows between n and nmax of every buffer hold its values afterwards
    full = [_sg_features(nmax, nmax, seed=900 + p) for p in range(B)]
    _sg_device(sgB, full, nmax, True)
    I0, I1, M0, M1 = _sg_device(sgB, pairs, nmax, normalize, post_stream)
    for p, (F0, F1) in enumerate(pairs):
        n0, n1 = F0.shape[1], F1.shape[1]
        # reference: the max_batch = 1 host path (normalize on: the same handle's one-pair device call, which is
        # what rspl_pm_match's host path enqueues)
        ok, i0, i1, m0, m1 = sg1.infer(F0, F1)
        assert ok, sg1.error
        if normalize:
            r = _sg_device(sg1, [(F0, F1)], nmax, True)
            i0, i1, m0, m1 = r[0][0, :n0], r[1][0, :n1], r[2][0, :n0], r[3][0, :n1]
            if n0 == 0 or n1 == 0:  # the host path reports an empty pair's keypoints as unmatched
                i0, i1, m0, m1 = np.full(n0, -1, np.int32), np.full(n1, -1, np.int32), np.zeros(n0), np.zeros(n1)
        Zr = sg1.debug_scores(0, n0, n1)
        tag = f"B={B} pair {p} ({n0}, {n1})"
        _bytes_equal(I0[p, :n0], i0, tag + " indices0")
        _bytes_equal(I1[p, :n1], i1, tag + " indices1")
        _bytes_equal(M0[p, :n0], m0, tag + " mscores0")
        _bytes_equal(M1[p, :n1], m1, tag + " mscores1")
        if n0 == 0 or n1 == 0:
            assert (I0[p, :n0] == -1).all() and (I1[p, :n1] == -1).all() and not M0[p, :n0].any() and not M1[p, :n1].any()
            continue  # no couplings: Z of an empty pair is not defined
        _sg_prime(sgB, F0, F1)
        _sg_device(sgB, pairs, nmax, normalize, post_stream)
        _bytes_equal(sgB.debug_scores(p, n0, n1), Zr, tag + " Z")


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalize"])
@pytest.mark.parametrize("B", [2, 3, 5])
def test_sg_fp16_batched_equals_single_bitwise(pkg, weight_blobs, B, normalize):
    _sg_bitwise(pkg, weight_blobs[1], 96, B, normalize, False, SG_MIX[B])


def test_sg_fp16_batched_post_stream_bitwise(pkg, weight_blobs):
    _sg_bitwise(pkg, weight_blobs[1], 96, 2, True, True, SG_MIX[2])


def test_sg_fp16_batched_nmax72_bitwise(pkg, weight_blobs):
    _sg_bitwise(pkg, weight_blobs[1], 72, 3, True, False, [(72, 71), (33, 0), (40, 72)])


# --------------------------------------------------------------------------------------------------------------
# 2a. SuperPoint, one stage at a time
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sp_dbg(pkg, weight_blobs):
    """limits for the largest case at every level: 136 x 200 at level 4 (conv3a) is a 544 x 800 image"""
    return _sp16(pkg, weight_blobs[0], 544, 800, 2, k=16)


@pytest.mark.parametrize("case", C.SP_CASES, ids=C.case_id)
def test_sp_stage_vs_fp64(case, sp_dbg, sp_w):
    stage, B, H, W = case
    x = C.sp_input(stage, B, H, W)
    out = sp_dbg.debug_layer(stage, x)
    if stage == "conv1":
        v, S, F = E.conv1(x, sp_w, gamma1=C.GAMMA["conv1a"])
    else:
        Wt, b, pool = E.sp_stage_weights(sp_w, stage)
        v, S = E.conv3x3(x, Wt, b, pool)
        F = 0.0
    assert out.shape == v.shape
    ratio, flips = E.check_fp16(out, v, S, C.GAMMA["conv"], extra=F)
    print(f"{C.case_id(case)}: worst |gpu - ref| / bound {ratio:.3f}, flip share {flips:.5f}")
    assert ratio <= 1.0
    assert flips <= C.FLIP_CAP


@pytest.mark.parametrize("case", C.HEAD_CASES, ids=C.case_id)
def test_sp_det_head_vs_fp64(case, sp_dbg, sp_w):
    B, H8, W8 = case
    cells = C.cells_input(B, H8, W8)
    out = sp_dbg.debug_layer("det_head", cells)
    ref, bound, _ = E.det_head(cells, sp_w)
    ratio = float((np.abs(out - ref) / bound(C.GAMMA["head"])).max())
    print(f"det_head {C.case_id(case)}: worst |gpu - ref| / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("counts", C.TAP_CASES, ids=C.case_id)
def test_sp_taps_vs_fp64(counts, sp_dbg, sp_w):
    B, H8, W8 = 2, 17, 33
    H, W = 8 * H8, 8 * W8
    cells = C.cells_input(B, H8, W8)
    scores = np.random.default_rng(5).random((B, H, W)).astype(np.float32)
    kps = [C.tap_keypoints(n, H, W, seed=11 + b) for b, n in enumerate(counts)]
    feats, cnt = sp_dbg.debug_layer("taps", cells, scores, kps)
    assert list(cnt) == list(counts)
    worst = 0.0
    for b in range(B):
        ref, bound, _ = E.taps(cells[b], scores[b], kps[b], sp_w)
        assert feats[b].shape == ref.shape
        _bytes_equal(feats[b][:, :3], ref[:, :3], f"image {b}: score, x, y")
        nan = np.isnan(ref[:, 3:])
        assert np.array_equal(np.isnan(feats[b][:, 3:]), nan)  # the degenerate corners (fp16_cases.tap_keypoints)
        ok = ~nan.any(1)
        if ok.any():
            worst = max(worst, float((np.abs(feats[b][ok, 3:] - ref[ok, 3:]) / bound(C.GAMMA["head"])[ok]).max()))
    print(f"taps {C.case_id(counts)}: worst |gpu - ref| / bound {worst:.3f}")
    assert worst <= 1.0


def test_sp_debug_layer_needs_fp16(pkg, weight_blobs):
    sp = pkg.SuperPoint(pkg.SuperPointConfig(max_keypoints=16, weights=weight_blobs[0], max_height=64, max_width=96,
                                             max_batch=1))
    assert sp.build(), sp.error
    with pytest.raises(pkg.capi.RsplError, match="RSPL_PREC_FP16"):
        sp.debug_layer("conv2a", C.sp_input("conv2a", 1, 12, 20))


# --------------------------------------------------------------------------------------------------------------
# 2b. SuperGlue, one fused GNN layer at a time
# --------------------------------------------------------------------------------------------------------------
SG_HANDLE_B = 6  # one pair more than the largest batch: the sets beyond the batch are the guard


@pytest.fixture(scope="module")
def sg_dbg(pkg, weight_blobs):
    return {96: _sg16(pkg, weight_blobs[1], 96, SG_HANDLE_B), 72: _sg16(pkg, weight_blobs[1], 72, SG_HANDLE_B),
            400: _sg16(pkg, weight_blobs[1], 400, 3)}


def _sg_layer_case(sg, w, nmax, n0, n1, l0, l1, seed, tag):
    B = len(n0)
    X = C.sg_input(2 * sg.config.max_batch, nmax, n0, n1, seed)
    Xo, Q = sg.debug_layers(B, X, n0, n1, l0, l1)
    A = E.sg_layers(w, X[:2 * B], n0, n1, l0, l1)
    sx, sq = E.sg_spread(A, E.sg_layers(w, X[:2 * B], n0, n1, l0, l1, fp32=True))
    tx, tq = C.SG_FACTOR * max(sx, C.SG_SPREAD_FLOOR), C.SG_FACTOR * max(sq, C.SG_SPREAD_FLOOR)
    # nothing outside the batch's sets is written (a tile's rows at or beyond nmax belong to the next set: the last
    # set's fall into the guard), and every row of the batch stays finite (rows at or beyond a set's count are
    # unspecified, but finite: the next call's k / v tiles read them under a zero probability)
    _bytes_equal(Xo[2 * B:], X[2 * B:], tag + ": sets beyond the batch")
    assert np.isfinite(Xo[:2 * B]).all(), tag
    rx = rq = 0.0
    for s, a in enumerate(A):
        n = a["n"]
        if n == 0:
            continue
        rx = max(rx, float((np.abs(Xo[s, :n] - a["X"]) / (tx * a["SX"])).max()))
        if Q is not None:
            assert np.isfinite(Q[s].astype(np.float64)).all(), tag
            rq = max(rq, float((np.abs(Q[s, :n].astype(np.float64) - a["q"]) / (E.ulp16(a["q"]) + tq * a["Sq"])).max()))
    print(f"sg {tag}: spread X {sx:.2e} q {sq:.2e}; worst |gpu - ref| / bound: X {rx:.3f}, q {rq:.3f}")
    assert rx <= 1.0 and rq <= 1.0
    return Xo


@pytest.mark.parametrize("layers", [(0, 1), (1, 2), (17, 18), (0, 2)], ids=lambda l: f"{l[0]}-{l[1]}")
def test_sg_layer_vs_restatement_layers(layers, sg_dbg, sg_w):
    _sg_layer_case(sg_dbg[96], sg_w, 96, [96, 33], [95, 5], *layers, seed=1, tag=f"layers {layers}")


@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_sg_layer_vs_restatement_batches(B, sg_dbg, sg_w):
    n0, n1 = C.sg_counts_for(B)
    _sg_layer_case(sg_dbg[96], sg_w, 96, n0, n1, 0, 2, seed=2, tag=f"B={B}")


@pytest.mark.parametrize("counts", C.SG_COUNTS, ids=C.case_id)
def test_sg_layer_vs_restatement_counts(counts, sg_dbg, sg_w):
    other = (64, 64) if counts != (64, 64) else (96, 95)
    _sg_layer_case(sg_dbg[96], sg_w, 96, [counts[0], other[0]], [counts[1], other[1]], 0, 2, seed=3,
                   tag=f"counts {counts}")


@pytest.mark.parametrize("nmax,counts", [(72, [(72, 71), (33, 5)]), (400, [(400, 380), (64, 64)])], ids=["72", "400"])
def test_sg_layer_vs_restatement_nmax(nmax, counts, sg_dbg, sg_w):
    _sg_layer_case(sg_dbg[nmax], sg_w, nmax, [c[0] for c in counts], [c[1] for c in counts], 0, 2, seed=4,
                   tag=f"nmax {nmax}")


def test_sg_layer_unwritten_rows(sg_dbg, sg_w):
    """nmax = 72: the third 32-token tile of a set covers rows 64 .. 95, of which 72 .. 95 are the NEXT set's first
    rows.  With B = 5 (2-D grid) and B = 2 (XCD placement) the sets beyond the batch keep their sentinel bytes and an
    empty set's rows are left as they were (finite)."""
    for B in (2, 5):
        n0, n1 = [72, 0, 40, 1, 72][:B], [0, 72, 72, 71, 8][:B]
        Xo = _sg_layer_case(sg_dbg[72], sg_w, 72, n0, n1, 0, 2, seed=5, tag=f"unwritten rows B={B}")
        assert np.isfinite(Xo).all()
