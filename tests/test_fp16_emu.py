"""CPU checks of oracle/fp16_emu.py: the moved whole-network emulation is unchanged, and the single-stage
restatements' own accumulation-order spread stays inside what tests/fp16_cases.py builds the GPU tolerances on
(GAMMA0, FLIP_CAP, the SuperGlue spread), at every shape the GPU tests use."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import fp16_cases as C
import fp16_emu as E

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def sp_w(weight_blobs):
    from rspl_slam_amd import weights as W
    return W.read_blob(weight_blobs[0])


@pytest.fixture(scope="module")
def sg_w(weight_blobs):
    from rspl_slam_amd import weights as W
    return W.read_blob(weight_blobs[1])


def test_moved_emu_reproduces_old_forward(golden, weight_blobs, tmp_path):
    """Emu.forward, as tools/sp_fp16_split.py ran it before the move, on one 64 x 96 image (fp16_all and fp32_all).
    In a child process: the emulation needs torch, which must not meet librspl's HIP runtime in the test process."""
    g = golden("sp_fp16_emu")
    np.save(tmp_path / "img.npy", g["image"])
    code = ("import sys, numpy as np\n"
            f"sys.path[:0] = [{str(ROOT)!r}, {str(ROOT / 'oracle')!r}]\n"
            "import fp16_emu as E\n"
            f"emu = E.Emu({weight_blobs[0]!r})\n"
            f"img = np.load({str(tmp_path / 'img.npy')!r})\n"
            f"np.savez({str(tmp_path / 'out.npz')!r}, fp16_all=emu.forward(img, set(E.ENC + E.HEADS)),\n"
            "         fp32_all=emu.forward(img, set()))\n")
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)
    out = np.load(tmp_path / "out.npz")
    for k in ("fp16_all", "fp32_all"):
        np.testing.assert_array_equal(out[k], g[k], err_msg=k)


def _spread(v64, S, variants):
    """largest |v - v64| / (2^-24 S) and flip share of h16(v) against h16(v64) over the fp32-order variants"""
    g0 = max(float((np.abs(v - v64) / (E.U24 * S)).max()) for v in variants)
    flips = max(float((E.h16(v) != E.h16(v64)).mean()) for v in variants)
    return g0, flips


@pytest.mark.parametrize("case", C.SP_CASES, ids=C.case_id)
def test_reference_spread(case, sp_w):
    stage, B, H, W = case
    x = C.sp_input(stage, B, H, W)
    if stage == "conv1":
        v64, S, _ = E.conv1(x, sp_w)
        var = [E.conv1(x, sp_w, order=o)[0] for o in ("f32", "perm")]
        g1 = max(float((d / (E.U24 * S1)).max()) for d, S1 in (E.conv1a_spread(x, sp_w, o) for o in ("f32", "perm")))
        print(f"{C.case_id(case)}: conv1a gamma0 {g1:.3f}")
        assert g1 <= C.GAMMA0["conv1a"]
        # conv1b's own order spread on the same (fp64-rounded) conv1a output: v differs from v64 through conv1a's
        # flips too, which the F allowance of the GPU test covers, so hold the variants to GAMMA0 S + F(GAMMA0)
        _, _, F = E.conv1(x, sp_w, gamma1=C.GAMMA0["conv1a"])
        r = max(float((np.abs(v - v64) / (C.GAMMA0["conv"] * E.U24 * S + F)).max()) for v in var)
        flips = max(float((E.h16(v) != E.h16(v64)).mean()) for v in var)
        print(f"{C.case_id(case)}: conv1 spread / (gamma0 S + F) {r:.3f}, flip share {flips:.5f}")
        assert r <= 1.0 and flips <= C.FLIP_CAP
        return
    Wt, b, pool = E.sp_stage_weights(sp_w, stage)
    v64, S = E.conv3x3(x, Wt, b, pool)
    g0, flips = _spread(v64, S, [E.conv3x3(x, Wt, b, pool, o)[0] for o in ("f32", "perm")])
    print(f"{C.case_id(case)}: gamma0 {g0:.3f}, flip share {flips:.5f}")
    assert g0 <= C.GAMMA0["conv"] and flips <= C.FLIP_CAP


@pytest.mark.parametrize("case", C.HEAD_CASES, ids=C.case_id)
def test_reference_spread_heads(case, sp_w):
    B, H8, W8 = case
    cells = C.cells_input(B, H8, W8)
    p64, bound, (z64, S) = E.det_head(cells, sp_w)
    for o in ("f32", "perm"):
        p, _, (z, _) = E.det_head(cells, sp_w, o)
        g0 = float((np.abs(z - z64) / (E.U24 * S)).max())
        r = float((np.abs(p - p64) / bound(C.GAMMA0["head"])).max())
        print(f"det_head {C.case_id(case)} {o}: logits gamma0 {g0:.3f}, scores / bound(gamma0) {r:.3f}")
        assert g0 <= C.GAMMA0["head"] and r <= 1.0
    if H8 == 1:
        return  # one cell: no bilinear neighbourhood (all four tap weights vanish); taps run at 17 x 33 only
    H, W = 8 * H8, 8 * W8
    kp = C.tap_keypoints(9, H, W, 3)
    sc = np.zeros((H, W), np.float32)
    F64, tb, (d64, Sd) = E.taps(cells[0], sc, kp, sp_w)
    for o in ("f32", "perm"):
        F, _, (d, _) = E.taps(cells[0], sc, kp, sp_w, o)
        g0 = float((np.abs(d - d64) / (E.U24 * Sd)).max())
        ok = ~np.isnan(F64[:, 3])  # the degenerate corners (fp16_cases.tap_keypoints)
        assert ok.sum() == 6 and np.array_equal(np.isnan(F[:, 3:]), np.isnan(F64[:, 3:]))
        r = float((np.abs(F[ok, 3:] - F64[ok, 3:]) / tb(C.GAMMA0["head"])[ok]).max())
        print(f"taps {C.case_id(case)} {o}: descriptor gamma0 {g0:.3f}, features / bound(gamma0) {r:.3f}")
        assert g0 <= C.GAMMA0["head"] and r <= 1.0
        np.testing.assert_array_equal(F[:, :3], F64[:, :3])


SG_SPREAD_CASES = [("l0", 96, 0, 1), ("l1", 96, 1, 2), ("l17", 96, 17, 18), ("l0-2", 96, 0, 2), ("nmax72", 72, 0, 2),
                   ("nmax400", 400, 0, 2)]


@pytest.mark.parametrize("case", SG_SPREAD_CASES, ids=lambda c: c[0])
def test_sg_restatement_spread(case, sg_w):
    """The two variants of the fused-layer restatement (fp64 / final maximum, fp32 / online softmax) agree to a
    fraction of an fp16 ulp of the terms; the GPU tolerance is SG_FACTOR times this spread (floored), so it must stay small enough
    that a wrong key mask or a dropped tile cannot hide: below 2^-11 S (every term off by an fp16 ulp), when one
    key of 96 carries about 1e-2 of a message."""
    _, nmax, l0, l1 = case
    if nmax == 400:
        n0, n1 = [400, 64], [380, 64]
    elif nmax == 72:
        n0, n1 = [72, 33], [71, 5]
    else:
        n0, n1 = [c[0] for c in C.SG_COUNTS], [c[1] for c in C.SG_COUNTS]
    X = C.sg_input(2 * len(n0), nmax, n0, n1, seed=9)
    A = E.sg_layers(sg_w, X, n0, n1, l0, l1)
    Bv = E.sg_layers(sg_w, X, n0, n1, l0, l1, fp32=True)
    rx, rq = E.sg_spread(A, Bv)
    print(f"sg {case[0]}: spread X {rx:.3e} S, q {rq:.3e} S")
    assert all(np.isfinite(a["X"]).all() for a in A)
    assert rx < C.SG_SPREAD_CAP and rq < C.SG_SPREAD_CAP
