"""Shapes, inputs and tolerances shared by tests/test_fp16_emu.py (CPU: the reference's own spread) and
tests/test_gpu_fp16.py (GPU: the fp16 kernels against the fp64-accumulated restatements of oracle/fp16_emu.py).

Tolerances.  A stage with an fp16 output must satisfy, per element,
    |gpu - ref| <= ulp16(ref) + GAMMA * 2^-24 * S,          GAMMA = 4 * GAMMA0,
where GAMMA0 bounds what the restatement's own two fp32 accumulation orders (numpy's sgemm per tap, and the same
with the input channels permuted and the taps reversed) differ from its fp64 accumulation by, in units of
2^-24 * S; the factor 4 covers the MFMA's blocked order, which neither CPU order reproduces.  GAMMA0 is asserted on
every CPU run (test_fp16_emu.py) at every shape below.  Largest values measured there:
    "conv"    3x3, K = 576: 1.36 (conv3a 136 x 200)    K = 1152: 1.57 (convPD 17 x 33)      -> GAMMA0 2.0, GAMMA 8
    "head"    1x1, K = 256: convPb 3.34, convDb 3.55 (few rows: sgemm sums them nearly in sequence) -> 4.0, 16
    "conv1a"  K = 10, one addition per tap in fp32: 3.83                                      -> 4.0, 16
(rounded up: the maximum over 10^5 .. 10^7 outputs still creeps with the sample and with the BLAS at hand).  The
guaranteed worst case is K * 2^-24 * S, so GAMMA stays far below K for the convolutions and heads: a dropped tap
cannot pass.  conv1a's GAMMA only decides WHICH of its fp16 outputs may round to the other neighbour (fp16_emu.conv1's
allowance F); a wrong tap moves an output by far more than one fp16 ulp and is not covered by it.
At most FLIP_CAP of a stage's fp16 outputs may differ from the rounded reference at all; the two fp32 orders flip at
most 0.08 % of them on these inputs (0.2 % for convPD 1 x 1, one of 512, and for conv1, whose intermediate fp16
rounding feeds 576 products per output).

SuperGlue's fused layer rounds to fp16 inside one launch (the probabilities, the message, the hidden layer, the fp16
shadow of x), so its outputs move by fp16 ulps of their terms, far more than fp32 roundoff.  Its tolerance is
SG_FACTOR = 4 times the restatement's own spread between its fp64 variant (probabilities relative to the row's final
maximum) and its fp32 variant (online softmax in 32-key tiles, two partial states), as a ratio to S = sum |terms| of
the row, computed per case by both tests.  Measured spreads (X, next q), in units of S:
    layer 0: 7.1e-5, 7.4e-5    layer 1: 7.5e-5, 5.7e-5    layer 17: 6.7e-5    layers [0, 2): 1.4e-4, 7.4e-5
    nmax 72: 1.2e-4, 5.9e-5    nmax 400: 1.3e-4, 6.1e-5
The CPU test caps the spread at SG_SPREAD_CAP = 2^-11 (every term off by a whole fp16 ulp); one wrongly admitted key
of 96 moves a message by about 1e-2 of its size.  SG_SPREAD_FLOOR (one flipped hidden value carrying 4 % of S:
0.04 * 2^-11) keeps the bound from collapsing where a tiny case happens to show no flip at all.
"""
import numpy as np

import fp16_emu as E

GAMMA0 = {"conv": 2.0, "conv1a": 4.0, "head": 4.0}
GAMMA = {k: 4 * v for k, v in GAMMA0.items()}
FLIP_CAP = 0.005
SG_FACTOR = 4.0
SG_SPREAD_CAP = 2.0 ** -11
SG_SPREAD_FLOOR = 2.0e-5

# (stage, B, H, W) at the stage's own input level
SP_CASES = [
    ("conv1", 1, 8, 8), ("conv1", 2, 24, 40), ("conv1", 2, 136, 264),
    ("conv2b", 2, 12, 20), ("conv2b", 2, 68, 132),
    ("conv2a", 2, 12, 20), ("conv2a", 2, 34, 66), ("conv2a", 2, 136, 200),
    ("conv3a", 2, 12, 20), ("conv3a", 2, 34, 66), ("conv3a", 2, 136, 200),
    ("conv3b", 2, 6, 10), ("conv3b", 2, 34, 66),
    ("conv4a", 1, 1, 1), ("conv4a", 2, 17, 33), ("conv4a", 1, 129, 191),
    ("conv4b", 1, 1, 1), ("conv4b", 2, 17, 33), ("conv4b", 1, 129, 191),
    ("convPD", 1, 1, 1), ("convPD", 2, 17, 33), ("convPD", 1, 129, 191),
]
HEAD_CASES = [(1, 1, 1), (2, 17, 33)]  # (B, H8, W8): P = 1; P = 561 (waves and 128-cell blocks straddle the images)
CIN = {"conv2a": 64, "conv2b": 64, "conv3a": 64, "conv3b": 128, "conv4a": 128, "conv4b": 128, "convPD": 128}


def case_id(c):
    return "-".join(str(v) for v in c)


def sp_input(stage, B, H, W):
    rng = np.random.default_rng(1000 + 7 * B + 31 * H + W + sum(map(ord, stage)))
    if stage == "conv1":
        return rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    return E.relu_like(rng, (B, H, W, CIN[stage]))


def cells_input(B, H8, W8):
    return E.relu_like(np.random.default_rng(50 + B + H8 * W8), (B, H8, W8, 512))


# taps: keypoint counts per image of a B = 2 batch on a 17 x 33 cell grid (8 keypoints per workgroup)
TAP_CASES = [(9, 0), (0, 8), (1, 7)]


def tap_keypoints(n, H, W, seed):
    """n flat pixel indices: the four corners and border pixels first (their taps clamp), then interior ones.
    Left of / above the first cell centre the clamped taps extrapolate (weights outside [0, 1]); right of / below the
    last one (x > W - 4.5) both columns clamp to the same cell and every weight of src/super_point.cpp:294-332 is 0:
    the blend is the zero vector and its normalisation 0 / 0, NaN in the reference and in the kernel alike (the
    product never samples there with remove_borders >= 4)."""
    fixed = [0, W - 1, (H - 1) * W, H * W - 1, 5, 3 * W, 5 * W - 5, (H - 5) * W + 17, (H // 2) * W + W // 2]
    rng = np.random.default_rng(seed)
    return (fixed + list(rng.integers(0, H * W, 16)))[:n] if n != 1 else [H * W - 1]


# SuperGlue
SG_COUNTS = [(96, 95), (64, 64), (33, 5), (32, 31), (1, 1), (1, 7), (0, 8), (8, 0)]
SG_SENTINEL = 1.75  # rows at or beyond a set's count (finite: prep writes zeros there, a layer keeps them finite)


def sg_input(nsets_total, nmax, n0, n1, seed):
    """X [nsets_total, nmax, 256]: unit-scale descriptors below each set's count, the sentinel elsewhere (the sets
    beyond the batch included)"""
    rng = np.random.default_rng(seed)
    X = np.full((nsets_total, nmax, 256), SG_SENTINEL, np.float32)
    for p, (a, b) in enumerate(zip(n0, n1)):
        X[2 * p, :a] = rng.standard_normal((a, 256)) * 0.6
        X[2 * p + 1, :b] = rng.standard_normal((b, 256)) * 0.6
    return X


def sg_counts_for(B):
    """a ragged mix for a batch of B pairs"""
    mix = [(96, 95), (33, 5), (1, 7), (64, 64), (32, 31)]
    return [m[0] for m in mix[:B]], [m[1] for m in mix[:B]]
