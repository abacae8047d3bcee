"""fp16 EMULATION (test infrastructure only) -- CPU restatements of librspl's RSPL_PREC_FP16 kernels.

Two parts:

1. `Emu`: the whole-network SuperPoint emulation of tools/sp_fp16_split.py (moved here unchanged; it needs
   torch and the CPU oracle and is imported by that tool only).

2. Single-stage restatements in numpy (no torch: the GPU tests import them beside librspl).  Each takes the
   stage's fp16-representable operands and returns the result ACCUMULATED IN FP64 before the stage's final
   rounding, with the magnitude sum S = sum |x| |w| + |b| of every output, so that a kernel's fp32 accumulation
   can be held to   |gpu - ref| <= ulp16(ref) + gamma * 2^-24 * S   per element (fp16 outputs; fp32 outputs
   have no ulp term).  `order="f32"` / `order="perm"` evaluate the same stage with fp32 accumulation in two
   different orders (numpy's own; input channels permuted and taps reversed): the reference's own
   accumulation-order spread gamma0, measured by tests/test_fp16_emu.py, is the basis of gamma = 4 gamma0.

Where the kernels round (rspl-slam_amd/csrc/sp_conv.hip, sp_heads.hip, sg_gemm.hip, sg_gnn.hip):
  conv3x3_h_kernel     fp16 x, fp16 w; fp32 accumulation; (2x2 max-pool of the accumulators;) + fp32 bias; ReLU;
                       rounded to fp16.
  conv1_res_kernel     pixel (float)(u / 255.0) rounded to fp16; conv1a = one MFMA over the 9 fp16 taps and the
                       bias as a tenth fp16 tap (input 1); ReLU; fp16.  Then conv1b as conv3x3_h_kernel with pool.
                       The intermediate fp16 rounding makes this a two-layer stage: where conv1a's fp32 sum may
                       round to the other neighbour than the fp64 sum, conv1b's input differs by an fp16 ulp.
                       conv1() returns that propagated allowance separately (F).
  det_head_h_kernel    cells[:, :256] fp16 x fp16 convPb, fp32 accumulation, + fp32 bias; softmax over 65 in fp32;
                       dustbin dropped; depth-to-space.
  sample_taps_h_kernel cells[:, 256:] fp16 x fp16 convDb at the 4 bilinear taps, fp32 accumulation + fp32 bias;
                       per tap L2 normalisation in fp32; bilinear blend and final normalisation in fp64.
  layer_kernel         see sg_layers().
"""
from __future__ import annotations

import numpy as np

U24 = 2.0 ** -24  # unit roundoff of fp32


def h16(a, dtype=np.float64):
    """round to fp16 (nearest even), carried in `dtype`"""
    return np.asarray(a).astype(np.float16).astype(dtype)


def ulp16(v):
    """spacing of fp16 at |v| (subnormal spacing 2^-24 below 2^-14)"""
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    return np.ldexp(1.0, np.maximum(e - 11, -24))


def relu_like(rng, shape, zero_frac=0.3, scale=1.0):
    """post-ReLU-like fp16-representable activations: non-negative, about zero_frac exact zeros"""
    x = np.abs(rng.standard_normal(shape)) * scale
    x[rng.random(shape) < zero_frac] = 0.0
    return h16(x, np.float32)


# --------------------------------------------------------------------------------------------------------------
# SuperPoint stages
# --------------------------------------------------------------------------------------------------------------
SP_CONVS = {"conv2a": ("conv2a", False), "conv2b": ("conv2b", True), "conv3a": ("conv3a", False),
            "conv3b": ("conv3b", True), "conv4a": ("conv4a", False), "conv4b": ("conv4b", False),
            "convPD": (("convPa", "convDa"), False)}


def sp_stage_weights(w, stage):
    """(fp16-rounded weight [Cout, Cin, 3, 3] float64, fp32 bias [Cout] float64, pool) of a 3x3 stage from the
    state dict (convPD = convPa | convDa side by side, as sp.cpp fuses them)"""
    names, pool = SP_CONVS[stage] if stage != "conv1b" else ("conv1b", True)
    names = (names,) if isinstance(names, str) else names
    W = np.concatenate([w[n + ".weight"] for n in names]).astype(np.float32)
    b = np.concatenate([w[n + ".bias"] for n in names]).astype(np.float32)
    return h16(W), b.astype(np.float64), pool


def _conv_acc(x, W, order):
    """sum over taps and input channels of x [B, H, W, Cin] (zero padded) with W [Cout, Cin, 3, 3] -> [B, H, W, Cout]
    order None: fp64; "f32": fp32, taps in order; "perm": fp32, taps reversed and input channels permuted"""
    dt = np.float64 if order is None else np.float32
    B, H, Wd, C = x.shape
    xp = np.pad(np.asarray(x, dt), ((0, 0), (1, 1), (1, 1), (0, 0)))
    Wt = np.asarray(W, dt)
    perm = np.random.default_rng(12345).permutation(C) if order == "perm" else np.arange(C)
    taps = range(9) if order != "perm" else range(8, -1, -1)
    acc = np.zeros((B * H * Wd, Wt.shape[0]), dt)
    for kk in taps:
        ky, kx = divmod(kk, 3)
        a = xp[:, ky:ky + H, kx:kx + Wd, :].reshape(-1, C)[:, perm]
        acc += a @ np.ascontiguousarray(Wt[:, perm, ky, kx].T)
    return acc.reshape(B, H, Wd, -1)


def _pool(a):
    B, H, W, C = a.shape
    return a.reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def conv3x3(x, W, b, pool, order=None):
    """One conv3x3_h_kernel stage.  x [B, H, W, Cin] and W fp16-representable, b fp32.
    Returns (v, S): v = ReLU(pool(acc) + b) before the fp16 rounding (the kernel stores h16(v)) and S = the
    magnitude sum per output (pooled: the maximum over the window, since |max a - max a'| <= max |a - a'|)."""
    acc = _conv_acc(x, W, order)
    S = _conv_acc(np.abs(x), np.abs(W), None) + np.abs(b)
    if pool:
        acc, S = _pool(acc), _pool(S)
    v = acc.astype(np.float64) + b if order is None else (acc + b.astype(np.float32)).astype(np.float64)
    return np.maximum(v, 0.0), S


def conv1(img_u8, w, gamma1=0.0, order=None):
    """conv1_res_kernel: u8 [B, H, W] -> (v, S, F) at [B, H/2, W/2, 64].
    v, S as conv3x3 for conv1b on the fp64-accumulated, fp16-rounded conv1a output.  F >= 0: the change of conv1b's
    sum if every conv1a output whose fp16 rounding is undecided within +-gamma1 2^-24 S1a (S1a its own magnitude
    sum) took the other neighbour -- the allowance for the stage's intermediate rounding (0 with gamma1 = 0)."""
    p = h16((np.asarray(img_u8, np.float64) / 255.0).astype(np.float32))[..., None]  # LUT value, then fp16 A operand
    W1a, b1a = h16(w["conv1a.weight"]), h16(w["conv1a.bias"])                           # bias: the tenth fp16 tap
    a = _conv_acc(p, W1a, order).astype(np.float64)
    a = a + b1a if order is None else (a.astype(np.float32) + b1a.astype(np.float32)).astype(np.float64)
    S1 = _conv_acc(np.abs(p), np.abs(W1a), None) + np.abs(b1a)
    h = h16(np.maximum(a, 0.0))
    W1b, b1b, _ = sp_stage_weights(w, "conv1b")
    v, S = conv3x3(h, W1b, b1b, True, order)
    e = gamma1 * U24 * S1
    D = np.abs(h16(np.maximum(a + e, 0.0)) - h16(np.maximum(a - e, 0.0)))
    F = _pool(_conv_acc(D, np.abs(W1b), None)) if gamma1 > 0 else np.zeros_like(S)
    return v, S, F


def conv1a_spread(img_u8, w, order):
    """(|fp32-order conv1a sum - fp64 sum|, S1a) for the reference-spread test"""
    p = h16((np.asarray(img_u8, np.float64) / 255.0).astype(np.float32))[..., None]
    W1a, b1a = h16(w["conv1a.weight"]), h16(w["conv1a.bias"])
    a64 = _conv_acc(p, W1a, None) + b1a
    a32 = (_conv_acc(p, W1a, order) + b1a.astype(np.float32)).astype(np.float64)
    return np.abs(a32 - a64), _conv_acc(np.abs(p), np.abs(W1a), None) + np.abs(b1a)


def check_fp16(out, v, S, gamma, extra=0.0):
    """out (fp16 values) against the pre-rounding reference v: (worst |out - v| / bound, share of elements that
    differ from h16(v) at all), bound = ulp16(v) + gamma 2^-24 S + extra"""
    out = np.asarray(out, np.float64)
    bound = ulp16(v) + gamma * U24 * S + extra
    return float((np.abs(out - v) / bound).max()), float((out != h16(v)).mean())


def _gemm(a, Wt, order):
    """a [M, K] @ Wt [K, N]; order as _conv_acc (perm: K permuted)"""
    dt = np.float64 if order is None else np.float32
    K = a.shape[1]
    perm = np.random.default_rng(777).permutation(K) if order == "perm" else np.arange(K)
    return np.asarray(a, dt)[:, perm] @ np.ascontiguousarray(np.asarray(Wt, dt)[perm])


def det_head(cells, w, order=None):
    """det_head_h_kernel: cells [B, H8, W8, 512] -> (scores [B, 8 H8, 8 W8], bound(gamma) -> same shape,
    (logits, S)).
    logits z_c = sum_k x_k w_ck + b_c with |dz_c| <= gamma 2^-24 S_c; p = softmax(z) to first order moves by
    |dp_i| <= p_i (|dz_i| + sum_j p_j |dz_j|).  The kernel's fp32 softmax itself (x - m rounded: <= |x - m| 2^-24
    relative in e; expf <= 2 ulp; the 65-term sum as 3 in-lane + 5 shuffle additions <= 8 ulp, once for the own e
    and once through the division; the division <= 1 ulp) adds <= (16 + max_j |z_j - m|) 2^-24 p_i."""
    B, H8, W8, _ = cells.shape
    x = np.asarray(cells, np.float64).reshape(-1, 512)[:, :256]
    Wt = h16(w["convPb.weight"]).reshape(65, 256).T
    b = w["convPb.bias"].astype(np.float64)
    z = _gemm(x, Wt, order).astype(np.float64) + b
    S = np.abs(x) @ np.abs(Wt) + np.abs(b)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    p = e / e.sum(1, keepdims=True)

    def d2s(a):  # [B*P, 64] -> [B, 8 H8, 8 W8] (superpoint.py:133-135)
        return a.reshape(B, H8, W8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(B, H8 * 8, W8 * 8)

    def bound(gamma):
        dz = gamma * U24 * S
        dp = p * (dz + (p * dz).sum(1, keepdims=True)) + (16.0 + (m - z).max(1, keepdims=True)) * U24 * p
        return d2s(dp[:, :64])
    return d2s(p[:, :64]), bound, (z, S)


def tap_geometry(x, y, h, w):
    """the 4 bilinear taps (cells, weights) of pixel (x, y) on an h x w cell grid: normalize_keypoints and
    grid_sample of src/super_point.cpp:276-332 exactly as sample_taps_h_kernel evaluates them in double"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    gx = (x - 4 + 0.5) / (w * 8 - 4 - 0.5) * 2 - 1
    gy = (y - 4 + 0.5) / (h * 8 - 4 - 0.5) * 2 - 1
    ix, iy = ((gx + 1) / 2) * (w - 1), ((gy + 1) / 2) * (h - 1)
    cl = lambda v, m: np.clip(v, 0, m - 1)  # noqa: E731
    ix_nw, iy_nw = cl(np.floor(ix).astype(np.int64), w), cl(np.floor(iy).astype(np.int64), h)
    ix_ne, iy_ne = cl(ix_nw + 1, w), cl(iy_nw, h)
    ix_sw, iy_sw = cl(ix_nw, w), cl(iy_nw + 1, h)
    ix_se, iy_se = cl(ix_nw + 1, w), cl(iy_nw + 1, h)
    wt = np.stack([(ix_se - ix) * (iy_se - iy), (ix - ix_sw) * (iy_sw - iy), (ix_ne - ix) * (iy - iy_ne),
                   (ix - ix_nw) * (iy - iy_nw)], -1)
    c = np.stack([iy_nw * w + ix_nw, iy_ne * w + ix_ne, iy_sw * w + ix_sw, iy_se * w + ix_se], -1)
    return c, wt


def taps(cells, scores, keypoints, w, order=None):
    """sample_taps_h_kernel for one image: cells [H8, W8, 512], scores [8 H8, 8 W8], keypoints = flat pixel indices.
    Returns (F [n, 259], bound(gamma) -> [n, 256] on the descriptor columns, (tap descriptors d, S)).  First order, per tap: d_c = sum_k x_k
    w_ck + b_c with |dd_c| <= gamma 2^-24 S_c; u = d / |d| moves by |du_c| <= (|dd_c| + |u_c| sum_j |u_j| |dd_j|) /
    |d|, and the fp32 evaluation of |d| and the division (256 squares, 10 additions deep, sqrt, divide: <= 8 ulp)
    adds 8 2^-24 |u_c|.  The fp64 blend v = sum_t wt_t u_t moves by e_c = sum_t |wt_t| |du_tc|, and the final f =
    v / |v| by (e_c + |f_c| sum_j |f_j| e_j) / |v|."""
    H8, W8, _ = cells.shape
    Wd = 8 * W8
    kp = np.asarray(keypoints, np.int64)
    n = kp.size
    ys, xs = kp // Wd, kp % Wd
    F = np.zeros((n, 259))
    F[:, 0] = np.asarray(scores, np.float32).reshape(-1)[kp].astype(np.float64)
    F[:, 1], F[:, 2] = xs, ys
    if n == 0:
        return F, (lambda gamma: np.zeros((0, 256))), (np.zeros((0, 256)), np.ones((0, 256)))
    c, wt = tap_geometry(xs, ys, H8, W8)
    x = np.asarray(cells, np.float64).reshape(-1, 512)[c.reshape(-1), 256:]
    Wt = h16(w["convDb.weight"]).reshape(256, 256).T
    b = w["convDb.bias"].astype(np.float64)
    d = _gemm(x, Wt, order).astype(np.float64) + b
    S = np.abs(x) @ np.abs(Wt) + np.abs(b)
    nd = np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    u = d / nd
    v = (u.reshape(n, 4, 256) * wt[:, :, None]).sum(1)
    nv = np.linalg.norm(v, axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        F[:, 3:] = v / nv  # 0 / 0 = NaN where every tap weight vanishes, as in the kernel

    def bound(gamma):
        dd = gamma * U24 * S
        du = (dd + np.abs(u) * (np.abs(u) * dd).sum(1, keepdims=True)) / nd + 8 * U24 * np.abs(u)
        e = (du.reshape(n, 4, 256) * np.abs(wt)[:, :, None]).sum(1)
        f = np.abs(F[:, 3:])
        with np.errstate(invalid="ignore", divide="ignore"):
            return (e + f * (f * e).sum(1, keepdims=True)) / nv
    return F, bound, (d, S)


# --------------------------------------------------------------------------------------------------------------
# SuperGlue: the fused GNN layer (layer_kernel)
# --------------------------------------------------------------------------------------------------------------
SG_LAYERS = 18


def sg_layer_weights(w, l):
    """The fp16 engine's operands of GNN layer l as sg.cpp lays them out (:172-238): head-contiguous q | k | v
    columns (o = j 256 + h 64 + d from channel d 4 + h), BatchNorm folded into mlp.0, attn.merge folded into mlp.0's
    message half (W1m, b1m).  Weights fp16-rounded [K, N] float64, biases fp32."""
    p = f"gnn.layers.{l}."
    f64 = lambda n: w[p + n].astype(np.float64)  # noqa: E731
    c = (np.arange(64)[None, :] * 4 + np.arange(4)[:, None]).reshape(-1)  # column h 64 + d <- channel d 4 + h
    Wqkv = np.concatenate([w[p + f"attn.proj.{j}.weight"].reshape(256, 256)[c].T for j in range(3)], 1)
    bqkv = np.concatenate([w[p + f"attn.proj.{j}.bias"][c] for j in range(3)])
    sc = f64("mlp.1.weight") / np.sqrt(f64("mlp.1.running_var") + 1e-5)
    sh = f64("mlp.1.bias") - f64("mlp.1.running_mean") * sc
    w0 = f64("mlp.0.weight").reshape(512, 512)
    wmt = w[p + "attn.merge.weight"].reshape(256, 256)[:, c].T.astype(np.float64)  # [h 64 + d][o]
    w1x = (sc[None, :] * w0[:, :256].T).astype(np.float32)                         # [k][o], as w1t
    w1d = sc[None, :] * w0[:, 256:].T                                             # message half [m][o]
    w1m = (wmt @ w1d).astype(np.float32)
    b1m = (sc * f64("mlp.0.bias") + sh + (sc[:, None] * w0[:, 256:] * f64("attn.merge.bias")[None, :]).sum(1))
    return {"Wqkv": h16(Wqkv.astype(np.float32)), "bqkv": bqkv.astype(np.float64),
            "W1": h16(np.concatenate([w1x, w1m])), "b1": b1m.astype(np.float32).astype(np.float64),
            "W2": h16(w[p + "mlp.3.weight"].reshape(256, 512).T.astype(np.float32)), "b2": f64("mlp.3.bias")}


def _attention(q, k, v, fp32):
    """one head: q [nq, 64], k / v [nk, 64] fp16 values -> (message o / L before its fp16 rounding [nq, 64])
    fp64 variant: probabilities relative to the row's final maximum, rounded to fp16 for P V, the normaliser sums the
    unrounded ones.  fp32 variant: layer_kernel's online softmax over 32-key tiles, even and odd tiles as two partial
    states (m, l, o) merged at the end."""
    nq, nk = q.shape[0], k.shape[0]
    if nk == 0:
        return np.zeros((nq, 64))
    if not fp32:
        s = (q @ k.T) * 0.125
        p = np.exp(s - s.max(1, keepdims=True))
        return (h16(p) @ v) / p.sum(1, keepdims=True)
    f = np.float32
    q, k, v = q.astype(f), k.astype(f), v.astype(f)
    st = []
    for part in range(2):
        m, l, o = np.full(nq, -np.inf, f), np.zeros(nq, f), np.zeros((nq, 64), f)
        for t in range(part, (nk + 31) // 32, 2):
            x = (q @ k[32 * t:32 * t + 32].T) * f(0.125)
            mn = np.maximum(m, x.max(1))
            with np.errstate(invalid="ignore"):
                al = np.where(np.isinf(m), f(0), np.exp(m - mn)).astype(f)
            x = np.exp(x - mn[:, None]).astype(f)
            l = l * al + x.sum(1, dtype=f)
            o = o * al[:, None] + h16(x, f) @ v[32 * t:32 * t + 32]
            m = mn
        st.append((m, l, o))
    (m0, l0, o0), (m1, l1, o1) = st
    M = np.maximum(m0, m1)
    with np.errstate(invalid="ignore"):
        e0 = np.where(np.isinf(m0), f(0), np.exp(m0 - M)).astype(f)
        e1 = np.where(np.isinf(m1), f(0), np.exp(m1 - M)).astype(f)
    L = e0 * l0 + e1 * l1
    return ((e0[:, None] * o0 + e1[:, None] * o1) * (f(1) / L)[:, None]).astype(np.float64)


def sg_layers(w, X, n0, n1, l0, l1, fp32=False):
    """rspl_sg_debug_layers restated: X [2 B, nmax, 256] fp32 (set 2p / 2p + 1 = images 0 / 1 of pair p), counts per
    pair, layers [l0, l1).  layer_kernel's roundings: Xh = h16(X); q, k, v = h16(Xh W + b); scores * 0.125, softmax;
    probabilities fp16 for P V, normaliser unrounded; message = h16(o / L) (0 when the source set is empty);
    hidden = h16(ReLU([Xh | message] W1m + b1m)); X += hidden W2 + b2 in fp32; Xh = h16(X).
    fp32 = False: every accumulation in fp64; True: in fp32 with the online softmax (_attention).
    Only rows below a set's count are computed (the rest of the kernel's output is unspecified).
    Returns per set a dict: n, X (new, unrounded in the fp64 variant), SX = |hidden| |W2| + |b2| + |X old|, and when
    l1 < 18 q (the next layer's q before its fp16 rounding) and Sq = |Xh| |Wq| + |bq|."""
    acc = np.float32 if fp32 else np.float64
    mm = lambda a, Wt: (a.astype(acc) @ Wt.astype(acc)).astype(np.float64)  # noqa: E731
    nset = X.shape[0]
    cnt = [int((n1 if s & 1 else n0)[s >> 1]) for s in range(nset)]
    Xc = [np.asarray(X[s][:cnt[s]], np.float32).astype(np.float64) for s in range(nset)]
    L = sg_layer_weights(w, l0)
    add = (lambda a, b: (a.astype(np.float32) + b.astype(np.float32)).astype(np.float64)) if fp32 else (lambda a, b: a + b)
    qkv = [h16(add(mm(h16(x), L["Wqkv"]), L["bqkv"])) for x in Xc]
    out = None
    for l in range(l0, l1):
        L = sg_layer_weights(w, l)
        Ln = sg_layer_weights(w, l + 1) if l + 1 < SG_LAYERS else None
        newX, newqkv, out = [], [], []
        for s in range(nset):
            src = s ^ 1 if l & 1 else s
            n = cnt[s]
            msg = np.concatenate([_attention(qkv[s][:, 64 * h:64 * h + 64], qkv[src][:, 256 + 64 * h:320 + 64 * h],
                                             qkv[src][:, 512 + 64 * h:576 + 64 * h], fp32) for h in range(4)], 1)
            a = np.concatenate([h16(Xc[s]), h16(msg)], 1)
            hid = h16(np.maximum(add(mm(a, L["W1"]), L["b1"]), 0.0))
            d = add(mm(hid, L["W2"]), L["b2"])
            xn = add(Xc[s], d)
            r = {"n": n, "X": xn, "SX": np.abs(hid) @ np.abs(L["W2"]) + np.abs(L["b2"]) + np.abs(Xc[s])}
            xs = xn.astype(np.float32).astype(np.float64)  # the fp32 residual stream
            if Ln is not None:
                r["q"] = add(mm(h16(xs), Ln["Wqkv"]), Ln["bqkv"])
                r["Sq"] = (np.abs(h16(xs)) @ np.abs(Ln["Wqkv"]) + np.abs(Ln["bqkv"]))[:, :256]
                newqkv.append(h16(r["q"]))
                r["q"] = r["q"][:, :256]
            newX.append(xs)
            out.append(r)
        Xc, qkv = newX, newqkv
    return out


def sg_spread(A, B):
    """largest |A - B| / S over the valid rows of two sg_layers() results: (X, q) ratios"""
    rx = max([float((np.abs(a["X"] - b["X"]) / a["SX"]).max()) for a, b in zip(A, B) if a["n"]] + [0.0])
    rq = max([float((np.abs(a["q"] - b["q"]) / a["Sq"]).max()) for a, b in zip(A, B) if a["n"] and "q" in a] + [0.0])
    return rx, rq


# --------------------------------------------------------------------------------------------------------------
# Whole-network SuperPoint emulation (tools/sp_fp16_split.py)
# --------------------------------------------------------------------------------------------------------------
ENC = ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"]
HEADS = ["convPa", "convPb", "convDa", "convDb"]


def r16(t):
    return t.half().float()


def split16(t):
    """t = hi + lo, both fp16 (lo unscaled: it goes subnormal below |t| ~ 0.125, where its absolute error
    stays under fp16's subnormal spacing of 6e-8)"""
    hi = r16(t)
    return hi, r16(t - hi)


class Emu:
    """Per layer one of: "16" (fp16 operands, fp32 accumulation), "x3" (split fp16: activations and weights as
    hi + lo fp16 pairs, three MFMA products hi*hi + lo*hi + hi*lo accumulated in fp32), "x2a" / "x2w" (only the
    activations / only the weights split: two products), anything else fp32.  A layer's output is stored fp16
    only when the next layer is "16" (x2w too reads fp16 activations); otherwise it stays fp32 (x3 / x2a split
    it at load)."""
    def __init__(self, blob, k=400):
        import torch
        import rspl_loader
        self.k = k
        self.w = {k_: torch.from_numpy(np.asarray(v, np.float32))
                  for k_, v in rspl_loader.load().weights.read_blob(blob).items()}

    def conv(self, x, name, mode, out16, relu=True, pad=1):
        import torch.nn.functional as Fn
        w, b = self.w[name + ".weight"], self.w[name + ".bias"]
        if mode in ("16", "x2w"):
            x = r16(x)
        if mode == "16" and name == "conv1a":  # conv1_res_kernel: the bias rides the MFMA as the tenth tap (fp16)
            b = r16(b)
        if mode == "16":
            y = Fn.conv2d(x, r16(w), b, padding=pad)
        elif mode in ("x3", "x2a", "x2w"):
            xh, xl = split16(x)
            wh, wl = split16(w)
            y = Fn.conv2d(xh, wh, b, padding=pad)
            if mode in ("x3", "x2a"):
                y = y + Fn.conv2d(xl, wh, None, padding=pad)
            if mode in ("x3", "x2w"):
                y = y + Fn.conv2d(xh, wl, None, padding=pad)
        else:
            y = Fn.conv2d(x, w, b, padding=pad)
        if relu:
            y = Fn.relu(y)
        return r16(y) if out16 else y

    def forward(self, img_u8, half):
        """half: a set of fp16 layers, or a dict layer -> mode"""
        import torch
        import torch.nn.functional as Fn
        import oracle
        import post
        md = half if isinstance(half, dict) else {n: "16" for n in half}
        m = lambda n: md.get(n, "32")  # noqa: E731
        o16 = lambda n: m(n) in ("16", "x2w")  # noqa: E731  (the layer reads fp16 activations)
        x = torch.from_numpy(post.image_to_input(img_u8))[None, None]
        seq = ENC + ["convPa"]
        for i, name in enumerate(ENC):
            nxt = seq[i + 1]
            x = self.conv(x, name, m(name), m(name) != "32" and o16(nxt))
            if name in ("conv1b", "conv2b", "conv3b"):
                x = Fn.max_pool2d(x, 2, 2)
        pa = self.conv(x, "convPa", m("convPa"), m("convPa") != "32" and o16("convPb"))
        da = self.conv(x, "convDa", m("convDa"), m("convDa") != "32" and o16("convDb"))
        semi = self.conv(pa, "convPb", m("convPb"), False, relu=False, pad=0)
        desc = self.conv(da, "convDb", m("convDb"), False, relu=False, pad=0)
        s = torch.softmax(semi, 1)[:, :-1]
        h8, w8 = s.shape[2], s.shape[3]
        s = s.permute(0, 2, 3, 1).reshape(1, h8, w8, 8, 8).permute(0, 1, 3, 2, 4).reshape(h8 * 8, w8 * 8)
        desc = Fn.normalize(desc, p=2, dim=1)[0]
        scores = oracle.simple_nms(s.numpy().astype(np.float32))
        return post.sp_postprocess(scores, desc.numpy(), 0.004, 4, self.k)
