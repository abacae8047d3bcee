"""Restatement of the reference's rectification stage in numpy: the maps Camera::Camera builds
(src/camera.cc:9-63: cv::initUndistortRectifyMap, or its cv::fisheye twin for distortion_type 1) and
Camera::UndistortImage (src/camera.cc:87-91: cv::remap with float maps, INTER_LINEAR, u8, BORDER_CONSTANT 0).

OpenCV is not available to these tests, so this restates its published arithmetic and parity is unpinned at
OpenCV itself.  What is known to differ: the 3x3 inverse here is Gauss-Jordan with partial pivoting (OpenCV:
LU for the pinhole model, SVD for the fisheye one), x = _x / _w is a division (OpenCV multiplies by 1 / _w)
and _x is formed directly per column (OpenCV accumulates it along the row).  The remap is integer arithmetic
after one rounding and has no such freedom.

Every double operation below is a separate IEEE operation in the order the native code (csrc/rect.cpp,
contraction off) performs it, so the maps are compared bitwise.  atan goes through math.atan, the C library's,
as the native code's does; numpy's own arctan may take a SIMD path with other last bits.
"""
import math

import numpy as np


def inv3(A):
    """Gauss-Jordan with partial pivoting on Python floats (the order of oracle/ba.c's small_inv)."""
    M = [[float(A[i][j]) for j in range(3)] + [1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for c in range(3):
        p = c
        for r in range(c + 1, 3):
            if abs(M[r][c]) > abs(M[p][c]):
                p = r
        if M[p][c] == 0:
            raise ValueError("singular")
        if p != c:
            M[c], M[p] = M[p], M[c]
        iv = 1.0 / M[c][c]
        M[c] = [v * iv for v in M[c]]
        for r in range(3):
            if r != c:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [[M[i][3 + j] for j in range(3)] for i in range(3)]


def _rays(R, P, H, W):
    R = np.asarray(R, np.float64).reshape(3, 3).tolist()
    P = np.asarray(P, np.float64).reshape(3, 4).tolist()
    PR = [[P[i][0] * R[0][j] + P[i][1] * R[1][j] + P[i][2] * R[2][j] for j in range(3)] for i in range(3)]
    iR = inv3(PR)
    i = np.arange(H, dtype=np.float64)[:, None]
    j = np.arange(W, dtype=np.float64)[None, :]
    return [i * iR[k][1] + iR[k][2] + j * iR[k][0] for k in range(3)]


def build_maps(K, D, R, P, distortion_type, H, W, cast=True):
    """(map_x, map_y) float32 [H, W]; cast=False returns the doubles before the cast."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    D = [float(v) for v in np.asarray(D, np.float64).ravel()] + [0.0] * 8
    _x, _y, _w = _rays(R, P, H, W)
    with np.errstate(all="ignore"):
        if distortion_type == 0:
            k1, k2, p1, p2, k3, k4, k5, k6 = D[:8]
            x, y = _x / _w, _y / _w
            x2, y2 = x * x, y * y
            r2 = x2 + y2
            _2xy = 2 * x * y
            kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
            xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
            yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
            u, v = fx * xd + cx, fy * yd + cy
        elif distortion_type == 1:
            k1, k2, k3, k4 = D[:4]
            behind = _w <= 0
            x = np.where(behind, np.where(_x > 0, -np.inf, np.inf), _x / _w)
            y = np.where(behind, np.where(_y > 0, -np.inf, np.inf), _y / _w)
            rr = x * x + y * y
            r = np.array([math.sqrt(t) for t in rr.ravel()]).reshape(rr.shape)
            th = np.array([math.atan(t) for t in r.ravel()]).reshape(r.shape)
            t2 = th * th
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            thd = th * (1 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8)
            scale = np.where(r == 0, 1.0, thd / r)
            u, v = fx * x * scale + cx, fy * y * scale + cy
        else:
            raise ValueError("distortion_type")
        if not cast:
            return u, v
        return u.astype(np.float32), v.astype(np.float32)


def _cv_round32(m):
    """cvRound(m * 32) for float32 m as int64 and a mask of the finite ones (NaN rounds to INT_MIN and
    +-inf / huge values saturate in OpenCV: all of them end outside any image)."""
    with np.errstate(all="ignore"):
        v = np.asarray(m, np.float32) * np.float32(32)
        ok = np.isfinite(v) & (np.abs(v) < 2.0 ** 40)
        s = np.rint(np.where(ok, v, np.float32(0))).astype(np.int64)  # half to even
    return s, ok


def fixed(map_x, map_y, H, W):
    """The table the kernel reads: (ix, iy) int16 and frac = fx | fy << 5 uint16, with the coordinates whose
    taps all lie outside clamped to -2 (left / above, NaN, -inf) or to the extent, fraction 0."""
    def axis(m, N):
        s, ok = _cv_round32(m)
        with np.errstate(all="ignore"):
            v = np.asarray(m, np.float32) * np.float32(32)
            low = ~(v >= np.float32(-64))
            high = v >= np.float32(N * 32)
        s = np.where(ok, s, 0)
        i, f = s >> 5, s & 31
        f = np.where(i == -2, 0, f)
        i = np.where(low, -2, np.where(high, N, i))
        f = np.where(low | high, 0, f)
        return i, f
    ix, fx = axis(map_x, W)
    iy, fy = axis(map_y, H)
    return ix.astype(np.int16), iy.astype(np.int16), (fx | fy << 5).astype(np.uint16)


def classes(map_x, map_y, H, W):
    """Per pixel 0: all four taps outside the source, 1: some outside, 2: all inside."""
    sx, okx = _cv_round32(map_x)
    sy, oky = _cv_round32(map_y)
    ix, iy = sx >> 5, sy >> 5
    ok = okx & oky
    inside = ok & (ix >= 0) & (ix + 1 < W) & (iy >= 0) & (iy + 1 < H)
    outside = ~ok | (ix >= W) | (ix + 1 < 0) | (iy >= H) | (iy + 1 < 0)
    return np.where(outside, 0, np.where(inside, 2, 1))


def remap(src, map_x, map_y):
    """cv::remap(src, map_x, map_y, INTER_LINEAR) on a u8 image [H, W] -> u8 of the maps' shape."""
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    sx, okx = _cv_round32(map_x)
    sy, oky = _cv_round32(map_y)
    ok = okx & oky
    # OpenCV saturates the integer parts to int16: far outside either way
    ix = np.clip(sx >> 5, -32768, 32767)
    iy = np.clip(sy >> 5, -32768, 32767)
    fx, fy = sx & 31, sy & 31

    def tap(y, x):
        inside = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(inside, src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0).astype(np.int64)

    w = (32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy)
    acc = w[0] * tap(iy, ix) + w[1] * tap(iy, ix + 1) + w[2] * tap(iy + 1, ix) + w[3] * tap(iy + 1, ix + 1)
    return ((acc + 16384) >> 15).astype(np.uint8)
