"""Test helper: the device detector's decomposition restated in Python over oracle/fld_ref.py.

Chains interact only through the pixels they consume and never leave their 8-connected component, so walking
each component on its own (its seeds in raster order) and sorting the segments by (seed raster index, index
within the chain) must give what the sequential detector gives.  ``detect_parallel`` does exactly that, taking
the components in reverse order; ``walk_sequential`` is the plain raster walk the chain kernels are checked
against.  Also the builders of the hysteresis and chain test maps.
"""
from __future__ import annotations

import numpy as np

import fld_ref as FR


def edges_of(half: np.ndarray, th1: float = 200.0, th2: float = 250.0) -> np.ndarray:
    """Canny edges of the half image after the corner zeroing (what the chain walk starts from)"""
    e = FR.canny(half, th1, th2).copy()
    zero_corners(e)
    return e


def zero_corners(e: np.ndarray) -> np.ndarray:
    H, W = e.shape
    e[0:6, 0:6] = 0
    e[max(H - 5, 0):H, max(W - 5, 0):W] = 0
    return e


def components(e: np.ndarray):
    """8-connected components of the non-zero pixels: lists of (r, c) in raster order, by first pixel"""
    H, W = e.shape
    lab = -np.ones((H, W), np.int64)
    comps = []
    for r in range(H):
        for c in range(W):
            if e[r, c] == 0 or lab[r, c] >= 0:
                continue
            k = len(comps)
            lab[r, c] = k
            stack, px = [(r, c)], []
            while stack:
                y, x = stack.pop()
                px.append((y, x))
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < H and 0 <= xx < W and e[yy, xx] and lab[yy, xx] < 0:
                            lab[yy, xx] = k
                            stack.append((yy, xx))
            comps.append(sorted(px))
    return comps


def _walk(e: np.ndarray, pixels):
    """chains seeded at `pixels` (raster order) on the shared, consumed edge map: [(seed index, [(x, y)])]"""
    W = e.shape[1]
    out = []
    for r, c in pixels:
        if e[r, c] == 0:
            continue
        pt = (c, r)
        pts = [pt]
        e[r, c] = 0
        direction, step = 0, 0
        while True:
            nxt = FR._chain_step(e, pt, direction, step)
            if nxt is None:
                break
            pt, direction = nxt
            pts.append(pt)
            step += 1
            e[pt[1], pt[0]] = 0
        out.append((r * W + c, pts))
    return out


def walk_sequential(edges: np.ndarray):
    e = edges.copy()
    H, W = e.shape
    return _walk(e, [(r, c) for r in range(H) for c in range(W)])


def walk_parallel(edges: np.ndarray, reverse: bool = True):
    """component by component (in reverse order), chains sorted by seed"""
    e = edges.copy()
    comps = components(e)
    chains = []
    for comp in (reversed(comps) if reverse else comps):
        chains += _walk(e, comp)
    return sorted(chains, key=lambda ch: ch[0])


def segments_of(half: np.ndarray, chains, length_threshold: int = 10, distance_threshold: float = 1.414213562):
    """fld_detect's tail per chain: [(seed, k, oriented segment)] in the order of `chains`"""
    H, W = half.shape
    out = []
    for seed, pts in chains:
        if len(pts) < length_threshold + 1:
            continue
        for k, seg in enumerate(FR.extract_segments(pts, length_threshold, distance_threshold)):
            x1, y1, x2, y2 = (float(np.float32(v)) for v in seg)
            ddx, ddy = np.float32(x1) - np.float32(x2), np.float32(y1) - np.float32(y2)
            if np.sqrt(np.float32(ddx * ddx + ddy * ddy)) < length_threshold:
                continue
            if ((x1 <= 5.0 and x2 <= 5.0) or (y1 <= 5.0 and y2 <= 5.0) or
                    (x1 >= W - 5.0 and x2 >= W - 5.0) or (y1 >= H - 5.0 and y2 >= H - 5.0)):
                continue
            out.append((seed, k, FR._orient(half, (x1, y1, x2, y2))))
    return out


def detect_parallel(half: np.ndarray, th1: float = 200.0, th2: float = 250.0) -> np.ndarray:
    chains = walk_parallel(edges_of(half, th1, th2))
    chains.reverse()  # the fit sees the chains in no particular order
    segs = sorted(segments_of(half, chains), key=lambda s: (s[0], s[1]))
    return np.array([s[2] for s in segs], np.float32).reshape(-1, 4)


# --- test maps -------------------------------------------------------------------------------------------
def spiral_classes(n: int = 64):
    """a one-pixel-wide candidate spiral from (0, 0) inwards, one blank pixel between its turns, as a class map
    (0 candidate, 1 none); returns (cls, path [(r, c)])"""
    cls = np.ones((n, n), np.uint8)
    on = np.zeros((n, n), bool)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    r = c = d = 0
    on[0, 0] = True
    path = [(0, 0)]

    def free(y, x):
        return not (0 <= y < n and 0 <= x < n) or not on[y, x]

    def ok(dr, dc):
        y, x = r + dr, c + dc
        return 0 <= y < n and 0 <= x < n and not on[y, x] and free(y + dr, x + dc)

    while True:
        if not ok(*dirs[d]):
            d = (d + 1) % 4
            if not ok(*dirs[d]):
                break
        r, c = r + dirs[d][0], c + dirs[d][1]
        on[r, c] = True
        path.append((r, c))
    cls[on] = 0
    return cls, path


def dots_and_bars(h: int = 64, w: int = 160, n: int = 200, seed: int = 11) -> np.ndarray:
    """n isolated dots and short bars on a 4 x 4 grid of cells (no two touch)"""
    rng = np.random.default_rng(seed)
    e = np.zeros((h, w), np.uint8)
    cells = [(r, c) for r in range(0, h - 3, 4) for c in range(0, w - 3, 4)]
    assert len(cells) >= n
    for i in rng.permutation(len(cells))[:n]:
        r, c = cells[i]
        kind = rng.integers(0, 3)
        e[r, c] = 255
        if kind == 1:
            e[r, c + 1] = e[r, c + 2] = 255
        elif kind == 2:
            e[r + 1, c] = e[r + 2, c] = 255
    return e
