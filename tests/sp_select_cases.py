"""Built score maps for the SuperPoint tail (nms_kernel's candidate extraction, topk_kernel, the fp32 sample_kernel),
shared by test_sp_select_cpu.py (which proves from the reference alone that every case lands in the regime it is
meant for) and test_gpu_sp_select.py (which holds the device to the reference exactly).

The reference is the existing chain: oracle.simple_nms, then post.sp_postprocess (threshold in double, borders,
top-k with the flat-index tie-break, fp64 sample_descriptors).

Every map is built from a fixed seed; the arrays are read-only and the reference of a map is computed once.

topk_kernel's branch is a pure function of (n candidates, k, LDS_CAP); `regime` restates it:
  none        k = 0: count 0
  keep_all    k = -1, n <= LDS_CAP: all candidates in scan order (flat index ascending)
  overflow    k = -1 (or n <= k), n > LDS_CAP: count 0, the documented keep-all limit
  scan        n <= k: no sort by score, scan order
  whole_sort  k < n <= 2k and n <= LDS_CAP: bitonic sort of all n keys
  select      n > 2k or n > LDS_CAP: 8-pass radix select, compaction, sort of k keys

What simple_nms allows (and so what the maps can be): a pixel survives only if nothing within Chebyshev distance 4
is higher, so two surviving pixels closer than 5 are equal.  Distinct peaks therefore sit at least 5 apart (the
pitch-5 lattice), and a map whose whole interior survives is constant there.  The 136 x 136 map of case f, which
must give n = 16384 EXACTLY (n = 2k at k = 8192, the select at k = 8191, keep-all exactly full), is for that
reason a plain constant: one higher peak would remove the 80 pixels around it.  The 136 x 144 map carries the five
higher peaks (n = 17408 - 5 * 80, still beyond LDS_CAP).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

import oracle
import post

LDS_CAP = 16384          # kCandCap in rspl-slam_amd/csrc/sp.cpp: keys sorted whole in LDS, the keep-all and k limits
THRESHOLD = 0.004
PITCH = 5                # NMS radius 4: peaks 5 apart never suppress one another
FILL = -777.25           # prefill of every feature slot: rows at or beyond an image's count must keep it

T0 = np.float32(THRESHOLD)                     # widened to double it is above 0.004: kept
T_DN = np.nextafter(T0, np.float32(0))         # the next float down: dropped
T_UP = np.nextafter(T0, np.float32(1))         # the next float up: kept

# Largest difference, over all cases, between post.sample_descriptors as written (the norm summed sequentially) and
# the same function with the norm summed by np.sum (pairwise): the reference's own summation-order error, measured
# by test_sp_select_cpu.test_descriptor_tolerance_is_the_references_own_error (which asserts it is not exceeded).
NORM_ORDER_DIFF = 1.95e-16   # measured 1.943e-16
DESC_TOL = max(8 * NORM_ORDER_DIFF, 4 * np.finfo(np.float64).eps)   # floor: 4 double ulps at 1.0


def regime(n: int, k: int) -> str:
    if k == 0:
        return "none"
    if k == -1 or n <= k:
        if n > LDS_CAP:
            return "overflow"
        return "keep_all" if k == -1 else "scan"
    return "select" if (n > LDS_CAP or n > 2 * k) else "whole_sort"


def expected_count(n: int, k: int) -> int:
    r = regime(n, k)
    if r in ("none", "overflow"):
        return 0
    return n if r in ("keep_all", "scan") else k


@dataclass
class Case:
    name: str
    map_id: str                       # cases on the same maps share one NMS and one keep-all reference
    scores: np.ndarray                # [B, H, W] float32, pre-NMS
    desc: np.ndarray                  # [B, 256, H/8, W/8] float32, unit norm over the channels
    k: int
    border: int
    n: Tuple[int, ...]                # candidates per image the case is meant to have
    regime: Tuple[str, ...]           # topk_kernel's branch per image
    kept: List[Tuple[int, int, int]] = field(default_factory=list)      # (image, y, x) the reference must keep
    dropped: List[Tuple[int, int, int]] = field(default_factory=list)   # ... and must drop
    tie_cut: bool = False             # the k-th and (k+1)-th best scores are equal
    threshold: float = THRESHOLD

    @property
    def shape(self):
        return self.scores.shape


def lattice(H: int, W: int, origin: int = 2):
    ys, xs = np.meshgrid(np.arange(origin, H, PITCH), np.arange(origin, W, PITCH), indexing="ij")
    return ys.ravel(), xs.ravel()


def _noise(rng, H, W):
    """background in [0, 0.003]: whatever of it survives the NMS is below the threshold"""
    return rng.uniform(0.0, 0.003, (H, W)).astype(np.float32)


def _distinct(rng, n):
    return rng.permutation(np.linspace(0.1, 0.9, n)).astype(np.float32)


def _desc(seed, B, H, W):
    d = np.random.default_rng(seed).standard_normal((B, 256, H // 8, W // 8)).astype(np.float32)
    d /= np.sqrt((d.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    return d


def _ro(a):
    a.setflags(write=False)
    return a


HA, WA = 40, 56      # cases a, b, c, d, g, h: one partial 64 x 32 tile row, 8 x 11 = 88 lattice peaks
NA = 88


def _map_a(values, seed=101):
    m = _noise(np.random.default_rng(seed), HA, WA)
    ys, xs = lattice(HA, WA)
    assert ys.size == NA
    m[ys, xs] = values
    return m


def _peaks_map(H, W, peaks, seed):
    """noise plus distinct peaks at the (y, x) listed"""
    rng = np.random.default_rng(seed)
    m = _noise(rng, H, W)
    v = _distinct(rng, len(peaks))
    for (y, x), s in zip(peaks, v):
        m[y, x] = s
    return m


def _cheb_far(p, q, d=PITCH):
    return max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= d


# case e: 72 x 136 = 3 x 3 tiles of 64 x 32, the last column 8 wide and the last row 8 high
HE, WE = 72, 136
SEAM_X, SEAM_Y = (63, 64, 127, 128, 135), (31, 32, 63, 64, 71)
PLATEAU = (28, 40, 60, 72)     # rows 28..39, columns 60..71: across the seam corner (31|32, 63|64)
E_SPECIAL = (
    [(31, 127), (32, 135), (63, 63), (71, 64), (64, 128), (71, 135), (63, 135), (32, 20), (64, 40)],
    [(31, 63), (32, 128), (63, 64), (64, 135), (71, 127), (31, 135), (71, 63), (64, 20)],
)


def _map_e(b):
    rng = np.random.default_rng(500 + b)
    m = _noise(rng, HE, WE)
    special = E_SPECIAL[b]
    ys, xs = lattice(HE, WE)
    pts = [(int(y), int(x)) for y, x in zip(ys, xs)]
    if b == 0:   # the plateau's image: lattice rows above the plateau only, so that n stays below k = 400
        y0, y1, x0, x1 = PLATEAU
        pts = [p for p in pts if p[0] < y0 - PITCH]
        m[y0:y1, x0:x1] = np.float32(0.3)
        for p in special:   # nothing within reach of the plateau: all 144 of its pixels survive
            assert p[0] < y0 - 4 or p[0] >= y1 + 4 or p[1] < x0 - 4 or p[1] >= x1 + 4, p
    pts = [p for p in pts if all(_cheb_far(p, q) for q in special)]
    for i, p in enumerate(special):
        assert all(_cheb_far(p, q) for q in special[:i]), p
    allp = pts + special
    for (y, x), s in zip(allp, _distinct(rng, len(allp))):
        m[y, x] = s
    return m, len(allp) + (144 if b == 0 else 0)


F_PEAKS = [(20, 20), (20, 120), (70, 70), (110, 30), (115, 125)]   # far from each other and from the border


def _map_f(W, with_peaks):
    m = np.full((136, W), 0.01, np.float32)
    if with_peaks:
        for i, (y, x) in enumerate(F_PEAKS):
            m[y, x] = np.float32(0.5 + 0.05 * i)
    return m


D_KEPT = [(4, 4), (4, 22), (35, 12), (22, 4), (12, 51), (4, 51), (35, 4), (35, 51), (20, 30)]
D_DROPPED = [(3, 12), (36, 22), (12, 3), (22, 52)]
G_THREE = [(10, 10), (20, 30), (30, 45)]


@functools.lru_cache(maxsize=None)
def cases() -> Dict[str, Case]:
    out: Dict[str, Case] = {}

    def add(c: Case):
        assert c.name not in out
        _ro(c.scores), _ro(c.desc)
        out[c.name] = c

    rng = np.random.default_rng(7)
    desc_a = _desc(11, 1, HA, WA)
    ys, xs = lattice(HA, WA)

    # a. branch boundaries on the 88-peak lattice, distinct scores, border 0
    map_a = _map_a(_distinct(rng, NA))[None]
    for k, r in ((-1, "keep_all"), (100, "scan"), (88, "scan"), (87, "whole_sort"), (44, "whole_sort"),
                 (43, "select"), (1, "select")):
        add(Case(f"a_k{k}", "a", map_a, desc_a, k, 0, (NA,), (r,)))
    # the max_keypoints contract: 0 yields no keypoints
    add(Case("a_k0", "a", map_a, desc_a, 0, 0, (NA,), ("none",)))

    # b. ties and low bytes: both cuts (k = 43: select, k = 60: whole sort) on the same lattice
    three = np.repeat(np.float32([0.8, 0.5, 0.2]), [30, 25, 33])      # cuts 43 and 60 fall inside groups 2 and 3
    map_bi = _map_a(rng.permutation(three))[None]
    low = (np.uint32(0x3F000000) + rng.permutation(NA).astype(np.uint32)).view(np.float32)   # differ in the last byte
    map_bii = _map_a(low)[None]
    map_biii = _map_a(np.full(NA, 0.5, np.float32))[None]
    for k, r in ((43, "select"), (60, "whole_sort")):
        add(Case(f"b1_three_values_k{k}", "b1", map_bi, desc_a, k, 0, (NA,), (r,), tie_cut=True))
        add(Case(f"b2_low_byte_k{k}", "b2", map_bii, desc_a, k, 0, (NA,), (r,)))
        add(Case(f"b3_all_equal_k{k}", "b3", map_biii, desc_a, k, 0, (NA,), (r,), tie_cut=True))

    # c. threshold edge: float32(0.004) and its two neighbours among ordinary peaks
    vals = _distinct(rng, NA)
    vals[0:3], vals[3:6], vals[6:9] = T0, T_DN, T_UP
    order = rng.permutation(NA)
    vc = np.empty(NA, np.float32)
    vc[order] = vals
    at = lambda sl: [(0, int(ys[i]), int(xs[i])) for i in order[sl]]
    add(Case("c_threshold_edge", "c", _map_a(vc)[None], desc_a, 100, 0, (NA - 3,), ("scan",),
             kept=at(slice(0, 3)) + at(slice(6, 9)), dropped=at(slice(3, 6))))

    # d. borders: border 4, peaks on rows and columns 3, 4, H-5, H-4 (W-5, W-4): only 4 and H-5 (W-5) survive
    map_d = _peaks_map(HA, WA, D_KEPT + D_DROPPED, 202)[None]
    add(Case("d_borders", "d", map_d, desc_a, 100, 4, (len(D_KEPT),), ("scan",),
             kept=[(0, y, x) for y, x in D_KEPT], dropped=[(0, y, x) for y, x in D_DROPPED]))

    # e. tile seams and partial tiles, B = 2 with different maps
    (e0, n0), (e1, n1) = _map_e(0), _map_e(1)
    map_e, desc_e = np.stack([e0, e1]), _desc(12, 2, HE, WE)
    y0, y1, x0, x1 = PLATEAU
    seam = [(b, y, x) for b in range(2) for y, x in E_SPECIAL[b]] + \
           [(0, y, x) for y in range(y0, y1) for x in range(x0, x1)]
    add(Case("e_seams_k400", "e", map_e, desc_e, 400, 0, (n0, n1), ("scan", "scan"), kept=seam))
    add(Case("e_seams_k50", "e", map_e, desc_e, 50, 0, (n0, n1), ("select", "select")))

    # f. around the LDS sort size, border 4
    map_f0, map_f1 = _map_f(136, False)[None], _map_f(144, True)[None]
    desc_f0, desc_f1 = _desc(13, 1, 136, 136), _desc(14, 1, 136, 144)
    for k, r in ((-1, "keep_all"), (8192, "whole_sort"), (8191, "select")):
        add(Case(f"f_136x136_k{k}", "f0", map_f0, desc_f0, k, 4, (LDS_CAP,), (r,), tie_cut=k > 0))
    n_f1 = 128 * 136 - 80 * len(F_PEAKS)
    for k, r in ((400, "select"), (LDS_CAP, "select"), (-1, "overflow")):
        add(Case(f"f_136x144_k{k}", "f1", map_f1, desc_f1, k, 4, (n_f1,), (r,), tie_cut=k > 0,
                 kept=[(0, y, x) for y, x in F_PEAKS]))

    # g. mixed batch, k = 43: nothing above the threshold | the 88-peak lattice (select) | three peaks (n < k)
    rg = np.random.default_rng(303)
    map_g = np.stack([_noise(rg, HA, WA), map_a[0], _peaks_map(HA, WA, G_THREE, 304)])
    add(Case("g_mixed_batch", "g", map_g, _desc(15, 3, HA, WA), 43, 0, (0, NA, 3), ("scan", "select", "scan")))

    # h. clamped and extrapolating taps: the case-a map with three lattice peaks moved to the left and top edges
    moved = {(2, 2): (0, 0), (12, 2): (12, 0), (2, 12): (0, 12)}
    mh = _noise(np.random.default_rng(101), HA, WA)
    va = map_a[0][ys, xs]
    for i in range(NA):
        y, x = moved.get((int(ys[i]), int(xs[i])), (int(ys[i]), int(xs[i])))
        mh[y, x] = va[i]
    add(Case("h_edge_taps", "h", mh[None], desc_a, -1, 0, (NA,), ("keep_all",),
             kept=[(0, y, x) for y, x in moved.values()] + [(0, 2, 7), (0, 7, 2)],
             dropped=[(0, y, x) for y, x in moved]))
    return out


_nms_cache: dict = {}
_all_cache: dict = {}


def nms_maps(c: Case) -> np.ndarray:
    if c.map_id not in _nms_cache:
        _nms_cache[c.map_id] = _ro(np.stack([oracle.simple_nms(s) for s in c.scores]))
    return _nms_cache[c.map_id]


def keep_all_reference(c: Case) -> List[np.ndarray]:
    """per image, every candidate in scan order (k = -1): its column count is the image's n"""
    key = (c.map_id, c.border, c.threshold)
    if key not in _all_cache:
        with np.errstate(divide="ignore", invalid="ignore"):   # 0/0 at x = W-1 or y = H-1 (the seam case)
            _all_cache[key] = [_ro(post.sp_postprocess(m, d, c.threshold, c.border, -1))
                               for m, d in zip(nms_maps(c), c.desc)]
    return _all_cache[key]


def reference(c: Case) -> List[np.ndarray]:
    """per image the reference's features [259, count] for the case's own k; count 0 in the regimes `none` and
    `overflow` (the latter the device's documented keep-all limit, not the reference's behaviour)"""
    out = []
    for b, A in enumerate(keep_all_reference(c)):
        n = A.shape[1]
        r = regime(n, c.k)
        if r in ("none", "overflow"):
            out.append(A[:, :0])
        elif r in ("keep_all", "scan"):
            out.append(A)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                out.append(post.sp_postprocess(nms_maps(c)[b], c.desc[b], c.threshold, c.border, c.k))
    return out
