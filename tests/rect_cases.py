"""Cases shared by test_rect_cpu.py and test_gpu_rect.py: the golden calibrations, synthetic calibrations whose
rectified view crosses the source's border, and crafted map coordinates at every rounding and border seam."""
import pathlib

import numpy as np

import rect_ref as RR

CALIB = pathlib.Path(__file__).resolve().parent / "golden" / "calib"
GOLDEN = ("euroc", "uma_bumblebee")

# EuRoC's left camera (tests/golden/calib/euroc.yaml)
EUROC_R = [0.999966347530033, -0.001422739138722922, 0.008079580483432283,
           0.001365741834644127, 0.9999741760894847, 0.007055629199258132,
           -0.008089410156878961, -0.007044357138835809, 0.9999424675829176]
EUROC_D = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]
FISHEYE_D = [-0.01, 0.02, -0.005, 0.001]

# (W, H, f) and the pixels (wholly outside, partly outside, inside) per model, counted from the restatement
# when the cases were chosen
SYNTHETIC = {(96, 64, 60): {0: (1654, 307, 4183), 1: (1427, 364, 4353)},
             (200, 136, 120): {0: (6993, 645, 19562), 1: (5595, 751, 20854)},
             (72, 40, 45): {0: (818, 207, 1855), 1: (752, 209, 1919)}}


def synthetic(W, H, f, model):
    """K, D, R, P of a camera whose new view (focal 2f/3, centred) sees past the source on every side."""
    K = [f, 0, (W - 1) / 2 + 0.7, 0, 0.997 * f, (H - 1) / 2 - 0.4, 0, 0, 1]
    fn = 2 * f / 3
    P = [fn, 0, (W - 1) / 2, 0, 0, fn, (H - 1) / 2, 0, 0, 0, 1, 0]
    return K, (EUROC_D if model == 0 else FISHEYE_D), EUROC_R, P


def synthetic_pair(W, H, f, model):
    """left as synthetic(); right with a slightly different K so the two cameras' maps differ"""
    K, D, R, P = synthetic(W, H, f, model)
    Kr = list(K)
    Kr[2] += 1.3
    Kr[5] -= 0.9
    return (K, D, R, P), (Kr, D, R, P)


def crafted_axis(N):
    """Coordinates on an axis of extent N: exact ties (k + 0.5)/32 for even and odd k, the signed zero and
    the first negatives, the last column and what follows it, and the non-finite and huge ones."""
    return np.array([6.5 / 32, 7.5 / 32, 10 + 12.5 / 32, 10 + 13.5 / 32, -0.5 / 32, -1.5 / 32,
                     -0.0, -1 / 64, -1 - 1 / 32, -1.0, -1 + 1 / 32, -2.0,
                     N - 1, N - 1 + 1 / 32, N - 1 / 64, N, N + 0.5,
                     1e9, -1e9, np.inf, -np.inf, np.nan,
                     3.25, 17.71875, N / 2 + 0.40625, 0.0, 1.0], np.float32)


# what cv::remap's rounding makes of crafted_axis(N)[:22], written out by hand: (ix, fx), clamped as the table is
def crafted_expected(N):
    return [(0, 6), (0, 8), (10, 12), (10, 14), (0, 0), (-1, 30),
            (0, 0), (0, 0), (-2, 0), (-1, 0), (-1, 1), (-2, 0),
            (N - 1, 0), (N - 1, 1), (N, 0), (N, 0), (N, 0),
            (N, 0), (-2, 0), (N, 0), (-2, 0), (-2, 0)]


def crafted_maps(H, W):
    """Every pair of crafted x and y coordinates, tiled over an H x W map."""
    xs, ys = crafted_axis(W), crafted_axis(H)
    k = np.arange(H * W)
    assert H * W >= len(xs) * len(ys)
    return xs[k % len(xs)].reshape(H, W), ys[(k // len(xs)) % len(ys)].reshape(H, W)


def ref_maps(cam, model, H, W):
    K, D, R, P = cam
    return RR.build_maps(K, D, R, P, model, H, W)
