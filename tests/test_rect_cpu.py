"""CPU-side checks of stereo rectification (rspl_rect_*, rspl_slam_amd.Camera): the boundary is declared and
bound, the native map builders equal the restatement (tests/rect_ref.py) bitwise, the restatement's pinhole
maps agree with an independently written formula, the fixed-point table equals the restatement and a
hand-written list at every rounding and border seam, Camera reads the reference's calibration files, and bad
configurations are refused before a device is touched.  OpenCV is not available: parity is unpinned there."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import rect_ref as RR
from rect_cases import CALIB, GOLDEN, SYNTHETIC, crafted_axis, crafted_expected, crafted_maps, synthetic

ROOT = pathlib.Path(__file__).resolve().parents[1]
FUNCS = ("rspl_rect_build_maps", "rspl_rect_debug_fixed", "rspl_rect_debug_sizeof", "rspl_rect_debug_copy", "rspl_rect_create",
         "rspl_rect_destroy", "rspl_rect_get_maps", "rspl_rect_set_maps", "rspl_rect_enqueue_device", "rspl_rect_pair")


def _pkg():
    import rspl_loader
    return rspl_loader.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _native_maps(cam, model, H, W):
    from rspl_slam_amd import camera
    K, D, R, P = cam
    return camera.build_maps(camera.rect_camera(K, D, R, P, model), model, H, W)


def _assert_bitwise(cam, model, H, W):
    mx, my = _native_maps(cam, model, H, W)
    rx, ry = RR.build_maps(*cam, model, H, W)
    assert np.array_equal(_bits(mx), _bits(rx)) and np.array_equal(_bits(my), _bits(ry))
    return rx, ry


def _golden_cam(name, side=0):
    c = _pkg().Camera(CALIB / f"{name}.yaml")
    rc = c.cams[side]
    return c, (list(rc.K), list(rc.D), list(rc.R), list(rc.P))


def test_header_declares_rect_api():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    for n in FUNCS:
        assert n in names
    for s in ("rspl_rect_camera", "rspl_rect_config"):
        assert re.search(r"}\s*%s;" % s, hdr), s
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct changed


def test_capi_binds_rect_api_and_struct_layouts():
    from rspl_slam_amd import capi
    lib = capi.load()
    for n in FUNCS:
        assert n in capi.EXPORTS and hasattr(lib, n)
    assert len(lib.rspl_rect_enqueue_device.argtypes) == 10 and len(lib.rspl_rect_pair.argtypes) == 7
    assert [f[0] for f in capi.RectConfig._fields_] == ["height", "width", "distortion_type", "cam", "max_batch",
                                                        "device"]
    assert lib.rspl_rect_debug_sizeof(0) == C.sizeof(capi.RectCamera) == 38 * 8
    assert lib.rspl_rect_debug_sizeof(1) == C.sizeof(capi.RectConfig)
    assert lib.rspl_rect_debug_sizeof(2) == -1


@pytest.mark.parametrize("name", GOLDEN)
@pytest.mark.parametrize("side", [0, 1])
def test_build_maps_bitwise_on_golden_calibrations(name, side):
    """Both models, small and at the calibration's own size.  The fisheye restatement calls math.atan, the
    same C library the native code calls, and bitwise equality is reached."""
    c, cam = _golden_cam(name, side)
    _assert_bitwise(cam, c.distortion_type, 64, 96)
    rx, ry = _assert_bitwise(cam, c.distortion_type, int(c.ImageHeight()), int(c.ImageWidth()))
    mx, my = c.maps(side)  # Camera's own accessor goes the same way
    assert np.array_equal(_bits(mx), _bits(rx)) and np.array_equal(_bits(my), _bits(ry))


@pytest.mark.parametrize("whf", sorted(SYNTHETIC))
@pytest.mark.parametrize("model", [0, 1])
def test_build_maps_bitwise_on_synthetic_calibrations(whf, model):
    W, H, f = whf
    rx, ry = _assert_bitwise(synthetic(W, H, f, model), model, H, W)
    # the cases do cross the border, as counted when they were chosen
    assert tuple(np.bincount(RR.classes(rx, ry, H, W).ravel(), minlength=3)) == SYNTHETIC[whf][model]


def test_build_maps_with_rational_coefficients():
    """k4..k6 take part (the reference's files carry five coefficients, so nothing else reaches them)"""
    K, D, R, P = synthetic(96, 64, 60, 0)
    cam = (K, D[:5] + [0.01, -0.002, 0.0005], R, P)
    rx, _ = _assert_bitwise(cam, 0, 64, 96)
    assert not np.array_equal(rx, RR.build_maps(K, D, R, P, 0, 64, 96)[0])


def test_euroc_maps_match_an_independent_formula():
    """Guards against a mistake shared by the restatement and the native code: the same maps from numpy's own
    inverse, a multiplication by 1 / w as OpenCV does, and the expanded polynomial, to 1e-9 before the cast;
    after it the native floats are within one float spacing at these magnitudes (< 1024: 2^-14)."""
    c, (K, D, R, P) = _golden_cam("euroc")
    H, W = 480, 752
    K, R, P = np.reshape(K, (3, 3)), np.reshape(R, (3, 3)), np.reshape(P, (3, 4))
    k1, k2, p1, p2, k3 = D[:5]
    iR = np.linalg.inv(P[:, :3] @ R)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([jj, ii, np.ones_like(jj)], -1) @ iR.T
    x, y = ray[..., 0] * (1 / ray[..., 2]), ray[..., 1] * (1 / ray[..., 2])
    r2 = x ** 2 + y ** 2
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    u = K[0, 0] * (x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2)) + K[0, 2]
    v = K[1, 1] * (y * radial + p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y) + K[1, 2]
    ru, rv = RR.build_maps(K, D, R, P, 0, H, W, cast=False)
    assert np.abs(ru - u).max() < 1e-9 and np.abs(rv - v).max() < 1e-9
    mx, my = c.maps(0)
    assert np.abs(mx - u).max() <= 2.0 ** -14 and np.abs(my - v).max() <= 2.0 ** -14
    assert np.all(RR.classes(mx, my, H, W) == 2)  # on EuRoC no pixel leaves the source


def _native_fixed(mx, my, H, W):
    from rspl_slam_amd import capi
    mx, my = np.ascontiguousarray(mx, np.float32).ravel(), np.ascontiguousarray(my, np.float32).ravel()
    ix, iy, fr = np.empty(mx.size, np.int16), np.empty(mx.size, np.int16), np.empty(mx.size, np.uint16)
    rc = capi.load().rspl_rect_debug_fixed(mx.ctypes.data, my.ctypes.data, mx.size, H, W, ix.ctypes.data, iy.ctypes.data,
                                           fr.ctypes.data)
    assert rc == 0
    return ix, iy, fr


@pytest.mark.parametrize("hw", [(40, 72), (480, 752), (2044, 2044), (1, 1)])
def test_fixed_point_table_on_crafted_coordinates(hw):
    H, W = hw
    xs, ys = crafted_axis(W), crafted_axis(H)
    n = len(xs)
    ix, iy, fr = _native_fixed(xs, ys, H, W)
    rix, riy, rfr = RR.fixed(xs, ys, H, W)
    assert np.array_equal(ix, rix) and np.array_equal(iy, riy) and np.array_equal(fr, rfr)
    if min(H, W) > 20:  # the hand-written list assumes the interior entries are interior
        ex, ey = crafted_expected(W), crafted_expected(H)
        assert [(int(a), int(b) & 31) for a, b in zip(ix, fr)][:len(ex)] == ex
        assert [(int(a), int(b) >> 5) for a, b in zip(iy, fr)][:len(ey)] == ey
    # every pairing of an x with a y
    if H * W >= n * n:
        mx, my = crafted_maps(H, W) if H * W < 1 << 20 else (np.repeat(xs, n), np.tile(ys, n))
        got, ref = _native_fixed(mx, my, H, W), RR.fixed(mx, my, H, W)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r.ravel())


def test_fixed_point_table_on_real_maps():
    for whf in sorted(SYNTHETIC):
        W, H, f = whf
        for model in (0, 1):
            rx, ry = RR.build_maps(*synthetic(W, H, f, model), model, H, W)
            for g, r in zip(_native_fixed(rx, ry, H, W), RR.fixed(rx, ry, H, W)):
                assert np.array_equal(g, r.ravel())


def test_remap_restatement_by_hand():
    src = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)
    jj, ii = np.meshgrid(np.arange(3, dtype=np.float32), np.arange(2, dtype=np.float32))
    assert np.array_equal(RR.remap(src, jj, ii), src)
    # half a pixel right: the mean of two neighbours, the last column against the border's 0
    assert RR.remap(src, jj + 0.5, ii).tolist() == [[15, 25, 15], [45, 55, 30]]
    # a quarter down and right of (0, 0): (9*10 + 3*20 + 3*40 + 50) / 16 = 20
    assert RR.remap(src, np.float32([[0.25]]), np.float32([[0.25]])).tolist() == [[20]]
    # one pixel left of the image still sees column 0 at weight fx; further left, and non-finite, nothing
    out = RR.remap(src, np.float32([[-0.5, -1.0, -1 - 1 / 32, np.nan, np.inf, 1e9, 3.0]]), np.zeros((1, 7), np.float32))
    assert out.tolist() == [[5, 0, 0, 0, 0, 0, 0]]


def test_camera_reads_the_reference_calibrations():
    pkg = _pkg()
    c = pkg.Camera(CALIB / "euroc.yaml")
    assert (c.ImageHeight(), c.ImageWidth(), c.distortion_type) == (480.0, 752.0, 0)
    assert c.BF() == 47.90639384423901 and c.DepthLowerThr() == 0.1 and c.DepthUpperThr() == 10.0
    assert c.MaxXDiff() == c.BF() / 0.1 and c.MinXDiff() == c.BF() / 10.0 and c.MaxYDiff() == 2.0
    assert (c.Fx(), c.Fy(), c.Cx(), c.Cy()) == (435.2046959714599, 435.2046959714599, 367.4517211914062,
                                                252.2008514404297)
    assert np.array_equal(c.GetCamerMatrix(), [[c.Fx(), 0, c.Cx()], [0, c.Fy(), c.Cy()], [0, 0, 1]])
    assert c.GetDistCoeffs().shape == (5, 1) and not c.GetDistCoeffs().any()
    assert list(c.cams[1].K) == [457.587, 0.0, 379.999, 0.0, 456.134, 255.238, 0.0, 0.0, 1.0]
    assert list(c.cams[1].D) == [-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0, 0.0, 0.0, 0.0]
    assert c.cams[1].P[3] == -47.90639384423901 and c.cams[0].R[0] == 0.999966347530033
    np.testing.assert_allclose(c.BackProjectMono([c.Cx() + c.Fx(), c.Cy() - 2 * c.Fy()]), [1, -2, 1], rtol=1e-15)
    np.testing.assert_allclose(c.BackProjectStereo([c.Cx() + c.Fx(), c.Cy(), c.Cx() + c.Fx() - c.BF() / 4]),
                               [4, 0, 4], rtol=1e-13, atol=1e-13)
    u = pkg.Camera(CALIB / "uma_bumblebee.yaml")
    assert (u.ImageHeight(), u.ImageWidth(), u.distortion_type) == (768.0, 1024.0, 1)
    assert u.MaxXDiff() == 52.1485318013 / 0.1 and u.MaxYDiff() == 3.0 and u.DepthUpperThr() == 10.0
    assert list(u.cams[0].D) == [-0.06871322616238257, 0.02451994273357104, -0.02288817712592593,
                                 0.005970525621928401, 0.0, 0.0, 0.0, 0.0]


def test_camera_refuses_incomplete_or_unmodelled_calibrations(tmp_path):
    pkg = _pkg()
    text = (CALIB / "euroc.yaml").read_text()
    cut = re.sub(r"RIGHT\.R:.*?(?=RIGHT\.P)", "", text, flags=re.S)
    assert "RIGHT.R" not in cut and "RIGHT.P" in cut
    (tmp_path / "cut.yaml").write_text(cut)
    with pytest.raises(ValueError, match="RIGHT.R"):
        pkg.Camera(tmp_path / "cut.yaml")
    (tmp_path / "nosize.yaml").write_text(text.replace("image_height: 480", "image_height: 0"))
    with pytest.raises(ValueError):
        pkg.Camera(tmp_path / "nosize.yaml")
    # twelve coefficients with a non-zero thin-prism term are not modelled; with zeros there they load
    d12 = "cols: 12\n   dt: d\n   data: [-0.28, 0.07, 0.0002, 1.7e-05, 0.0, 0, 0, 0, %s, 0, 0, 0]"
    for s1, ok in (("0.001", False), ("0", True)):
        (tmp_path / "prism.yaml").write_text(re.sub(r"cols: 5\n   dt: d\n   data: \[-0.28340811[^\]]*\]", d12 % s1, text))
        if ok:
            assert list(pkg.Camera(tmp_path / "prism.yaml").cams[0].D)[:2] == [-0.28, 0.07]
        else:
            with pytest.raises(ValueError, match="not modelled"):
                pkg.Camera(tmp_path / "prism.yaml")


def test_build_maps_refuses_bad_cameras():
    from rspl_slam_amd import camera, capi
    lib = capi.load()
    K, D, R, P = synthetic(96, 64, 60, 0)
    out = np.empty((64, 96), np.float32)

    def rc(cam, model=0, H=64, W=96):
        return lib.rspl_rect_build_maps(C.byref(cam), model, H, W, out.ctypes.data, out.ctypes.data)

    good = camera.rect_camera(K, D, R, P)
    assert rc(good) == 0
    assert rc(good, 2) == -1 and rc(good, 0, 0, 96) == -1 and rc(good, 0, 64, 2045) == -1
    singular = camera.rect_camera(K, D, R, [0.0] * 12)
    assert rc(singular) == -1 and b"singular" in lib.rspl_last_error()
    fish = camera.rect_camera(K, [0.1, 0, 0, 0], R, P, 1)
    assert rc(fish, 1) == 0
    fish.D[5] = 0.01  # the fisheye model has four coefficients
    assert rc(fish, 1) == -1
    bad = camera.rect_camera(K, D, R, P)
    bad.K[0] = float("nan")
    assert rc(bad) == -1


@pytest.mark.parametrize("kw", [dict(height=0), dict(width=2045), dict(max_batch=0), dict(distortion_type=2),
                                dict(height=2045), dict(width=-3), dict(max_batch=1025)])
def test_create_rejects_bad_config_before_the_device(kw):
    from rspl_slam_amd import camera, capi
    lib = capi.load()
    cam = camera.rect_camera(*synthetic(96, 64, 60, 0))
    args = dict(height=64, width=96, distortion_type=0, max_batch=2)
    args.update(kw)
    cfg = capi.RectConfig(args["height"], args["width"], args["distortion_type"], (capi.RectCamera * 2)(cam, cam),
                          args["max_batch"], 0)
    h = C.c_void_p()
    assert lib.rspl_rect_create(C.byref(cfg), C.byref(h)) == -1  # RSPL_E_ARG, not a device error
    assert not h.value
    with pytest.raises(ValueError):
        _pkg().Rectifier(args["height"], args["width"], [cam, cam], args["distortion_type"], args["max_batch"])
