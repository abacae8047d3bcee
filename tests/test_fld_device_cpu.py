"""The device line detector's CPU-checkable parts (no GPU): the component-wise decomposition restated in Python
(tests/fld_parallel_ref.py) against oracle/fld_ref.py, the shared host / device header (csrc/fld_device.hpp)
through rspl_lines_debug_fld_host against the same restatement, bit for bit, the host detector from Canny's
classes (csrc/fld_host.hpp, what rspl_lines_detect runs after the Canny kernel) through
rspl_lines_debug_fld_classes likewise, and the argument errors of rspl_lines_detect_device, refused before a
device is touched."""
import ctypes as C
import functools
import pathlib
import re
import subprocess

import numpy as np
import pytest

import fld_parallel_ref as PR
import fld_ref as FR
from conftest import pkg
from rspl_slam_amd import capi
from rspl_slam_amd import lines as L
from rspl_slam_amd import synthetic as SY

ROOT = pathlib.Path(__file__).resolve().parents[1]
IMAGES = [(64, 96, 4, 7), (96, 128, 3, 11), (70, 138, 2, 11)]  # h, w, seed, segments of the sequential detector
FUNCS = ("rspl_lines_detect_device", "rspl_lines_detect_status", "rspl_lines_extract_async_device",
         "rspl_lines_debug_hysteresis", "rspl_lines_debug_chains", "rspl_lines_debug_fld_host",
         "rspl_lines_debug_fld_classes")


@functools.lru_cache(maxsize=None)
def _case(h, w, seed):
    half = FR.resize_half(SY.edge_map(h, w, n_lines=8, seed=seed)[0])
    return half, FR.fld_detect(half)


@pytest.mark.parametrize("h,w,seed,count", IMAGES)
def test_componentwise_walk_and_seed_order_equal_the_sequential_detector(h, w, seed, count):
    half, ref = _case(h, w, seed)
    assert len(ref) == count
    np.testing.assert_array_equal(PR.detect_parallel(half), ref)
    e = PR.edges_of(half)
    assert PR.walk_parallel(e) == PR.walk_sequential(e)


@pytest.mark.parametrize("h,w,seed,count", IMAGES)
def test_shared_header_on_the_host_equals_the_restatement(h, w, seed, count):
    half, ref = _case(h, w, seed)
    got = L.debug_fld_host(half, PR.edges_of(half))
    assert got.dtype == np.float32 and len(got) == count
    np.testing.assert_array_equal(got, ref)


def test_shared_header_capacity_and_bad_arguments():
    half, ref = _case(*IMAGES[1][:3])
    with pytest.raises(capi.RsplError, match="exceed capacity"):
        L.debug_fld_host(half, PR.edges_of(half), capacity=3)
    with pytest.raises(capi.RsplError):
        L.debug_fld_host(half, PR.edges_of(half), length_threshold=0)


# --- the product's host half from Canny's classes (rspl_lines_debug_fld_classes runs what rspl_lines_detect runs) ---
DT = 1.414213562


def _restate(half, cls, lt=10, dt=DT):
    chains = PR.walk_sequential(PR.zero_corners(FR.hysteresis(cls).copy()))
    return np.array([s[2] for s in PR.segments_of(half, chains, lt, dt)], np.float32).reshape(-1, 4)


def _random_half(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


@pytest.mark.parametrize("h,w,seed,count", IMAGES)
def test_host_detector_from_classes_equals_the_oracle(h, w, seed, count):
    half, ref = _case(h, w, seed)
    got = L.debug_fld_classes(half, FR.canny_classes(half, 200, 250))
    assert got.dtype == np.float32 and len(got) == count
    np.testing.assert_array_equal(got, ref)


def test_host_detector_spiral_deep_hysteresis_one_long_turning_chain():
    cls, path = PR.spiral_classes(64)
    cls[path[len(path) // 2]] = 2
    half = _random_half(64, 64, 3)
    ref = _restate(half, cls)
    assert len(ref) >= 1
    np.testing.assert_array_equal(L.debug_fld_classes(half, cls), ref)


def _box_classes():
    cls = np.ones((24, 40), np.uint8)
    cls[7, 7:33] = cls[16, 7:33] = 0
    cls[7:17, 7] = cls[7:17, 32] = 0
    cls[7, 20] = 2
    return cls


@pytest.mark.parametrize("lt,count", [(3, 4), (10, 2)])
def test_host_detector_box_at_two_length_thresholds(lt, count):
    cls, half = _box_classes(), _random_half(24, 40, 5)
    ref = _restate(half, cls, lt)
    assert len(ref) == count
    np.testing.assert_array_equal(L.debug_fld_classes(half, cls, length_threshold=lt), ref)


@pytest.mark.parametrize("lt", [1, 3, 5])
def test_host_detector_border_ring_gives_no_segment(lt):
    """both corner zeroings and the border filter apply; the walk tests out-of-image neighbours on all four sides"""
    cls = np.ones((12, 12), np.uint8)
    cls[0, :] = cls[-1, :] = cls[:, 0] = cls[:, -1] = 0
    cls[0, 7] = 2
    half = _random_half(12, 12, 6)
    ref = _restate(half, cls, lt)
    assert len(ref) == 0
    np.testing.assert_array_equal(L.debug_fld_classes(half, cls, length_threshold=lt), ref)


def test_host_detector_two_by_two_of_strong_pixels():
    got = L.debug_fld_classes(_random_half(2, 2, 7), np.full((2, 2), 2, np.uint8))
    assert got.shape == (0, 4)  # rc 0: the binding raises on any other


def test_host_detector_capacity_and_bad_arguments():
    half, _ = _case(*IMAGES[1][:3])
    cls = FR.canny_classes(half, 200, 250)
    with pytest.raises(capi.RsplError, match="exceed capacity"):
        L.debug_fld_classes(half, cls, capacity=3)
    # the rows written before the error, read through the C call itself; a fourth row must stay untouched
    lib, seg, n = L._declare(capi.load()), np.full((4, 4), -1.0, np.float32), C.c_int()
    rc = lib.rspl_lines_debug_fld_classes(half.ctypes.data_as(L._u8p), cls.ctypes.data_as(L._u8p), half.shape[0],
                                          half.shape[1], C.byref(L.FldConfig(10, DT, 0.0, 0.0, 3)),
                                          seg.ctypes.data_as(L._fp), 3, C.byref(n))
    ref = _restate(half, cls)
    assert rc != 0 and n.value == len(ref) > 3
    np.testing.assert_array_equal(seg[:3], ref[:3])
    assert (seg[3] == -1.0).all()
    with pytest.raises(capi.RsplError):
        L.debug_fld_classes(half, cls, length_threshold=0)


def test_host_detector_header_alone_in_a_plain_program():
    """tests/c/fld_check.cpp: csrc/fld_host.hpp compiled by the host compiler with no librspl, on the box, ring,
    spiral and 2 x 2 maps built in C++, at capacity 0 and ample; it exits non-zero on any count but the ones above"""
    exe = ROOT / "tests" / "c" / "build" / "fld_check"
    # always through make, whose rule names the two headers: a binary of an older header is rebuilt
    subprocess.run(["make", "-C", str(ROOT / "tests" / "c"), "build/fld_check"], check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    for name in ("box", "ring", "spiral", "2x2"):
        assert any(line.startswith(name) for line in run.stdout.splitlines()), run.stdout


def test_header_and_binding_declare_the_device_detector():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    lib = L._declare(capi.load())
    for n in FUNCS:
        assert n in names and n in capi.EXPORTS and hasattr(lib, n)
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct or call changed
    assert len(lib.rspl_lines_detect_device.argtypes) == 12 and len(lib.rspl_lines_extract_async_device.argtypes) == 8
    for m in ("detect_device", "submit_device", "debug_hysteresis", "debug_chains", "detect_status"):
        assert callable(getattr(L.LineDetector, m))


def test_detect_device_refuses_bad_arguments_before_any_device_call():
    """No handle exists without a device, and the handle is the last argument looked at: every shape error below
    is reported as such with a NULL handle, and a call that is right in everything else is refused for the handle."""
    lib = L._declare(capi.load())
    cfg = L.FldConfig(10, 1.414213562, 200.0, 250.0, 3)
    fake = 0x1000  # never dereferenced

    def call(batch=1, H=480, W=752, stride=None, pitch=None, cfg=cfg, cap=16, seg=fake, h=None):
        stride = W if stride is None else stride
        pitch = stride * H if pitch is None else pitch
        rc = lib.rspl_lines_detect_device(h, fake, batch, H, W, stride, pitch, C.byref(cfg) if cfg else None, seg, cap,
                                          fake, None)
        return rc, lib.rspl_last_error().decode()

    for kw, msg in [(dict(batch=0), "batch"), (dict(batch=3), "batch"), (dict(H=481), "even sizes"),
                    (dict(W=751), "even sizes"), (dict(H=2), "even sizes"), (dict(W=2), "even sizes"),
                    (dict(stride=750), "stride"), (dict(stride=760, pitch=760 * 479 + 751), "pitch"),
                    (dict(batch=2, pitch=752 * 480 - 1), "pitch"), (dict(H=2400, W=2400), "LDS budget"),
                    (dict(H=6, W=400000), "outside"), (dict(cfg=None), "rspl_fld_config"),
                    (dict(cfg=L.FldConfig(10, 1.4, 200.0, 250.0, 5)), "aperture"),
                    (dict(cfg=L.FldConfig(0, 1.4, 200.0, 250.0, 3)), "thresholds"), (dict(cap=-1), "capacity"),
                    (dict(seg=None), "capacity")]:
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    # the asynchronous job checks the same before it touches a device
    for H, W, stride, msg in ((481, 752, 752, "even sizes"), (480, 752, 700, "stride"), (2400, 2400, 2400, "LDS budget"),
                              (480, 752, 752, "NULL argument")):
        assert lib.rspl_lines_extract_async_device(None, fake, H, W, stride, C.byref(cfg), 1, None) == -1
        assert msg in lib.rspl_last_error().decode(), (H, W, stride)
    # the limits admit the sizes the pipeline uses; only the handle is missing then
    for H, W in ((480, 752), (512, 640), (1080, 1920), (4, 4)):
        rc, err = call(H=H, W=W, stride=W + 8, pitch=(W + 8) * H + 24, batch=2)
        assert rc == -1 and "NULL argument" in err, (H, W, err)
