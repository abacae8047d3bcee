"""Event scopes and the device copy kernel: ordering events carry a device-scope release,
timing events no system fence, and rspl_memcpy_d2d is a copy kernel.  What must still hold: a post-stream SuperGlue
call is ordered exactly as before (every one of 20 back-to-back calls gives the single-stream call's matches), the
stage timers still measure (finite, non-negative, inside the call's wall time), and the copy is exact for any byte
count and alignment."""
import time

import numpy as np
import pytest

from rspl_slam_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import rspl_loader
    return rspl_loader.load()


@pytest.fixture(scope="module")
def sg_small(pkg, golden, weight_blobs):
    g = golden("sg_small")
    F0, F1 = g["F0"].astype(np.float64), g["F1"].astype(np.float64)
    nmax = max(F0.shape[1], F1.shape[1])
    sg = pkg.SuperGlue(pkg.SuperGlueConfig(weights=weight_blobs[1], max_keypoints=nmax, max_batch=1))
    assert sg.build(), sg.error
    f0, f1 = np.zeros((1, nmax, 259)), np.zeros((1, nmax, 259))
    f0[0, :F0.shape[1]] = F0.T
    f1[0, :F1.shape[1]] = F1.T
    n0, n1 = np.array([F0.shape[1]], np.int32), np.array([F1.shape[1]], np.int32)
    bufs = {k: capi.DeviceBuffer(v.nbytes).upload(v) for k, v in dict(f0=f0, f1=f1, n0=n0, n1=n1).items()}
    return sg, bufs, nmax, int(n0[0]), int(n1[0])


def _outs(nmax):
    return {k: capi.DeviceBuffer(nmax * sz) for k, sz in dict(i0=4, i1=4, m0=8, m1=8).items()}


def _call(sg, bufs, nmax, o, st, pst=None):
    sg.infer_device(1, bufs["f0"].ptr, bufs["n0"].ptr, bufs["f1"].ptr, bufs["n1"].ptr, nmax, True, o["i0"].ptr,
                    o["i1"].ptr, o["m0"].ptr, o["m1"].ptr, st.handle, post_stream=pst.handle if pst else None)


def _read(o, nmax, n0, n1):
    return (o["i0"].download((nmax,), np.int32)[:n0], o["i1"].download((nmax,), np.int32)[:n1],
            o["m0"].download((nmax,), np.float64)[:n0], o["m1"].download((nmax,), np.float64)[:n1])


def test_post_stream_calls_equal_single_stream(sg_small):
    sg, bufs, nmax, n0, n1 = sg_small
    st, pst = capi.Stream(), capi.Stream()
    ref_o = _outs(nmax)
    _call(sg, bufs, nmax, ref_o, st)
    capi.synchronize()
    ref = _read(ref_o, nmax, n0, n1)
    assert (ref[0] >= 0).sum() > 0
    outs = [_outs(nmax) for _ in range(20)]
    for o in outs:  # back to back: no host wait between the calls
        _call(sg, bufs, nmax, o, st, pst)
    capi.synchronize()
    ok, mask = sg.status()
    assert ok, sg.error
    for o in outs:
        for a, b in zip(ref, _read(o, nmax, n0, n1)):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("post", [False, True], ids=["single-stream", "post-stream"])
def test_stage_times_inside_the_call(sg_small, post):
    sg, bufs, nmax, n0, n1 = sg_small
    st, pst = capi.Stream(), capi.Stream()
    o = _outs(nmax)
    try:
        sg.profile(True)
        _call(sg, bufs, nmax, o, st, pst if post else None)  # (first use of the streams)
        capi.synchronize()
        sg.profile(True)  # reset
        t0 = time.perf_counter()
        _call(sg, bufs, nmax, o, st, pst if post else None)
        capi.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms, calls = sg.stage_times()
    finally:
        sg.profile(False)
    print(f"stages {[round(v, 4) for v in ms]} sum {sum(ms):.4f} ms, wall {wall_ms:.4f} ms")
    assert calls == 1
    assert all(np.isfinite(v) and v >= 0.0 for v in ms), ms
    assert sum(ms) > 0.0
    assert sum(ms) <= wall_ms


def test_timer_measures_a_kernel():
    """rspl_timer (no system fence): a copy's time is finite, positive and inside the host's wall time"""
    st = capi.Stream()
    a, b = capi.DeviceBuffer(1 << 24), capi.DeviceBuffer(1 << 24)
    a.zero()
    capi.synchronize()
    tm = capi.Timer()
    t0 = time.perf_counter()
    tm.start(st)
    capi.memcpy_d2d(b.ptr, a.ptr, 1 << 24, st.handle)
    tm.stop(st)
    ms = tm.elapsed_ms()
    wall_ms = (time.perf_counter() - t0) * 1e3
    assert np.isfinite(ms) and 0.0 < ms <= wall_ms


@pytest.mark.parametrize("offsets", [(1, 1), (3, 1), (4, 12), (4, 8), (0, 0), (7, 23)],
                         ids=lambda o: f"dst+{o[0]}-src+{o[1]}")
@pytest.mark.parametrize("nbytes", [1, 3, 4, 5, 4095, 828800])
def test_memcpy_d2d_exact(nbytes, offsets):
    """every access width of the copy kernel (the two addresses' common alignment: 16, 8, 4, 1 bytes), head and tail
    bytes included; nothing outside [dst, dst + nbytes) is touched"""
    do, so = offsets
    rng = np.random.default_rng(nbytes * 31 + do * 7 + so)
    pad = 64
    src = rng.integers(0, 256, nbytes + 2 * pad, dtype=np.uint8)
    dst0 = np.full(nbytes + 2 * pad, 0xA5, np.uint8)
    st = capi.Stream()
    d_src, d_dst = capi.DeviceBuffer(src.nbytes).upload(src), capi.DeviceBuffer(dst0.nbytes).upload(dst0)
    capi.memcpy_d2d(d_dst.offset(do), d_src.offset(so), nbytes, st.handle)
    st.synchronize()
    got = d_dst.download(dst0.shape, np.uint8)
    want = dst0.copy()
    want[do:do + nbytes] = src[so:so + nbytes]
    np.testing.assert_array_equal(got, want)
