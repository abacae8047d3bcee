"""Time the rectifying remap (rspl_rect_enqueue_device, one launch per stereo pair) at the C3, C4 and C5 image
sizes against the copy kernel of copy_kernels.hip moving the same input + output bytes device to device, and
against the numpy restatement on one CPU core.

The remap moves 1 (source) + 1 (output) + 4 (table) bytes per pixel, the copy 1 + 1: up to 3x the copy's
time is bytes alone, the rest is the gather.  Times are HIP events around `--launches` back-to-back launches
on one stream after a warm-up, the remap and the copy alternating, the median of `--repeats` windows.

  python tools/bench_rect.py --out profiles/rect_bench.json
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import rspl_loader  # noqa: E402

pkg = rspl_loader.load()
from rspl_slam_amd import camera, capi  # noqa: E402

PAIRS = 32  # pairs per launch of the batched rows
SIZES = {"C3": (752, 480), "C4": (640, 512), "C5": (1920, 1080)}


def scaled_euroc(W, H):
    """EuRoC's calibration (tests/golden/calib/euroc.yaml) with K and P scaled to W x H: the same view, so the
    same relative gather pattern, at every size."""
    c = pkg.Camera(ROOT / "tests" / "golden" / "calib" / "euroc.yaml")
    sx, sy = W / c.ImageWidth(), H / c.ImageHeight()
    cams = []
    for rc in c.cams:
        K, P = np.array(rc.K).reshape(3, 3), np.array(rc.P).reshape(3, 4)
        K[0] *= sx
        K[1] *= sy
        P[0] *= sx
        P[1] *= sy
        cams.append(camera.rect_camera(K, list(rc.D), list(rc.R), P))
    return cams


def window(fn, stream, timer, launches):
    timer.start(stream)
    for _ in range(launches):
        fn()
    timer.stop(stream)
    return timer.elapsed_ms() * 1e3 / launches  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rect_bench.json"))
    args = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_rect: no HIP device")
    import rect_ref as RR
    lib = capi.load()
    stream, timer = capi.Stream(), capi.Timer()
    rng = np.random.default_rng(0)
    rows = {}
    for name, (W, H) in SIZES.items():
        rect = pkg.Rectifier(H, W, scaled_euroc(W, H), 0, max_batch=2 * PAIRS)
        px = H * W
        raws = rng.integers(0, 256, (2 * PAIRS, H, W), dtype=np.uint8)
        d_raw, d_out = capi.DeviceBuffer(2 * PAIRS * px), capi.DeviceBuffer(2 * PAIRS * px)
        d_raw.upload(raws)
        idx = (C.c_int * (2 * PAIRS))(*([0, 1] * PAIRS))

        def remap(n=2):  # the ctypes call itself: nothing of Python's per launch but this
            rc = lib.rspl_rect_enqueue_device(rect._h, n, d_raw.ptr, W, px, idx, d_out.ptr, W, px, stream.handle)
            assert rc == 0, lib.rspl_last_error()

        def copy(n=2):
            rc = lib.rspl_rect_debug_copy(d_out.ptr, d_raw.ptr, n * px, stream.handle)
            assert rc == 0, lib.rspl_last_error()

        # the timed configuration computes what the restatement computes
        remap()
        got = d_out.download((2, H, W), np.uint8, stream=stream.handle)  # (the first pair of the buffer)
        maps = [rect.get_maps(c) for c in (0, 1)]
        t0 = time.perf_counter()
        ref = [RR.remap(raws[c], *maps[c]) for c in (0, 1)]
        cpu_ms = (time.perf_counter() - t0) * 1e3
        assert all(got[c].tobytes() == ref[c].tobytes() for c in (0, 1)), f"{name}: the remap differs from the restatement"
        outside = float(np.mean([np.mean(RR.classes(*maps[c], H, W) != 2) for c in (0, 1)]))

        for fn in (remap, copy):
            window(fn, stream, timer, args.warmup)
        t_remap, t_copy = [], []
        for _ in range(args.repeats):
            t_remap.append(window(remap, stream, timer, args.launches))
            t_copy.append(window(copy, stream, timer, args.launches))
        r, c = statistics.median(t_remap), statistics.median(t_copy)
        # PAIRS pairs per launch: the launch's fixed cost spread thin, what is left is the kernels' own rate
        few = max(args.launches // PAIRS, 8)
        for fn in (remap, copy):
            window(lambda: fn(2 * PAIRS), stream, timer, 4)
        b_remap, b_copy = [], []
        for _ in range(args.repeats):
            b_remap.append(window(lambda: remap(2 * PAIRS), stream, timer, few) / PAIRS)
            b_copy.append(window(lambda: copy(2 * PAIRS), stream, timer, few) / PAIRS)
        rb, cb = statistics.median(b_remap), statistics.median(b_copy)
        rows[name] = dict(width=W, height=H, remap_us=round(r, 2), copy_us=round(c, 2), ratio=round(r / c, 2),
                          remap_us_min_max=[round(min(t_remap), 2), round(max(t_remap), 2)],
                          copy_us_min_max=[round(min(t_copy), 2), round(max(t_copy), 2)],
                          remap_gbytes_per_s=round(6 * 2 * px / (r * 1e-6) / 1e9, 1),
                          copy_gbytes_per_s=round(2 * 2 * px / (c * 1e-6) / 1e9, 1),
                          batched_pairs=PAIRS, batched_remap_us_per_pair=round(rb, 2),
                          batched_copy_us_per_pair=round(cb, 2), batched_ratio=round(rb / cb, 2),
                          batched_remap_gbytes_per_s=round(6 * 2 * px / (rb * 1e-6) / 1e9, 1),
                          batched_copy_gbytes_per_s=round(2 * 2 * px / (cb * 1e-6) / 1e9, 1),
                          cpu_restatement_ms=round(cpu_ms, 1), pixels_not_wholly_inside=round(outside, 4))
        print(f"{name} {W}x{H}: remap {r:.2f} us, copy {c:.2f} us ({r / c:.2f}x); {PAIRS} pairs per launch: "
              f"{rb:.2f} / {cb:.2f} us per pair ({rb / cb:.2f}x); numpy on one core {cpu_ms:.0f} ms",
              flush=True)
    res = dict(what="one launch per stereo pair, HIP events around back-to-back launches, median of windows",
               launches=args.launches, repeats=args.repeats, warmup=args.warmup,
               bytes_per_pixel=dict(remap=6, copy=2), calibration="EuRoC, K and P scaled to the size",
               version=lib.rspl_version().decode(), sizes=rows)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
