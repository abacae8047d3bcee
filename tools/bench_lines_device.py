"""The line detector on the device against the host path, per image and alone on the GPU.

For RCF-like edge maps (synthetic.edge_map) at 752x480, 640x512 and 1920x1080 (40 / 40 / 120 lines):
  * rspl_lines_detect_device's six launches by HIP events (Canny classes, hysteresis, labels, walk, fit, order),
  * its counters: hysteresis passes, edge pixels, components, the largest component, chains, segments, and the
    walk's iteration count (the busiest lane), from which the walk's time per iteration follows,
  * the end-to-end job time of rspl_lines_extract_async_device (submit to the worker's end) and the wall time
    from submit to the return of wait,
  * the same two figures of the host path rspl_lines_extract_async (unchanged by the device detector) on the
    same image.
Warm-up runs first, then --iters repeats; medians with the 10th / 90th percentiles and the extremes.  Writes
profiles/lines_device_bench.json (or --out)."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import rspl_loader  # noqa: E402

pkg = rspl_loader.load()
pkg.capi.load()
L, C = pkg.lines, pkg.capi

CASES = [(480, 752, 40), (512, 640, 40), (1080, 1920, 120)]


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2),
            "p90": round(float(np.percentile(v, 90)), 2), "min": round(float(v.min()), 2),
            "max": round(float(v.max()), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lines_device_bench.json"))
    a = ap.parse_args()
    rows = []
    for H, W, n_lines in CASES:
        img = pkg.synthetic.edge_map(H, W, n_lines=n_lines, seed=a.seed)[0]
        det = L.LineDetector()
        st = C.Stream()
        d_img = C.DeviceBuffer(H * W).upload(img, st.handle)
        cap = 4096
        d_seg, d_cnt = C.DeviceBuffer(cap * 16), C.DeviceBuffer(4)
        # the device detector's stages by events
        det.debug_fld_profile(True)
        stages = {k: [] for k in L.FLD_STAGES}
        for it in range(a.warmup + a.iters):
            det.detect_device(d_img, 1, H, W, W, H * W, d_seg, cap, d_cnt, st)
            ms = det.debug_fld_stage_ms()
            if it >= a.warmup:
                for k, v in ms.items():
                    stages[k].append(v * 1e3)
        det.debug_fld_profile(False)
        stats = det.debug_fld_stats(0)
        n_dev = int(d_cnt.download(1, np.int32, stream=st.handle)[0])
        n_host = len(det.detect(img))
        stage_us = {k: spread(v) for k, v in stages.items()}
        total = spread(np.sum([stages[k] for k in L.FLD_STAGES], axis=0))
        # the asynchronous jobs, each alone: device image in, then the host path on the host image
        job = {"device": ([], []), "host": ([], [])}
        for it in range(a.warmup + a.iters):
            st.synchronize()
            t = time.perf_counter()
            det.submit_device(d_img, H, W, W, st)
            lines_dev, ms = det.wait()
            wall = (time.perf_counter() - t) * 1e6
            if it >= a.warmup:
                job["device"][0].append(ms * 1e3)
                job["device"][1].append(wall)
        for it in range(a.warmup + a.iters):
            t = time.perf_counter()
            det.submit(img)
            lines_host, ms = det.wait()
            wall = (time.perf_counter() - t) * 1e6
            if it >= a.warmup:
                job["host"][0].append(ms * 1e3)
                job["host"][1].append(wall)
        walk_us = stage_us["walk"]["median"]
        rows.append({"image": f"{W}x{H}", "lines_drawn": n_lines, "segments_device": n_dev, "segments_host": n_host,
                     "lines_equal": bool(np.array_equal(lines_dev, lines_host)), "counters": stats,
                     "stage_us": stage_us, "stages_total_us": total,
                     "walk_ns_per_iteration": round(walk_us * 1e3 / max(1, stats["walk_iterations"]), 1),
                     "extract_async_device_job_us": spread(job["device"][0]),
                     "extract_async_device_wall_us": spread(job["device"][1]),
                     "extract_async_host_job_us": spread(job["host"][0]),
                     "extract_async_host_wall_us": spread(job["host"][1])})
        print(json.dumps(rows[-1]), flush=True)
    out = {"what": "rspl_lines_detect_device stages and extract_async_device against the host extract_async, "
                   "each alone on one MI355X; microseconds", "iters": a.iters, "warmup": a.warmup, "seed": a.seed,
           "cases": rows}
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
