"""Time the device-resident F-matrix RANSAC chain (rspl_fm_enqueue: gather | hypotheses | counts | acceptance and
write-back, four launches) on one 400-match frame at 30 % outliers and on a batch of 64 such frames, against the
numpy restatement (tests/fm_ref.py) on one CPU core for the same inputs.  No earlier commit has this stage.

Times are HIP events around `--calls` back-to-back rspl_fm_enqueue calls on one stream after `--warmup` calls.
A handle takes one enqueue at a time, so the calls rotate over a ring of handles and a handle is fetched just
before it is reused, `--ring` calls later -- its chain finished long before, the stream never runs dry.

  python tools/bench_fm.py --out profiles/fm_bench.json
"""
import argparse
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
from rspl_slam_amd import capi  # noqa: E402

N, OUTLIERS, NOISE, K = 400, 0.3, 0.3, 512


def frame(seed):
    """a 400-match frame: every keypoint matched (a permutation), SuperPoint records on the device"""
    import fm_cases as FC
    rng = np.random.default_rng(seed)
    p0, p1, _, _ = FC.scene(N, OUTLIERS, NOISE, seed)
    perm = rng.permutation(N).astype(np.int32)       # keypoint i of image 0 <-> keypoint perm[i] of image 1
    inv = np.empty(N, np.int32)
    inv[perm] = np.arange(N, dtype=np.int32)
    pts1 = np.empty_like(p1)
    pts1[perm] = p1
    bufs = dict(rec0=FC.superpoint_records(p0, N, rng), rec1=FC.superpoint_records(pts1, N, rng), idx0=perm, idx1=inv)
    return p0, p1, bufs


def upload(b):
    def dev(a):
        a = np.ascontiguousarray(a)
        return capi.DeviceBuffer(max(a.nbytes, 8)).upload(a)
    n = dev(np.array([N], np.int32))
    return dict(d_features0=dev(b["rec0"]), d_n0=n, d_features1=dev(b["rec1"]), d_n1=n, d_idx0=dev(b["idx0"]),
                d_idx1=dev(b["idx1"]), d_idx0_out=capi.DeviceBuffer(4 * N), d_idx1_out=capi.DeviceBuffer(4 * N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fm_bench.json"))
    args = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_fm: no HIP device")
    import fm_ref
    lib = capi.load()
    stream, timer = capi.Stream(), capi.Timer()
    scenes = [frame(1000 + s) for s in range(64)]
    # the yardstick: the restatement on one core, frame by frame
    cpu_ms, ref = [], []
    for p0, p1, _ in scenes:
        t0 = time.perf_counter()
        r = fm_ref.find_fundamental(p0, p1)
        cpu_ms.append((time.perf_counter() - t0) * 1e3)
        ref.append(r)
    devs = [upload(b) for _, _, b in scenes]
    rows = {}
    for name, batch in (("one_frame", 1), ("batch_64", 64)):
        ring = [pkg.FundamentalRansac(max_batch=batch, max_matches=K) for _ in range(args.ring)]
        busy = [False] * args.ring
        calls = [0]

        def enqueue():
            k = calls[0] % args.ring
            if busy[k]:
                ring[k].fetch()
            ring[k].enqueue(devs[:batch], stream=stream)
            busy[k] = True
            calls[0] += 1

        # the timed configuration computes what the restatement computes (its decisions, not its bits)
        enqueue()
        got = ring[0].fetch()
        busy[0] = False
        same = sum(int(g["n_inliers"] == r["n_inliers"] and g["hypotheses"] == r["hypotheses"] and
                       np.array_equal(g["inlier"], r["mask"])) for g, r in zip(got, ref))
        for _ in range(args.warmup):
            enqueue()
        t = []
        for _ in range(args.repeats):
            timer.start(stream)
            for _ in range(args.calls):
                enqueue()
            timer.stop(stream)
            t.append(timer.elapsed_ms() * 1e3 / args.calls)
        for k in range(args.ring):
            if busy[k]:
                ring[k].fetch()
        us = statistics.median(t)
        cpu = sum(cpu_ms[:batch])
        rows[name] = dict(frames=batch, matches=N, outliers=OUTLIERS, noise_px=NOISE,
                          enqueue_us=round(us, 1), enqueue_us_min_max=[round(min(t), 1), round(max(t), 1)],
                          us_per_frame=round(us / batch, 2), cpu_restatement_ms=round(cpu, 1),
                          speedup_vs_one_core=round(cpu * 1e3 / us, 1),
                          iterations_solved_per_frame=ring[0].max_iters,
                          iterations_evaluated=[int(g["hypotheses"]) for g in got][:8],
                          inliers=[int(g["n_inliers"]) for g in got][:8],
                          frames_equal_to_restatement=f"{same}/{batch}")
        print(f"{name}: {us:.1f} us per enqueue ({us / batch:.2f} us per frame), fm_ref on one core {cpu:.1f} ms "
              f"({cpu * 1e3 / us:.0f}x); {same}/{batch} frames decide as the restatement", flush=True)
        del ring
    res = dict(what="HIP events around back-to-back rspl_fm_enqueue calls on one stream, median of windows; "
                    "yardstick: tests/fm_ref.py on one core, same inputs",
               calls=args.calls, warmup=args.warmup, repeats=args.repeats, ring=args.ring,
               version=lib.rspl_version().decode(), workloads=rows)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
