"""Time local map tracking (rspl_lmap_*) on one frame at C3 (752x480, 400 keypoints, 3600 local points), C4 (640x512,
600 keypoints, 5400 local points) and C5 (1920x1080, 2048 keypoints, 18432 local points): the search alone
(rspl_lmap_enqueue: prep | search | merge, three launches) and the whole chain (rspl_lmap_track_enqueue: the same
three launches, then the tracking step's six), against the numpy restatement of the search (tests/lmap_ref.py) on
one CPU core for the same inputs.  No earlier commit has this stage.

Times are HIP events around `--calls` back-to-back enqueues on one stream after `--warmup` calls.  A handle takes one
enqueue at a time, so the calls rotate over a ring of handles and a handle is fetched just before it is reused,
`--ring` calls later -- its chain finished long before, the stream never runs dry.

  python tools/bench_lmap.py --out profiles/lmap_bench.json
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

CAM = (458.654, 457.296, 367.215, 248.375, 50.0)
WORKLOADS = dict(C3=dict(width=752, height=480, n_kp=400, n_local=3600),
                 C4=dict(width=640, height=512, n_kp=600, n_local=5400),
                 C5=dict(width=1920, height=1080, n_kp=2048, n_local=18432))
OWN = 0.1        # keypoints that hold a point of their own
VISIBLE = 0.6    # local points that project into the image
NEAR = 0.5       # ... of which this share sits near a free keypoint, with a descriptor near its own


def scene(width, height, n_kp, n_local, seed):
    """one frame and its local map in tests/lmap_ref.py's format, at a known pose"""
    import lmap_cases as LC
    rng = np.random.default_rng(seed)
    cam = (CAM[0] * width / 752, CAM[1] * width / 752, width / 2 - 8.8, height / 2 + 8.4, CAM[4])
    gt = LC.random_pose(rng)
    F = np.zeros((n_kp, 259))
    F[:, 0] = rng.uniform(0.01, 1, n_kp)
    F[:, 1], F[:, 2] = rng.integers(4, width - 4, n_kp), rng.integers(4, height - 4, n_kp)  # SuperPoint: whole pixels
    F[:, 3:] = LC.unit(rng, n_kp)
    own = rng.uniform(size=n_kp) < OWN
    depth = rng.uniform(2, 15, n_kp)
    xyz = np.array([LC.pixel_point(F[i, 1], F[i, 2], depth[i], gt, cam) for i in range(n_kp)])
    pid = np.where(own, 100000 + np.arange(n_kp), -1).astype(np.int32)
    free = np.flatnonzero(~own)
    pos, desc = np.zeros((n_local, 3)), LC.unit(rng, n_local)
    for p in range(n_local):
        r = rng.uniform()
        if r < VISIBLE * NEAR:  # the projection of a free keypoint's own landmark, its descriptor seen again
            i = free[rng.integers(len(free))]
            pos[p] = LC.pixel_point(F[i, 1] + rng.normal(0, 1.5), F[i, 2] + rng.normal(0, 1.5), depth[i], gt, cam)
            desc[p] = LC.at_distance(F[i, 3:], rng.uniform(0.02, 0.4), rng)
        elif r < VISIBLE:
            pos[p] = LC.pixel_point(rng.uniform(0, width), rng.uniform(0, height), rng.uniform(2, 15), gt, cam)
        else:  # around the image or behind the camera
            z = rng.uniform(2, 15) * (1 if rng.uniform() < 0.7 else -1)
            pos[p] = LC.pixel_point(rng.uniform(-width, 2 * width), rng.uniform(-height, 2 * height), z, gt, cam)
    fr = dict(features=F, u_right=None, point_id=pid, point_xyz=xyz, Twc=gt, cam=cam, width=width, height=height)
    lm = dict(ids=np.arange(n_local, dtype=np.int32) + 1, pos=pos, desc=desc)
    held = np.flatnonzero(own)[::2]  # every other held point is one of the local map's: not selected by the search
    pid[held] = lm["ids"][rng.choice(n_local, len(held), replace=False)]
    return fr, lm


def dev(a):
    a = np.ascontiguousarray(a)
    return capi.DeviceBuffer(max(a.nbytes, 8)).upload(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--workloads", default="C3,C4,C5")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lmap_bench.json"))
    args = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_lmap: no HIP device")
    import lmap_ref as LR
    lib = capi.load()
    stream, timer = capi.Stream(), capi.Timer()
    rows = {}
    for name in args.workloads.split(","):
        w = WORKLOADS[name]
        fr, lm = scene(seed=2000 + len(rows), **w)
        t0 = time.perf_counter()
        want = LR.search(fr, lm)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        kp, pt = LR.good_list(want)
        assoc, _ = LR.merge(fr, lm, kp, pt)
        n1, nl = w["n_kp"], w["n_local"]
        d = dict(d_features=dev(fr["features"]), d_n1=dev(np.array([n1], np.int32)), d_point_id=dev(fr["point_id"]),
                 d_point_xyz=dev(fr["point_xyz"]), Twc=fr["Twc"], cam=fr["cam"], width=fr["width"], height=fr["height"])
        tf = dict(slot=0, d_features=d["d_features"], d_n1=d["d_n1"], cam=fr["cam"], last_Twc=fr["Twc"])
        ring = []
        for _ in range(args.ring):
            h = pkg.LocalMap(max_bank_points=nl, max_local_points=nl, max_keypoints=n1, max_batch=1)
            h.store_host(lm["ids"], lm["desc"])
            h.set_local(lm["ids"], lm["pos"], stream)
            ring.append((h, pkg.Tracker(max_batch=1, max_keypoints=n1)))
        row = dict(keypoints=n1, local_points=nl, image=[w["width"], w["height"]], cpu_restatement_search_ms=round(cpu_ms, 1),
                   status_counts=dict(zip(("not_selected", "behind", "off_image", "no_candidate", "failed", "good"),
                                          (int(c) for c in np.bincount(want["status"], minlength=6)))))
        for mode in ("search", "chain"):
            busy = [None] * args.ring
            calls = [0]

            def fetch(k):
                h, t = ring[k]
                r = (t.fetch()[0] if busy[k] == "chain" else None, h.fetch()[0])
                busy[k] = None
                return r

            def enqueue():
                k = calls[0] % args.ring
                if busy[k]:
                    fetch(k)
                h, t = ring[k]
                if mode == "search":
                    h.enqueue([d], stream=stream)
                else:
                    h.track_enqueue(t, [d], [tf], stream=stream)
                busy[k] = mode
                calls[0] += 1

            # the timed configuration computes what the restatement computes, bit for bit
            enqueue()
            tr, s = fetch(0)
            p = ring[0][0].debug_points(0)
            same = bool(np.array_equal(p["status"], want["status"]) and np.array_equal(p["best_idx"], want["best_idx"]) and
                        np.array_equal(p["best"].view(np.int64), want["best"].view(np.int64)) and
                        np.array_equal(p["second"].view(np.int64), want["second"].view(np.int64)) and
                        np.array_equal(s["good_kp"], kp) and np.array_equal(s["good_point"], pt) and
                        np.array_equal(s["assoc_id"], assoc))
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
                    fetch(k)
            us = statistics.median(t)
            row[mode] = dict(enqueue_us=round(us, 1), enqueue_us_min_max=[round(min(t), 1), round(max(t), 1)],
                             equal_to_restatement_bitwise=same)
            if mode == "search":
                row[mode]["speedup_vs_one_core"] = round(cpu_ms * 1e3 / us, 1)
            else:
                err = float(np.abs(tr["pose_p"] - fr["Twc"][:3, 3]).max())
                row[mode].update(n_good=int(s["n_good"]), n_inliers=int(tr["n_inliers"]), pose_set=bool(tr["pose_set"]),
                                 translation_error_m=float(f"{err:.3g}"))
            print(f"{name} {mode}: {us:.1f} us per enqueue; lmap_ref's search on one core {cpu_ms:.0f} ms; "
                  f"equal to the restatement: {same}", flush=True)
        rows[name] = row
        del ring
    res = dict(what="HIP events around back-to-back rspl_lmap_enqueue (search) / rspl_lmap_track_enqueue (chain) calls "
                    "on one stream, one frame per call, median of windows; yardstick: tests/lmap_ref.py's search on "
                    "one core, same inputs",
               calls=args.calls, warmup=args.warmup, repeats=args.repeats, ring=args.ring,
               version=lib.rspl_version().decode(), workloads=rows)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
