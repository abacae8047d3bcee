"""Single-frame latency of turning a stereo frame into a keyframe for the tracker (Frame::AddRightFeatures, new
track ids, new map points, the tracker's keyframe table), two ways in one process on the same inputs, the
calls alternating:

  chain          KeyframeBuilder.enqueue -> fetch: one launch behind SuperGlue's device indices that ends in a
                 filled tracker slot, one sync
  host_composed  what a caller writes without rspl_kf_*: copy SuperGlue's two index arrays to the host, the
                 mutual check, the disparity filter and the back-projection in numpy, rspl_track_set_keyframe
                 (its upload waited for).  The keypoints' pixels are taken as already on the host.

Wall time per call around work that ends in a device synchronise; warm-up, then the median and the 10th / 90th
percentiles over --calls calls of each path.  Both paths must fill the same table.

Also recorded: rspl_map_insert_keyframe's bookkeeping and triangulation microseconds per keyframe over an
8-keyframe raw sequence (sequence.run_raw), next to sequence.run's insert_us on the sequence it was made from."""
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
from rspl_slam_amd import capi, sequence as SQ, synthetic as SY  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keypoints", type=int, default=400)
    ap.add_argument("--common", type=int, default=310)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "keyframe_insert.json"))
    a = ap.parse_args()
    if a.calls < 200:
        ap.error("--calls: the median is taken over at least 200 calls")
    n = a.keypoints
    p = SY.keyframe_problem(n_left=n, n_right=n, n_common=a.common, seed=0)
    fx, fy, cx, cy, bf = p["cam"]
    mn, mx, my = p["window"]
    R, t = p["Twc"][:3, :3], p["Twc"][:3, 3]

    def dev(x):
        x = np.ascontiguousarray(x)
        return capi.DeviceBuffer(max(x.nbytes, 8)).upload(x)

    d_idx0, d_idx1 = dev(p["idx0"]), dev(p["idx1"])
    tr = pkg.Tracker(max_batch=2, max_keypoints=max(n, 8))
    kf = pkg.KeyframeBuilder(max_batch=1, max_keypoints=max(n, 8), max_tri_points=1024, max_tri_observations=16384)
    frame = dict(d_features_left=dev(p["feat_left"]), d_features_right=dev(p["feat_right"]),
                 d_n_left=dev(np.array([n], np.int32)), d_n_right=dev(np.array([n], np.int32)), d_idx0=d_idx0,
                 d_idx1=d_idx1, cam=p["cam"], window=p["window"], Twc=p["Twc"], next_track_id=p["next_track_id"],
                 track_id=p["track_id"], point_slot=p["point_slot"], points=p["points"], state=p["state"],
                 table=tr.keyframe_table(0, n))
    stream = capi.Stream()
    ar = np.arange(n)
    xl, yl, xr_all, yr_all = p["feat_left"][:, 1], p["feat_left"][:, 2], p["feat_right"][:, 1], p["feat_right"][:, 2]
    held = p["point_slot"] >= 0

    def chain():
        kf.enqueue([frame])
        return kf.fetch()[0]

    def host_composed():
        i0, i1 = d_idx0.download(n, np.int32), d_idx1.download(n, np.int32)
        ok = (i0 >= 0) & (i0 < n)
        j = np.where(ok, i0, 0)
        ok &= i1[j] == ar
        dx, dy = np.abs(xl - xr_all[j]), np.abs(yl - yr_all[j])
        keep = ok & (dx > mn) & (dx < mx) & (dy <= my)
        u_right = np.where(keep, xr_all[j], -1.0)
        with np.errstate(divide="ignore"):
            depth = np.where(keep, bf / (xl - xr_all[j]), -1.0)
        tid = p["track_id"].copy()
        need = tid < 0
        tid[need] = p["next_track_id"] + np.arange(int(need.sum()))
        pos = depth > 0
        d = np.where(pos, depth, 0.0)
        pf = np.stack([(xl - cx) * (1.0 / fx) * d, (yl - cy) * (1.0 / fy) * d, d], 1)
        pts = np.where(pos[:, None], pf @ R.T + t, 0.0)
        pts = np.where(held[:, None], p["points"], pts)
        state = np.where(held, p["state"], np.where(pos, 1, 2)).astype(np.uint8)
        tr.set_keyframe(1, pts, state, tid, stream)
        stream.synchronize()
        return dict(u_right=u_right, depth=depth, track_id=tid, points=pts, state=state)

    rc, rh = chain(), host_composed()
    a0, a1 = tr.debug_keyframe_table(0, n), tr.debug_keyframe_table(1, n)
    assert np.array_equal(a0[1], a1[1]) and np.array_equal(a0[2], a1[2]) and np.abs(a0[0] - a1[0]).max() < 1e-9
    assert np.array_equal(rc["track_id"], rh["track_id"]) and np.array_equal(rc["u_right"], rh["u_right"])
    for _ in range(a.warmup):
        chain()
        host_composed()
    times = {"chain": [], "host_composed": []}
    for _ in range(a.calls):  # alternating: both paths see the same machine
        for name, fn in (("chain", chain), ("host_composed", host_composed)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = dict(keypoints=n, matches=rc["n_matches"], stereo_matches=rc["n_stereo_matches"], new_ids=rc["n_new_ids"],
               new_points=rc["n_new_points"], calls=a.calls, warmup=a.warmup)
    for name, ts in times.items():
        ts = np.array(ts)
        out[name] = dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(np.percentile(ts, 10)), 4),
                         p90_ms=round(float(np.percentile(ts, 90)), 4), min_ms=round(float(ts.min()), 4))
    out["speedup_median"] = round(out["host_composed"]["median_ms"] / out["chain"]["median_ms"], 3)

    # the map side: rspl_map_insert_keyframe over a raw sequence, next to the Python-composed bookkeeping of run()
    base = SY.map_sequence(n_keyframes=8, n_points=600, n_lines=10, seed=1, step=1.0, outlier_frac=0.0)
    ba = pkg.LocalBA(max_poses=16, max_points=2000, max_lines=64, max_edges=20000)
    kf2 = pkg.KeyframeBuilder(max_batch=1, max_keypoints=1024, max_tri_points=1024, max_tri_observations=16384)
    _, reports, _ = SQ.run_raw(SY.raw_sequence(base), ba, kf2)
    _, run_reports = SQ.run(base, ba)
    out["map_insert"] = dict(
        keyframes=len(reports),
        bookkeeping_us=[round(r["bookkeeping_us"], 1) for r in reports],
        triangulation_us=[round(r["triangulation_us"], 1) for r in reports],
        tri_candidates=[r["n_tri_candidates"] for r in reports],
        lines_triangulated=[r["n_lines_triangulated"] for r in reports],
        run_insert_us=[round(r["insert_us"], 1) for r in run_reports])
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
