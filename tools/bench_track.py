"""Single-frame latency of the tracking step (MapBuilder::TrackFrame + FramePoseOptimization) on the GPU,
two ways in one process on the same inputs, the calls alternating:

  chain          Tracker.enqueue -> Tracker.fetch: one stream-ordered chain of launches, one sync
  host_composed  what a caller has to write without rspl_track_*: copy SuperGlue's two index arrays to the
                 host, build the correspondences in numpy, PnP.solve (its own sync), the 0.5 m /
                 min_num_match gate, FrameBA.run (its own sync), the write-back in numpy.  The current
                 keypoints' pixels are taken as already on the host (no copy is charged for them).

Wall time per call around work that ends in a device synchronise; warm-up, then the median and the
10th / 90th percentiles over --calls calls of each path.  Both paths must give the same pose."""
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
from rspl_slam_amd import capi, synthetic as SY  # noqa: E402
from rspl_slam_amd.ba_types import FrameProblem, OptimizationConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keypoints", type=int, default=400)
    ap.add_argument("--common", type=int, default=310)  # ~250 valid correspondences after the state filter
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "track_frame.json"))
    a = ap.parse_args()
    if a.calls < 200:
        ap.error("--calls: the median is taken over at least 200 calls")
    n = a.keypoints
    p = SY.track_problem(n0=n, n1=n, n_common=a.common, seed=0)
    cam, last, min_match = p["cam"], p["last_Twc"], 10
    K4 = np.array(cam[:4])
    cfg = OptimizationConfig(mono_point=5.991, stereo_point=7.815)

    def dev(x):
        x = np.ascontiguousarray(x)
        return capi.DeviceBuffer(max(x.nbytes, 8)).upload(x)

    d_feat, d_n1, d_idx0, d_idx1 = dev(p["features"]), dev(np.array([n], np.int32)), dev(p["idx0"]), dev(p["idx1"])
    tr = pkg.Tracker(max_batch=1, max_keypoints=max(n, 8))
    tr.set_keyframe(0, p["points"], p["state"], p["track_id"])
    frame = dict(d_features=d_feat, d_n1=d_n1, d_idx0=d_idx0, d_idx1=d_idx1, cam=cam, last_Twc=last,
                 min_num_match=min_match)
    pnp = pkg.PnP(max_batch=1, max_points=max(n, 8))
    fba = pkg.FrameBA(max_batch=1, max_edges=max(n, 8), max_points=max(n, 8))
    ar = np.arange(n)

    def chain():
        tr.enqueue([frame])
        return tr.fetch()[0]

    def host_composed():
        i0, i1 = d_idx0.download(n, np.int32), d_idx1.download(n, np.int32)
        ok = (i1 >= 0) & (i1 < n)
        j = np.where(ok, i1, 0)
        ok &= i0[j] == ar
        corr = np.flatnonzero(ok & (p["state"][j] == 1))
        X, uv = p["points"][j[corr]], p["features"][corr, 1:3]
        k, R, t, _, _ = pnp.solve([(K4, X, uv)])[0]
        d = t - last[:3, 3]
        if k == 0 or np.sqrt(d @ d) > 0.5 or k < min_match:
            R, t = last[:3, :3], last[:3, 3]
        fp = FrameProblem(cameras=np.array([cam]), pose_q=SY.R_to_quat_xyzw(R), pose_p=t, points=X,
                          mono=dict(lm=np.arange(len(corr)), obs=uv), cfg=cfg)
        r = fba.run([fp])[0]
        inl = np.where(ok, p["track_id"][j], -1)
        if r.n_inliers > min_match:
            inl[corr[r.inlier["mono"] == 0]] = -1
            kept = ok & (inl > 0)
        else:
            kept = ok
        return dict(pose_q=r.pose_q, pose_p=r.pose_p, n_inliers=r.n_inliers, kept=kept)

    rc, rh = chain(), host_composed()
    assert rc["n_inliers"] == rh["n_inliers"] and np.abs(rc["pose_p"] - rh["pose_p"]).max() < 1e-9, (rc, rh)
    assert np.array_equal(rc["kept"], rh["kept"])
    for _ in range(a.warmup):
        chain()
        host_composed()
    times = {"chain": [], "host_composed": []}
    for _ in range(a.calls):  # alternating: both paths see the same machine
        for name, fn in (("chain", chain), ("host_composed", host_composed)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = dict(keypoints=n, valid_correspondences=rc["n_mono"] + rc["n_stereo"], n_inliers=rc["n_inliers"],
               calls=a.calls, warmup=a.warmup)
    for name, ts in times.items():
        ts = np.array(ts)
        out[name] = dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(np.percentile(ts, 10)), 4),
                         p90_ms=round(float(np.percentile(ts, 90)), 4), min_ms=round(float(ts.min()), 4))
    out["speedup_median"] = round(out["host_composed"]["median_ms"] / out["chain"]["median_ms"], 3)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
