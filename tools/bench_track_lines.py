"""Single-frame latency of the tracking step with its line side and keyframe decision, three ways in one
process on the same inputs, the calls alternating:

  ext            Tracker.enqueue with d_lines / keyframe -> Tracker.fetch (rspl_track_enqueue_ext /
                 rspl_track_fetch_ext): the chain plus one launch, one sync
  host_composed  what a caller wrote before: the plain chain (enqueue -> fetch), then LineMatcher.assign_csr for
                 the frame's lines (host arrays, its own sync), LineMatcher.MatchLines from the fetched match_kf
                 against the keyframe's CSR (computed once per keyframe, outside the timing; its own sync), the
                 id copy and the AddKeyframe decision in numpy.  The frame's lines and keypoints are taken as
                 already on the host (no copy is charged for them).
  plain          the plain chain alone: what the added launch costs is ext - plain

Wall time per call around work that ends in a device synchronise; warm-up, then the median and the 10th / 90th
percentiles over --calls calls of each path.  ext and host_composed must give the same lines and decision."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import rspl_loader  # noqa: E402

pkg = rspl_loader.load()
pkg.capi.load()
from rspl_slam_amd import capi  # noqa: E402
import track_lines_cases as TC  # noqa: E402  (the seeded scene the GPU tests use)
import track_lines_ref as TLR  # noqa: E402   (the numpy id copy and decision a caller would write)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keypoints", type=int, default=400)
    ap.add_argument("--lines", type=int, default=60)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "track_lines.json"))
    a = ap.parse_args()
    if a.calls < 200:
        ap.error("--calls: the median is taken over at least 200 calls")
    n, nl = a.keypoints, a.lines
    c = TC.line_case(nl, n)

    def dev(x):
        x = np.ascontiguousarray(x)
        return capi.DeviceBuffer(max(x.nbytes, 8)).upload(x)

    d_feat, d_n1, d_idx0, d_idx1 = dev(c["features"]), dev(np.array([n], np.int32)), dev(c["idx0"]), dev(c["idx1"])
    d_lines, d_kf_lines, d_kf_feat, d_n0 = dev(c["lines"]), dev(c["kf_lines"]), dev(c["kf_features"]), dev(np.array([n], np.int32))
    tr = pkg.Tracker(max_batch=1, max_keypoints=max(n, 8))
    tr.enable_lines(max_lines=max(nl, 1), max_pairs=65536)
    tr.set_keyframe(0, c["points"], c["state"], c["track_id"])
    tr.set_keyframe_lines(0, nl, d_kf_lines, d_kf_feat, d_n0, c["kf_line_track_id"], c["kf_line_slot"])
    plain_frame = dict(d_features=d_feat, d_n1=d_n1, d_idx0=d_idx0, d_idx1=d_idx1, cam=c["cam"], last_Twc=c["last_Twc"])
    ext_frame = dict(plain_frame, d_lines=d_lines, n_lines=nl, frame_id=c["frame_id"],
                     keyframe=dict(Twc=c["kf_Twc"], frame_id=c["kf_frame_id"]))
    lm = pkg.lines.LineMatcher(max_lines=max(nl, 1), max_points=max(n, 8), max_pairs=65536, max_matches=max(n, 8))
    kf_csr = lm.assign_csr(c["kf_lines"], c["kf_features"])  # once per keyframe

    def ext():
        tr.enqueue([ext_frame])
        return tr.fetch()[0]

    def plain():
        tr.enqueue([plain_frame])
        return tr.fetch()[0]

    def host_composed():
        r = plain()
        csr = lm.assign_csr(c["lines"], c["features"])
        line_matches = lm.MatchLines(kf_csr, csr, TLR.point_matches(r["match_kf"]), n, n)
        mk, tid, slot = TLR.id_copy(line_matches, c["kf_line_track_id"], c["kf_line_slot"], nl)
        r.update(TLR.decision_q(r["pose_q"], r["pose_p"], r["n_inliers"], c["kf_Twc"], c["kf_frame_id"], c["frame_id"]),
                 line_match_kf=mk, line_track_id=tid, line_slot=slot)
        return r

    re, rh = ext(), host_composed()
    for k in ("line_match_kf", "line_track_id", "line_slot", "add_keyframe", "tracked_well", "pose_p", "track_id"):
        assert np.array_equal(re[k], rh[k]), k
    assert abs(re["delta_angle"] - rh["delta_angle"]) < 1e-12 and abs(re["delta_distance"] - rh["delta_distance"]) < 1e-12
    paths = (("ext", ext), ("host_composed", host_composed), ("plain", plain))
    for _ in range(a.warmup):
        for _, fn in paths:
            fn()
    times = {name: [] for name, _ in paths}
    for _ in range(a.calls):  # alternating: the paths see the same machine
        for name, fn in paths:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = dict(keypoints=n, lines=nl, n_inliers=re["n_inliers"], n_line_matches=re["n_line_matches"],
               n_line_tracks=re["n_line_tracks"], calls=a.calls, warmup=a.warmup)
    for name, ts in times.items():
        ts = np.array(ts)
        out[name] = dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(np.percentile(ts, 10)), 4),
                         p90_ms=round(float(np.percentile(ts, 90)), 4), min_ms=round(float(ts.min()), 4))
    out["speedup_median"] = round(out["host_composed"]["median_ms"] / out["ext"]["median_ms"], 3)
    out["added_launch_median_ms"] = round(out["ext"]["median_ms"] - out["plain"]["median_ms"], 4)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
