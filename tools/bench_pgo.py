"""Time the whole pose-graph solve (rspl_pgo_solve: plan, uploads, every LM trial, the poses back) on ring graphs of
256, 1024 and 4096 poses: edges to the next 4 keyframes, three loop edges, noisy measurements (sigma_t 0.02 m,
sigma_r 0.01 rad), initial poses from integrated odometry with 1 % drift (tests/pgo_cases.py).  No earlier commit has
this stage, so there is no parent time.  The yardstick is tests/pgo_ref.py's sparse path -- the same LM rule with
scipy.sparse's direct solver -- in a child process pinned to one core; its time inside the sparse solves alone is kept
too, since the rest of it is per-edge Python.

The device time is wall time around PoseGraph.solve, median of `--repeats` calls after one warm-up call; the host
twin (rspl_pgo_debug_host, one core, plain C++ tiles) is timed once beside it.  Launches per trial follow from the
plan: one assemble, three per tile column that has tiles below its diagonal (one otherwise), one substitution, two
for the trial.  No hardware counters are read and no roofline fraction is claimed.

  python tools/bench_pgo.py --out profiles/pgo_bench.json
"""
import argparse
import json
import os
import pathlib
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SIZES = (256, 1024, 4096)


def graph(n):
    import pgo_cases as PC
    loops = [(n - 1 - 7 * k, 1 + 5 * k) for k in range(3)]
    return PC.build(n, 4, 100 + n, True, loops=loops)


def cpu_child(n):
    """pgo_ref's sparse solve on one core: one JSON line"""
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    import pgo_cases as PC
    import pgo_ref
    c = graph(n)
    P = pgo_ref.Problem(*PC.args(c))
    inner, t_solve = pgo_ref._solve, [0.0]

    def timed(*a):
        t0 = time.perf_counter()
        r = inner(*a)
        t_solve[0] += time.perf_counter() - t0
        return r

    pgo_ref._solve = timed
    t0 = time.perf_counter()
    R = pgo_ref.solve(P, sparse=True)
    t = time.perf_counter() - t0
    print(json.dumps(dict(seconds=t, seconds_in_sparse_solves=t_solve[0], iterations=R.iterations, trials=R.trials,
                          status=R.status, cost_initial=R.cost_initial, cost_final=R.cost_final)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pgo_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--cpu-child", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if a.cpu_child:
        return cpu_child(a.cpu_child)
    import rspl_loader
    pkg = rspl_loader.load()
    import pgo_cases as PC
    rows = []
    for n in a.sizes:
        c = graph(n)
        plan = pkg.pgo_plan(c["pose_fixed"], c["edge_i"], c["edge_j"], tile_map=True)
        tm = plan["tile_map"]
        below = [(tm[k + 1:, k] >= 0).any() for k in range(plan["tiles_per_side"])]
        launches = 1 + sum(3 if b else 1 for b in below) + 1 + 2
        h = pkg.PoseGraph(max_poses=n, max_edges=len(c["edge_i"]), max_tiles=plan["n_filled_tiles"])
        out = h.solve(*PC.args(c))  # warm-up
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = h.solve(*PC.args(c))
            ts.append(time.perf_counter() - t0)
        h.close()
        t0 = time.perf_counter()
        twin = pkg.pgo_host(*PC.args(c))
        t_twin = time.perf_counter() - t0
        row = dict(n_poses=n, n_edges=int(len(c["edge_i"])), n_tiles=plan["n_tiles"],
                   n_filled_tiles=plan["n_filled_tiles"], tile_bytes=plan["n_filled_tiles"] * 96 * 96 * 8,
                   launches_per_trial=launches,
                   device=dict(seconds_median=statistics.median(ts), seconds_min=min(ts), seconds_max=max(ts),
                               repeats=a.repeats, iterations=out["iterations"], trials=out["trials"],
                               status=out["status"], cost_initial=out["cost_initial"], cost_final=out["cost_final"],
                               seconds_per_trial=statistics.median(ts) / max(out["trials"], 1)),
                   host_twin=dict(seconds=t_twin, iterations=twin["iterations"], trials=twin["trials"],
                                  cost_final=twin["cost_final"]))
        if not a.no_cpu:
            r = subprocess.run([sys.executable, __file__, "--cpu-child", str(n)], capture_output=True, text=True,
                               check=True)
            row["pgo_ref_sparse_one_core"] = json.loads(r.stdout.strip().splitlines()[-1])
            row["pgo_ref_seconds_over_device_seconds"] = row["pgo_ref_sparse_one_core"]["seconds"] / row["device"]["seconds_median"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    doc = dict(what="whole pose-graph solve, ring graphs, span 4, three loop edges, noisy (tools/bench_pgo.py)",
               not_measured="per-kernel times, hardware counters; no roofline fraction is claimed", rows=rows)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
