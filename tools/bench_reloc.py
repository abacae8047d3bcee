"""Time the global descriptor search (rspl_lmap_global_enqueue: pack | search | merge, three launches) on one frame
at 400 / 3600, 600 / 5400 and 2048 / 18432 keypoints / candidates (tools/bench_lmap.py's three shapes) and at
400 / 65536, the full bank.  No earlier commit has this stage, so there is no parent time; two yardsticks on the
same inputs instead:

  1. tests/reloc_ref.py on one CPU core.  The restatement walks the keypoints one by one, so it is timed on the first
     `--cpu-keypoints` of them and scaled to the frame (both numbers are recorded).
  2. the same computation through torch on the same GPU: fp64 D = 2 (1 - Q @ B.T), topk(2, largest=False) per row,
     argmin per column -- run in a child process (one HIP runtime per process), timed the same way.

Times are HIP events around `--calls` back-to-back enqueues on one stream after `--warmup` calls, median of
`--repeats` windows, p10-p90 kept.  A handle takes one enqueue at a time, so the calls rotate over a ring of handles
and a handle is fetched just before it is reused.  Also reported: algorithmic FLOP/s (2 * 256 * keypoints *
candidates per launch) and the bank bytes one launch reads at least once.

  python tools/bench_reloc.py --out profiles/reloc_bench.json
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SHAPES = dict(C3=(400, 3600), C4=(600, 5400), C5=(2048, 18432), full_bank=(400, 65536))


def scene(n1, nl, seed):
    """a random unit bank; 75 % of the keypoints a noisy copy, at distance U(0.02, 0.5), of a distinct bank row"""
    import lmap_cases as LC
    import reloc_cases as RC
    rng = np.random.default_rng(seed)
    bank = LC.unit(rng, nl)
    rows = rng.permutation(nl)
    q = LC.unit(rng, n1)
    for i in range(n1):
        if rng.uniform() < 0.75:
            q[i] = LC.at_distance(bank[rows[i]], rng.uniform(0.02, 0.5), rng)
    return RC.records(q, rng), RC.table(bank, rng, first_id=1)


def pct(t, p):
    return float(np.percentile(np.asarray(t), p))


def torch_child(name, calls, warmup, repeats):
    import torch
    n1, nl = SHAPES[name]
    F, lm = scene(n1, nl, 3000 + list(SHAPES).index(name))
    Q = torch.tensor(F[:, 3:], dtype=torch.float64, device="cuda")
    Bk = torch.tensor(lm["desc"], dtype=torch.float64, device="cuda")

    def run():
        D = 2.0 * (1.0 - Q @ Bk.T)
        v, i = D.topk(2, dim=1, largest=False)
        return v, i, D.argmin(dim=0)

    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            run()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3 / calls)
    v, i, k = run()
    print(json.dumps(dict(us=statistics.median(t), p10=pct(t, 10), p90=pct(t, 90), arg=i[:, 0].cpu().tolist(),
                          kbest=k.cpu().tolist())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--cpu-keypoints", type=int, default=16)
    ap.add_argument("--torch-calls", type=int, default=20)
    ap.add_argument("--torch-child", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "reloc_bench.json"))
    args = ap.parse_args()
    if args.torch_child:
        return torch_child(args.torch_child, args.torch_calls, 3, args.repeats)

    import rspl_loader
    pkg = rspl_loader.load()
    from rspl_slam_amd import capi
    import reloc_ref as RR
    if capi.device_count() < 1:
        raise SystemExit("bench_reloc: no HIP device")
    lib = capi.load()
    stream, timer = capi.Stream(), capi.Timer()
    rows = {}
    for name in args.shapes.split(","):
        n1, nl = SHAPES[name]
        F, lm = scene(n1, nl, 3000 + list(SHAPES).index(name))
        nc = min(args.cpu_keypoints, n1)
        t0 = time.perf_counter()
        RR.search(F[:nc], lm)
        cpu_part_ms = (time.perf_counter() - t0) * 1e3
        cpu_ms = cpu_part_ms * n1 / nc
        d = dict(d_features=capi.DeviceBuffer(F.nbytes).upload(F),
                 d_n1=capi.DeviceBuffer(8).upload(np.array([n1], np.int32)))
        ring = []
        for _ in range(args.ring):
            h = pkg.LocalMap(max_bank_points=nl, max_local_points=nl, max_keypoints=n1, max_batch=1)
            h.store_host(lm["ids"], lm["desc"])
            h.set_local(lm["ids"], lm["pos"], stream)
            ring.append(h)
        busy, calls = [False] * args.ring, [0]

        def enqueue():
            k = calls[0] % args.ring
            if busy[k]:
                ring[k].global_fetch()
            ring[k].global_enqueue([d], stream=stream)
            busy[k] = True
            calls[0] += 1

        enqueue()
        got = ring[0].global_fetch()[0]
        busy[0] = False
        # the timed configuration decides what the host twin decides (the large shapes: on the first 64 keypoints)
        nh = n1 if n1 * nl <= 4e6 else 64
        want = pkg.lmap_global_host(F[:nh], lm["ids"], lm["pos"], lm["desc"])
        same = bool(np.array_equal(got["arg"][:nh], want["arg"]))
        if nh == n1:
            same = same and all(np.array_equal(got[k], want[k]) for k in ("match", "kbest", "match_kp", "match_id"))
        dmax = float(max(np.abs(got["best"][:nh] - want["best"]).max(), np.abs(got["second"][:nh] - want["second"]).max()))
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
                ring[k].global_fetch()
        del ring
        us = statistics.median(t)
        child = subprocess.run([sys.executable, __file__, "--torch-child", name, "--torch-calls", str(args.torch_calls),
                                "--repeats", str(args.repeats)], capture_output=True, text=True, timeout=300)
        tor = None
        if child.returncode == 0 and child.stdout.strip():
            tj = json.loads(child.stdout.strip().splitlines()[-1])
            tor = dict(us=round(tj["us"], 1), us_p10_p90=[round(tj["p10"], 1), round(tj["p90"], 1)],
                       same_arg_as_device=bool(np.array_equal(np.array(tj["arg"]), got["arg"])),
                       same_kbest_as_device=bool(np.array_equal(np.array(tj["kbest"]), got["kbest"])),
                       ratio_torch_over_fused=round(tj["us"] / us, 2))
        else:
            tor = dict(error=(child.stderr or "no output")[-400:])
        c, q, ks = pkg.lmap_global_plan(n1, nl)
        flop = 2.0 * 256 * n1 * nl
        rows[name] = dict(keypoints=n1, candidates=nl, plan=dict(chunk_rows=c, qtile_rows=q, k_slab=ks),
                          enqueue_us=round(us, 1), enqueue_us_p10_p90=[round(pct(t, 10), 1), round(pct(t, 90), 1)],
                          algorithmic_tflops=round(flop / us * 1e-6, 2), bank_mbytes_per_launch=round(nl * 2048 / 1e6, 1),
                          n_pass=int(got["n_pass"]), n_matched=int(got["n_matched"]),
                          decisions_equal_host_twin=same, host_twin_keypoints_checked=nh,
                          max_abs_diff_best_second=float(f"{dmax:.3g}"),
                          cpu_restatement_ms=round(cpu_ms, 1), cpu_restatement_timed_keypoints=nc,
                          cpu_restatement_timed_ms=round(cpu_part_ms, 1),
                          speedup_vs_one_core=round(cpu_ms * 1e3 / us, 1), torch_fp64_chain=tor)
        print(f"{name}: {us:.1f} us per enqueue, {flop / us * 1e-6:.2f} TFLOP/s; torch chain {tor.get('us')} us; "
              f"restatement on one core {cpu_ms:.0f} ms; decisions equal the host twin: {same}", flush=True)
    res = dict(what="HIP events around back-to-back rspl_lmap_global_enqueue calls on one stream, one frame per call, "
                    "median of windows with p10-p90; yardsticks: tests/reloc_ref.py on one core (timed on a few "
                    "keypoints, scaled) and the torch fp64 matmul | topk(2) | argmin chain on the same GPU",
               calls=args.calls, warmup=args.warmup, repeats=args.repeats, ring=args.ring, torch_calls=args.torch_calls,
               version=lib.rspl_version().decode(), shapes=rows)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
