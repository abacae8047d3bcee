"""RCF edge network timing on the GPU: a stereo pair at 752x480 and at 640x512 in both precisions with the
synthetic weights, per stage from device events on the kernels' stream, beside the same network through
torch's F.conv2d / max_pool2d / conv_transpose2d on the same GPU (the yardstick: a parent commit has no RCF).

    python tools/bench_rcf.py --out profiles/rcf_bench.json

The torch side runs in a child process of its own (`--torch-child`), so only one HIP runtime drives the device
from a process.  "mfma_share" of a stage is the FLOPs of its 3x3 convolutions on MFMA (conv1_1 runs on the
vector ALU and is left out) over the WHOLE stage's time -- pool and side branches included -- over the spec
peak of the precision's MFMA: a lower bound of the conv kernels' own share.
"""
import argparse
import json
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

STAGES = ((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))
UP = ((1, 1, 0), (4, 2, 1), (8, 4, 2), (16, 8, 4), (16, 8, 0))
SIZES = ((480, 752), (512, 640))
PEAK = {"fp32": 157.3e12, "fp16": 2516.6e12}  # spec, v_mfma_f32_32x32x2_f32 / v_mfma_f32_32x32x16_f16


def stage_sizes(H, W):
    out = [(H, W)]
    for _ in range(3):
        H, W = -(-H // 2), -(-W // 2)
        out.append((H, W))
    return out + [(H - 1, W - 1)]


def conv_flops(H, W, B):
    """FLOPs of each stage's 3x3 convolutions on MFMA (2 per multiply-add), conv1_1 left out"""
    out, cin = [], 3
    for s, ((n, c), (h, w)) in enumerate(zip(STAGES, stage_sizes(H, W))):
        f = 0
        for k in range(n):
            if not (s == 0 and k == 0):
                f += 2 * 9 * cin * c * h * w * B
            cin = c
        out.append(f)
    return out


def image(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.clip(np.sin(xx / 5) * np.cos(yy / 7) * 60 + 128 + rng.uniform(-40, 40, (H, W)), 0, 255).astype(np.uint8)


def bench_ours(iters, warmup):
    import rspl_loader
    pkg = rspl_loader.load()
    capi = pkg.capi
    capi.load()
    blob = pkg.weights.ensure_rcf_blob(str(ROOT / "weights"))
    rows = []
    for prec in ("fp32", "fp16"):
        for H, W in SIZES:
            B = 2
            rcf = pkg.RCF(blob, max_height=H, max_width=W, max_batch=B,
                          precision=capi.RSPL_PREC_FP16 if prec == "fp16" else capi.RSPL_PREC_FP32)
            st = capi.Stream()
            imgs = capi.DeviceBuffer(B * H * W).upload(np.stack([image(H, W, b) for b in range(B)]))
            out = capi.DeviceBuffer(B * H * W)

            def run():
                rcf.infer_device(imgs, B, H, W, W, H * W, out, W, H * W, st)

            for _ in range(warmup):
                run()
            st.synchronize()
            t = capi.Timer()
            t.start(st)
            for _ in range(iters):
                run()
            t.stop(st)
            st.synchronize()
            total = t.elapsed_ms() / iters
            rcf.profile(True)
            for _ in range(iters):
                run()
            st.synchronize()
            ms, calls = rcf.stage_times()
            rcf.profile(False)
            stage_ms = [m / calls for m in ms]
            fl = conv_flops(H, W, B)
            edges = out.download((B, H, W), np.uint8)
            rows.append({"precision": prec, "H": H, "W": W, "batch": B, "iters": iters, "ms_per_pair": total,
                         "stage_ms": stage_ms[:5], "tail_ms": stage_ms[5], "conv_gflop": [f / 1e9 for f in fl],
                         "mfma_share": [f / (m * 1e-3) / PEAK[prec] for f, m in zip(fl, stage_ms[:5])],
                         "edge_levels": int(len(np.unique(edges)))})
            print(json.dumps(rows[-1]), flush=True)
            rcf.close()
    return rows


def bench_torch(iters, warmup):
    """The same network, NCHW, on torch's GPU kernels; weights random (the time does not depend on them)."""
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda")
    rows = []
    for prec in ("fp32", "fp16"):
        dt = torch.float16 if prec == "fp16" else torch.float32
        g = torch.Generator(device="cpu").manual_seed(7)
        w = {}
        cin = 3
        for s, (n, c) in enumerate(STAGES, 1):
            for k in range(1, n + 1):
                w[f"c{s}{k}"] = (torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev, dt)
                w[f"b{s}{k}"] = torch.zeros(c).to(dev, dt)
                w[f"d{s}{k}"] = (torch.randn(21, c, 1, 1, generator=g) * 0.01).to(dev, dt)
                w[f"db{s}{k}"] = torch.zeros(21).to(dev, dt)
                cin = c
            w[f"s{s}"] = (torch.randn(1, 21, 1, 1, generator=g) * 0.1).to(dev, dt)
            w[f"sb{s}"] = torch.zeros(1).to(dev, dt)
        w["fuse"], w["fuseb"] = torch.full((1, 5, 1, 1), 0.2).to(dev, dt), torch.zeros(1).to(dev, dt)
        kern = {}
        for size, stride, off in UP[1:]:
            f = (size + 1) // 2
            k1 = 1 - (torch.arange(size, dtype=torch.float64) - (f - 0.5)).abs() / f
            kern[size] = (k1[:, None] * k1[None, :]).to(dev, dt)[None, None]
        for H, W in SIZES:
            B = 2
            x0 = (torch.from_numpy(np.stack([image(H, W, b) for b in range(B)])).to(dev).to(dt) / 255.0 * 2.55)
            x0 = x0[:, None].expand(B, 3, H, W).contiguous()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(7)] for _ in range(iters)]

            def run(marks=None):
                x, so = x0, []
                for s, (n, _) in enumerate(STAGES, 1):
                    if marks:
                        marks[s - 1].record()
                    if s > 1:
                        x = F.max_pool2d(x, 2, stride=1 if s == 5 else 2, ceil_mode=True)
                    d = 2 if s == 5 else 1
                    acc = None
                    for k in range(1, n + 1):
                        x = F.relu(F.conv2d(x, w[f"c{s}{k}"], w[f"b{s}{k}"], padding=d, dilation=d))
                        side = F.conv2d(x, w[f"d{s}{k}"], w[f"db{s}{k}"])
                        acc = side if acc is None else acc + side
                    so.append(F.conv2d(acc, w[f"s{s}"], w[f"sb{s}"]))
                if marks:
                    marks[5].record()
                for i, (size, stride, off) in enumerate(UP):
                    if size > 1:
                        so[i] = F.conv_transpose2d(so[i], kern[size], stride=stride)[:, :, off:off + H, off:off + W]
                fuse = F.conv2d(torch.cat(so, 1), w["fuse"], w["fuseb"])
                p = torch.sigmoid(fuse.float())
                e = (255.0 - p * 255.0).to(torch.uint8)
                if marks:
                    marks[6].record()
                return e

            with torch.no_grad():
                for _ in range(warmup):
                    run()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    run()
                b.record()
                torch.cuda.synchronize()
                total = a.elapsed_time(b) / iters
                for i in range(iters):
                    run(ev[i])
                torch.cuda.synchronize()
            stage = [sum(ev[i][j].elapsed_time(ev[i][j + 1]) for i in range(iters)) / iters for j in range(6)]
            rows.append({"precision": prec, "H": H, "W": W, "batch": B, "iters": iters, "ms_per_pair": total,
                         "stage_ms": stage[:5], "tail_ms": stage[5]})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/rcf_bench.json")
    ap.add_argument("--torch-timeout", type=int, default=300)
    ap.add_argument("--torch-child", action="store_true")
    a = ap.parse_args()
    if a.torch_child:
        print("TORCH_ROWS " + json.dumps(bench_torch(a.iters, a.warmup)), flush=True)
        return
    ours = bench_ours(a.iters, a.warmup)
    result = {"what": "RCF edge network, stereo pair (batch 2), synthetic weights; ms per pair from device events",
              "peak_flops": PEAK, "ours": ours, "torch": None,
              "ratio_to_torch": None}  # torch's time over ours: above 1, ours is faster
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")  # kept even if the torch side does not finish
    try:
        r = subprocess.run([sys.executable, __file__, "--torch-child", "--iters", str(a.iters), "--warmup",
                            str(a.warmup)], capture_output=True, text=True, timeout=a.torch_timeout)
    except subprocess.TimeoutExpired:
        result["torch"] = {"error": f"not finished within {a.torch_timeout} s", "returncode": 124}
        out.write_text(json.dumps(result, indent=1) + "\n")
        sys.exit(124)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("TORCH_ROWS ")]
    if r.returncode != 0 or not line:
        result["torch"] = {"error": (r.stderr or r.stdout)[-2000:], "returncode": r.returncode}
    else:
        th = json.loads(line[0][len("TORCH_ROWS "):])
        result["torch"] = th
        result["ratio_to_torch"] = [
            {"precision": o["precision"], "H": o["H"], "W": o["W"], "total": t["ms_per_pair"] / o["ms_per_pair"],
             "stages": [tm / om for tm, om in zip(t["stage_ms"], o["stage_ms"])], "tail": t["tail_ms"] / o["tail_ms"]}
            for o, t in zip(ours, th)]
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result["ratio_to_torch"]))
    if r.returncode != 0:
        sys.exit(r.returncode)


if __name__ == "__main__":
    main()
