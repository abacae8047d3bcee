"""The RCF edge network restated with torch.nn.functional on the CPU, from the layer table alone (the public
VGG16-based RCF, yun-liu/RCF-PyTorch; the reference ships only its engine's path, src/rcf.cpp).

  input   one gray u8 image as raw floats 0..255, replicated into 3 channels, no scaling
  stage s 3x3 convs conv{s}_{k} with bias and ReLU: 2, 2, 3, 3, 3 of them with 64, 128, 256, 512, 512 channels;
          pad 1 in stages 1..4, pad 2 and dilation 2 in stage 5; before stages 2..4 max_pool2d(2, stride 2,
          ceil_mode), before stage 5 max_pool2d(2, stride 1, ceil_mode)
  side    every conv's ReLU output through conv{s}_{k}_down (1x1, C -> 21, bias), the maps of a stage summed,
          score_dsn{s} (1x1, 21 -> 1, bias) gives so_s
  up      so_2..5 through conv_transpose2d with fixed bilinear kernels of size 4 / 8 / 16 / 16 and stride
          2 / 4 / 8 / 8, cropped to H x W from offset 1 / 2 / 4 / 0
  out     fuse = score_fuse(cat(so_1..5)); six maps sigmoid(so_1..5), sigmoid(fuse)
  edge    (uint8)(unsigned)(255.0f - p * 255.0f) in float arithmetic

``fp16=True`` is the restatement of RSPL_PREC_FP16: the 3x3 and the _down weights and every conv's stored ReLU
output rounded to fp16 (conv1_1's three input channels summed in float32 first, then rounded, and convolved
with the one gray channel), products accumulated in ``dtype``; biases, the side sums, score_dsn, score_fuse
and the tail stay in ``dtype``.
"""
import functools

import numpy as np

STAGES = ((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))
UP = ((1, 1, 0), (4, 2, 1), (8, 4, 2), (16, 8, 4), (16, 8, 0))  # (kernel size, stride, crop offset) of so_1..5


def bilinear_kernel(size):
    f = (size + 1) // 2
    c = f - 1 if size % 2 == 1 else f - 0.5
    i = np.arange(size, dtype=np.float64)
    k = 1 - np.abs(i - c) / f
    return k[:, None] * k[None, :]


def stage_sizes(H, W):
    """(Hs, Ws) of stages 1..5: the pools' ceil_mode arithmetic, without running the network"""
    out = [(H, W)]
    for _ in range(3):
        H, W = -(-H // 2), -(-W // 2)
        out.append((H, W))
    out.append((H - 1, W - 1))
    return out


def forward(weights, image, dtype="float64", fp16=False):
    """weights: name -> array (weights.rcf_shapes); image [H, W] u8.  Returns {"logits": [6, H, W] (so_1..5
    upsampled and cropped, fuse), "stage_shapes": the so_s shapes before upsampling, "up_shapes": after it and
    before the crop} with the logits in ``dtype``."""
    import torch
    import torch.nn.functional as F
    dt = getattr(torch, dtype)
    torch.set_num_threads(min(8, torch.get_num_threads()))

    def t(name):
        return torch.from_numpy(np.ascontiguousarray(weights[name])).to(dt)

    def h(x):  # rounded to fp16, carried on in dt
        return x.to(torch.float16).to(dt) if fp16 else x

    H, W = image.shape
    x = torch.from_numpy(np.ascontiguousarray(image)).to(dt)[None, None]
    if not fp16:
        x = x.expand(1, 3, H, W).contiguous()
    so, stage_shapes, up_shapes = [], [], []
    with torch.no_grad():
        for s, (n, _) in enumerate(STAGES, 1):
            if s > 1:
                x = F.max_pool2d(x, 2, stride=1 if s == 5 else 2, ceil_mode=True)
            d = 2 if s == 5 else 1
            acc = None
            for k in range(1, n + 1):
                w = t(f"conv{s}_{k}.weight")
                if fp16 and s == 1 and k == 1:
                    w = torch.from_numpy(np.ascontiguousarray(weights["conv1_1.weight"])).to(torch.float32)
                    w = w.sum(1, keepdim=True).to(dt)
                x = h(F.relu(F.conv2d(x, h(w), t(f"conv{s}_{k}.bias"), padding=d, dilation=d)))
                side = F.conv2d(x, h(t(f"conv{s}_{k}_down.weight")), t(f"conv{s}_{k}_down.bias"))
                acc = side if acc is None else acc + side
            o = F.conv2d(acc, t(f"score_dsn{s}.weight"), t(f"score_dsn{s}.bias"))
            stage_shapes.append(tuple(o.shape[2:]))
            size, stride, off = UP[s - 1]
            if size > 1:
                kern = torch.from_numpy(bilinear_kernel(size)).to(dt)[None, None]
                o = F.conv_transpose2d(o, kern, stride=stride)
                up_shapes.append(tuple(o.shape[2:]))
                assert off + H <= o.shape[2] and off + W <= o.shape[3], (s, o.shape, H, W)
                o = o[:, :, off:off + H, off:off + W]
            else:
                up_shapes.append(tuple(o.shape[2:]))
            so.append(o)
        fuse = F.conv2d(torch.cat(so, 1), t("score_fuse.weight"), t("score_fuse.bias"))
        logits = torch.cat(so + [fuse], 1)[0]
    return {"logits": logits.numpy(), "stage_shapes": stage_shapes, "up_shapes": up_shapes}


def edge_image(logit):
    """process_output's conversion of one logit map: the sigmoid in the logits' own dtype, then float32"""
    l = np.asarray(logit)
    p = (1.0 / (1.0 + np.exp(-l.astype(np.float64 if l.dtype == np.float64 else np.float32)))).astype(np.float32)
    return (np.float32(255.0) - p * np.float32(255.0)).astype(np.uint32).astype(np.uint8)


def test_image(H, W, seed=0):
    """clip(sin(x / 5) cos(y / 7) 60 + 128 + U[-40, 40)): texture with both smooth ramps and noise"""
    rng = np.random.default_rng(1000 * H + W + seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    v = np.sin(xx / 5) * np.cos(yy / 7) * 60 + 128 + rng.uniform(-40, 40, (H, W))
    return np.clip(v, 0, 255).astype(np.uint8)


test_image.__test__ = False  # (not a pytest case)


@functools.lru_cache(maxsize=None)
def synth_weights(seed=7):
    from rspl_slam_amd import weights as WT
    return WT.rcf_synth(seed)


# forward() needs torch, which must not meet librspl's HIP runtime in the test process (one HIP runtime per
# process): the tests get its results from a child process, one per pytest process, shared by every test.
VARIANTS = (("float64", False), ("float32", False), ("float32", True), ("float64", True))


def _key(H, W, seed, dtype, fp16):
    return f"{H}x{W}s{seed}_{dtype}_{'h' if fp16 else 'f'}"


def _child(out, mode, cases):
    import rspl_loader
    rspl_loader.load()
    res = {}
    for H, W, seed in cases:
        im = test_image(H, W, seed)
        if mode == "refs":
            for dtype, fp16 in VARIANTS:
                res[_key(H, W, seed, dtype, fp16)] = forward(synth_weights(), im, dtype, fp16)["logits"]
        else:  # "shapes"
            r = forward(synth_weights(), im, "float32")
            res[f"{H}x{W}_logits"] = np.array(r["logits"].shape + (int(np.all(np.isfinite(r["logits"]))),))
            res[f"{H}x{W}_stage"] = np.array(r["stage_shapes"])
            res[f"{H}x{W}_up"] = np.array(r["up_shapes"])
    np.savez(out, **res)


def run_child(mode, cases):
    """{name: array} of forward() on `cases` [(H, W, seed)], computed in a child process"""
    import pathlib
    import subprocess
    import sys
    import tempfile
    root = pathlib.Path(__file__).resolve().parents[1]
    with tempfile.TemporaryDirectory() as d:
        out = pathlib.Path(d) / "out.npz"
        subprocess.run([sys.executable, __file__, str(root), str(out), mode] + [f"{h},{w},{s}" for h, w, s in cases],
                       check=True, timeout=300)
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _references():
    from rcf_cases import ALL
    return run_child("refs", ALL)


def reference(H, W, dtype="float64", fp16=False, seed=0):
    """The logits [6, H, W] of test_image(H, W, seed) (a case of rcf_cases.ALL) under the synthetic weights"""
    return {"logits": _references()[_key(H, W, seed, dtype, fp16)]}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, sys.argv[1])
    _child(sys.argv[2], sys.argv[3], [tuple(int(v) for v in c.split(",")) for c in sys.argv[4:]])
