"""Times yolo355.convgrad.conv2d, forward + backward (dx, dw, db; the first layer without dx), on the thirteen convolutions of
YOLOv3tiny at a batch of device tensors, and beside it, in the same process and alternating with it, torch.nn.functional.conv2d
in fp32 and under bf16 autocast on the same tensors:

    python -m yolo355.tools.convgrad_bench [--config 32x416x416 --classes 20 --reps 10 --out FILE]

After two warm-up rounds: the median over --reps repetitions of the wall clock around one forward + backward that ends
synchronised.  Prints one JSON line per layer and one for the sum; --out writes them as a list.  Nobody asserts these figures:
the kernels are the straightforward form (no LDS staging), recorded so that a later change has something to compare with."""
import argparse
import json
import statistics
import time

import torch
import torch.nn.functional as F


def tiny_v3_layers(classes, H, W):
    """(name, cin, cout, k, map height, map width) of YOLOv3tiny's convolutions (backbone.darknet.darknet_light, models.tiny_yolo_v3)"""
    pred = 3 * (5 + classes)
    d = lambda s: (H // s, W // s)
    return [("conv_1", 3, 16, 3) + d(1), ("conv_2", 16, 32, 3) + d(2), ("conv_3", 32, 64, 3) + d(4), ("conv_4", 64, 128, 3) + d(8),
            ("conv_5", 128, 256, 3) + d(16), ("conv_6", 256, 512, 3) + d(32), ("conv_7", 512, 1024, 3) + d(32),
            ("conv_set_2", 1024, 256, 3) + d(32), ("conv_1x1_2", 256, 128, 1) + d(32), ("conv_set_1", 384, 256, 3) + d(16),
            ("extra_conv_2", 256, 512, 3) + d(32), ("pred_2", 512, pred, 1) + d(32), ("pred_1", 256, pred, 1) + d(16)]


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_layer(layer, B, reps, device):
    from yolo355 import convgrad
    name, cin, cout, k, h, w = layer
    first = cin == 3
    gen = torch.Generator(device=device).manual_seed(7)
    rnd = lambda *shape: torch.rand(shape, generator=gen, device=device) * 2.0 - 1.0
    x = rnd(B, cin, h, w).requires_grad_(not first)
    wt = (rnd(cout, cin, k, k) * float((cin * k * k) ** -0.5)).requires_grad_(True)
    b = rnd(cout).requires_grad_(True)
    dy = rnd(B, cout, h, w)
    leaves = [t for t in (x, wt, b) if t.requires_grad]

    def step(conv):
        for t in leaves:
            t.grad = None
        conv().backward(dy)

    def autocast():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return F.conv2d(x, wt, b, 1, k // 2).float()
    fns = {"yolo355": lambda: convgrad.conv2d(x, wt, b, 1, k // 2), "torch_fp32": lambda: F.conv2d(x, wt, b, 1, k // 2), "torch_bf16_autocast": autocast}
    times = {n: [] for n in fns}
    for rep in range(reps + 2):                                              # two warm-up rounds
        for n, fn in fns.items():
            dt = _timed(lambda: step(fn))
            if rep >= 2:
                times[n].append(dt)
    res = dict(layer=name, cin=cin, cout=cout, kernel=k, batch=B, height=h, width=w, reps=reps)
    for n in fns:
        res[n + "_fwd_bwd_ms"] = 1e3 * statistics.median(times[n])
    res["ratio_yolo355_over_torch_fp32"] = res["yolo355_fwd_bwd_ms"] / res["torch_fp32_fwd_bwd_ms"]
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="32x416x416", help="BxHxW")
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="write the results as a JSON list")
    a = ap.parse_args(argv)
    B, H, W = (int(v) for v in a.config.split("x"))
    device = torch.device("cuda", torch.cuda.current_device())
    res = [run_layer(l, B, a.reps, device) for l in tiny_v3_layers(a.classes, H, W)]
    total = dict(layer="sum", batch=B, height=H, width=W, reps=a.reps)
    for n in ("yolo355", "torch_fp32", "torch_bf16_autocast"):
        total[n + "_fwd_bwd_ms"] = sum(r[n + "_fwd_bwd_ms"] for r in res)
    total["ratio_yolo355_over_torch_fp32"] = total["yolo355_fwd_bwd_ms"] / total["torch_fp32_fwd_bwd_ms"]
    print(json.dumps(total), flush=True)
    res.append(total)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
