"""Times the training step of the BN-folded SlimYOLOv2 on the GPU (yolo355.train.SlimTrainer.step: forward, loss, backward, SGD)
on synthetic device batches, and beside it, in the same process and alternating with it, what a user would otherwise run: the
same ten-layer stack as torch.nn modules with the yolo355.grad criterion and torch.optim.SGD, in fp32 and under bf16 autocast:

    python -m yolo355.tools.train_bench [--config 32x240x320 64x416x416 --classes 20 --reps 30 --out FILE]
    python -m yolo355.tools.train_bench --only-ours --reps 5       # the run rocprofv3 --kernel-trace --stats wraps

After two warm-up rounds: the median over --reps repetitions of the wall clock around one call that ends synchronised.  The
convolution work of a step is counted as the forward's multiply-adds, once for the forward, once for the weight gradients and
once for the data gradients less conv1's (the image gets none), and set against the nominal dense bf16 MFMA peak.  Prints one
JSON line per configuration; --out writes them as a list."""
import argparse
import json
import statistics
import time

import torch

PEAK_BF16_TFLOPS = 2500.0            # nominal dense bf16 MFMA peak of one MI355X
CONVS = [(3, 16, 1), (16, 32, 2), (32, 64, 4), (64, 64, 4), (64, 128, 8), (128, 128, 8), (128, 256, 16), (256, 256, 16), (256, 256, 16)]


def step_macs(h, w, pred_channels):
    """multiply-adds of one image: (forward, the whole step)"""
    per = [cin * cout * 9 * (h // d) * (w // d) for cin, cout, d in CONVS + [(256, pred_channels, 16)]]
    fwd = sum(per)
    return fwd, 3 * fwd - per[0]


def torch_stack(pred_channels, device):
    import torch.nn as nn
    layers = []
    for i, (cin, cout, _) in enumerate(CONVS):
        layers += [nn.Conv2d(cin, cout, 3, 1, 1), nn.LeakyReLU(0.125)]
        if i in (0, 1, 3, 5):
            layers.append(nn.MaxPool2d(2, 2))
    layers.append(nn.Conv2d(256, pred_channels, 3, 1, 1))
    return nn.Sequential(*layers).to(device)


def run(cfg, a):
    from yolo355 import synth
    from yolo355.grad import YoloCriterion
    from yolo355.tools.grad_bench import bench_labels
    from yolo355.train import SlimTrainer
    B, H, W = cfg
    A, C = 5, a.classes
    ch = A * (5 + C)
    labels, counts = bench_labels(B, 2.4, C)
    ws = [(w, b) for _, w, b in synth.make_weights(5, num_classes=C, weight_gain=2.0)]
    t = SlimTrainer([H, W], C, synth.ANCHOR_SIZE, B, a.lr)
    t.load_weights(ws)
    x = torch.from_numpy(synth.make_images(9, B, H, W, "noise")).to(t.device)
    res = dict(batch=B, height=H, width=W, classes=C, reps=a.reps, lr=a.lr)
    nets = {}
    if not a.only_ours:
        crit = YoloCriterion([H, W], 16, synth.ANCHOR_SIZE, C, max_batch=B, max_labels_per_image=max(1, int(counts.max())))
        for mode in ("fp32", "bf16_autocast"):
            net = torch_stack(ch, t.device)
            with torch.no_grad():
                convs = [m for m in net if isinstance(m, torch.nn.Conv2d)]
                for m, (w, b) in zip(convs, ws):
                    m.weight.copy_(torch.from_numpy(w))
                    m.bias.copy_(torch.from_numpy(b))
            nets[mode] = (net, torch.optim.SGD(net.parameters(), lr=a.lr, momentum=0.9, weight_decay=5e-4))
        crit.handle.set_labels(labels)

    def torch_step(mode):
        net, opt = nets[mode]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=(mode == "bf16_autocast")):
            p = net(x)
        out = crit([p.float()])
        opt.zero_grad(set_to_none=True)
        out[3].backward()
        opt.step()
        return float(out[3].detach())

    times = {k: [] for k in ["ours"] + list(nets)}
    first = {}
    t.criterion().set_labels(labels)
    for rep in range(a.reps + 2):                                           # two warm-up rounds
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = t.step(x)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        first.setdefault("ours", float(out[3]))
        if rep >= 2:
            times["ours"].append(dt)
        for mode in nets:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = torch_step(mode)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            first.setdefault(mode, v)
            if rep >= 2:
                times[mode].append(dt)
    fwd, step = step_macs(H, W, ch)
    ms = 1e3 * statistics.median(times["ours"])
    res.update(step_ms=ms, images_per_s=B / (ms * 1e-3), forward_gmac_per_image=fwd * 1e-9, step_gmac_per_image=step * 1e-9,
               step_tflops=2.0 * step * B / (ms * 1e-3) * 1e-12, fraction_of_bf16_peak=2.0 * step * B / (ms * 1e-3) * 1e-12 / PEAK_BF16_TFLOPS,
               first_total_loss=first["ours"])
    for mode in nets:
        res["torch_%s_step_ms" % mode] = 1e3 * statistics.median(times[mode])
        res["torch_%s_first_total_loss" % mode] = first[mode]
    t.close()
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["32x240x320", "64x416x416"], help="BxHxW")
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--only-ours", action="store_true", help="leave the torch steps out (a kernel trace of the library alone)")
    ap.add_argument("--out", default=None, help="write the results as a JSON list")
    a = ap.parse_args(argv)
    res = [run(tuple(int(v) for v in c.split("x")), a) for c in a.config]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
