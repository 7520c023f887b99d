"""Times the training step of the BatchNorm SlimYOLOv2 on the GPU (yolo355.bntrain.SlimBNTrainer.step: forward in training mode,
loss, backward, SGD) on synthetic device batches, and beside it, in the same process and alternating with it: the same stack
as torch.nn modules with BatchNorm2d, the yolo355.grad criterion and torch.optim.SGD, in fp32 and under bf16 autocast; and the
step of the BN-folded network (yolo355.train.SlimTrainer.step) at the same shape:

    python -m yolo355.tools.bntrain_bench [--config 32x240x320 64x416x416 --classes 20 --reps 30 --out FILE]
    python -m yolo355.tools.bntrain_bench --only-ours --reps 5     # the run rocprofv3 --kernel-trace --stats wraps

After two warm-up rounds: the median over --reps repetitions of the wall clock around one call that ends synchronised.  Beside
the times, the bytes each of the five BatchNorm kernels must move in one step (Z, dY, A, I, G at two bytes an element, one an
index, summed over the nine layers): a kernel trace's times set against them give the bandwidth reached.  Prints one JSON line
per configuration; --out writes them as a list."""
import argparse
import json
import statistics
import time

import torch

from .train_bench import CONVS, step_macs

POOLED = (0, 1, 3, 5)


def bn_bytes(B, h, w):
    """{kernel: bytes it must read + write in one step} over the nine BatchNorm layers (the per-channel arrays are noise)"""
    out = dict(bn_stats_fwd=0, bn_norm=0, bn_stats_bwd=0, bn_apply=0)
    for i, (_, c, d) in enumerate(CONVS):
        z = 2 * B * (h // d) * (w // d) * c                                  # Z_k, dY_k or G_k
        out["bn_stats_fwd"] += z
        out["bn_norm"] += z + (z // 4 + z // 8 if i in POOLED else z)        # reads Z; writes A (and I, one byte an element)
        out["bn_stats_bwd"] += 2 * z
        out["bn_apply"] += 3 * z
    return out


def torch_stack(pred_channels, device):
    import torch.nn as nn
    layers = []
    for i, (cin, cout, _) in enumerate(CONVS):
        layers += [nn.Conv2d(cin, cout, 3, 1, 1), nn.BatchNorm2d(cout), nn.LeakyReLU(0.125)]
        if i in POOLED:
            layers.append(nn.MaxPool2d(2, 2))
    layers.append(nn.Conv2d(256, pred_channels, 3, 1, 1))
    return nn.Sequential(*layers).to(device).train()


def run(cfg, a):
    from yolo355 import synth
    from yolo355.bntrain import SlimBNTrainer
    from yolo355.grad import YoloCriterion
    from yolo355.tools.grad_bench import bench_labels
    from yolo355.train import SlimTrainer
    B, H, W = cfg
    A, C = 5, a.classes
    ch = A * (5 + C)
    labels, counts = bench_labels(B, 2.4, C)
    layers = synth.make_fp32_model("slim_yolo_v2", 5, C, A)
    t = SlimBNTrainer([H, W], C, synth.ANCHOR_SIZE, B, a.lr)
    t.load_state_dict(synth.state_dict_fp32(layers))
    x = torch.from_numpy(synth.make_images(9, B, H, W, "noise")).to(t.device)
    res = dict(batch=B, height=H, width=W, classes=C, reps=a.reps, lr=a.lr)
    nets, folded = {}, None
    if not a.only_ours:
        folded = SlimTrainer([H, W], C, synth.ANCHOR_SIZE, B, a.lr)
        folded.load_state_dict(t.fused_state_dict(corrected=True))
        folded.criterion().set_labels(labels)
        crit = YoloCriterion([H, W], 16, synth.ANCHOR_SIZE, C, max_batch=B, max_labels_per_image=max(1, int(counts.max())))
        for mode in ("fp32", "bf16_autocast"):
            net = torch_stack(ch, t.device)
            with torch.no_grad():
                convs = [m for m in net if isinstance(m, torch.nn.Conv2d)]
                bns = [m for m in net if isinstance(m, torch.nn.BatchNorm2d)]
                for m, L in zip(convs, layers):
                    m.weight.copy_(torch.from_numpy(L["w"]))
                    m.bias.copy_(torch.from_numpy(L["b"]))
                for m, L in zip(bns, layers):
                    for dst, src in zip((m.weight, m.bias, m.running_mean, m.running_var), L["bn"]):
                        dst.copy_(torch.from_numpy(src))
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

    steps = {"ours": lambda: float(t.step(x)[3])}
    if folded is not None:
        steps["folded"] = lambda: float(folded.step(x)[3])
    for mode in nets:
        steps[mode] = lambda mode=mode: torch_step(mode)
    times = {k: [] for k in steps}
    first = {}
    t.criterion().set_labels(labels)
    for rep in range(a.reps + 2):                                           # two warm-up rounds
        for name, fn in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            first.setdefault(name, v)
            if rep >= 2:
                times[name].append(dt)
    _, step = step_macs(H, W, ch)
    ms = 1e3 * statistics.median(times["ours"])
    res.update(step_ms=ms, images_per_s=B / (ms * 1e-3), step_gmac_per_image=step * 1e-9, first_total_loss=first["ours"],
               bn_kernel_bytes=bn_bytes(B, H, W), stats_plan={k: t.stats_plan(k) for k in range(1, 10)})
    if folded is not None:
        res["folded_step_ms"] = 1e3 * statistics.median(times["folded"])
        res["folded_first_total_loss"] = first["folded"]
        folded.close()
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
    ap.add_argument("--only-ours", action="store_true", help="leave the torch and folded steps out (a kernel trace of the library alone)")
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
