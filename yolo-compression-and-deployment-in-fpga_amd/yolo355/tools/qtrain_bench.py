"""Times the quantisation-aware training step (yolo355.qtrain.SlimQatTrainer.step: the fake-quantised forward, loss,
straight-through backward, SGD and the requantisation of every tensor) on synthetic device batches, and beside it, in the same
process and alternating with it, the bf16 step it is built from (yolo355.train.SlimTrainer.step, the yardstick of
tools/train_bench.py) on the same weights, images and labels:

    python -m yolo355.tools.qtrain_bench [--config 32x240x320 64x416x416 --classes 20 --reps 30 --out FILE]

The activation exponents are calibrated on the batch itself before the clock starts (three rounds of forward +
update_trackers on fresh trackers).  After two warm-up rounds: the median over --reps repetitions of the wall clock around one
call that ends synchronised -- the whole step, and its three parts on their own (forward; loss + backward; update, which for
the quantised trainer includes the range reduction and the requantise-and-pack launch).  Prints one JSON line per
configuration with the ratio quantised / bf16; --out writes them as a list."""
import argparse
import json
import statistics
import time

import torch


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _parts(t, x):
    """(forward, loss + backward, update) seconds of one step run in its three parts"""
    crit = t.criterion()
    tf, pred = _timed(lambda: t.forward(x))
    if t._dpred is None or t._dpred.shape != pred.shape:
        t._dpred = torch.empty_like(pred)

    def back():
        crit.forward_backward([pred], grad_maps=[t._dpred])
        t.backward(t._dpred)
    tb, _ = _timed(back)
    tu, _ = _timed(t.update)
    return tf, tb, tu


def run(cfg, a):
    from yolo355 import synth
    from yolo355.qtrain import SlimQatTrainer
    from yolo355.tools.grad_bench import bench_labels
    from yolo355.train import SlimTrainer
    B, H, W = cfg
    C = a.classes
    labels, _ = bench_labels(B, 2.4, C)
    ws = [(w, b) for _, w, b in synth.make_weights(5, num_classes=C, weight_gain=2.0)]
    ts = {"bf16": SlimTrainer([H, W], C, synth.ANCHOR_SIZE, B, a.lr), "quantised": SlimQatTrainer([H, W], C, synth.ANCHOR_SIZE, B, a.lr)}
    x = torch.from_numpy(synth.make_images(9, B, H, W, "noise")).to(ts["bf16"].device)
    for t in ts.values():
        t.load_weights(ws)
        t.criterion().set_labels(labels)
    q = ts["quantised"]
    q.set_act_exponents([0] * 11)
    for _ in range(3):
        q.forward(x)
        q.trackers = None
        exps = q.update_trackers()
    q.forward(x)
    res = dict(batch=B, height=H, width=W, classes=C, reps=a.reps, lr=a.lr, act_exponents=exps, clipped=[int(v) for v in q.act_stats()[1]])
    step = {k: [] for k in ts}
    parts = {k: [] for k in ts}
    first = {}
    for rep in range(a.reps + 2):                                           # two warm-up rounds
        for name, t in ts.items():
            dt, out = _timed(lambda: t.step(x))
            first.setdefault(name, float(out[3]))
            p = _parts(t, x)
            if rep >= 2:
                step[name].append(dt)
                parts[name].append(p)
    for name in ts:
        ms = 1e3 * statistics.median(step[name])
        res["%s_step_ms" % name] = ms
        res["%s_images_per_s" % name] = B / (ms * 1e-3)
        for i, part in enumerate(("forward", "loss_backward", "update")):
            res["%s_%s_ms" % (name, part)] = 1e3 * statistics.median(p[i] for p in parts[name])
        res["%s_first_total_loss" % name] = first[name]
    res["ratio_quantised_over_bf16"] = res["quantised_step_ms"] / res["bf16_step_ms"]
    res["weight_exponents"] = q.weight_exponents()
    for t in ts.values():
        t.close()
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["32x240x320", "64x416x416"], help="BxHxW")
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--lr", type=float, default=1e-5)
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
