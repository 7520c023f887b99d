"""Times the losses with their gradient on the GPU (yolo355.grad.YoloLossGrad.forward_backward) at loss_bench's VOC-like batch,
and beside it, on the same GPU and the same inputs, what a user would otherwise run: torch's own forward plus backward() of a
torch restatement of the loss branch (torch_loss_branch below: split of the maps, decode and IoU under no_grad, the four losses):

    python -m yolo355.tools.grad_bench [--arch slim_yolo_v2 tiny_yolo_v3 yolo_v3 --batch 64 --size 416 --classes 20 --reps 30 --out FILE]

After two warm-up rounds: the median over --reps repetitions of the wall clock around one call that ends synchronised
(forward_backward returns after its stream has finished; the torch path is followed by torch.cuda.synchronize()), the
prediction maps and the dense targets already on the device.  Prints one JSON line per head; --out writes them as a list.
--lib PATH times another build of libyolo355_grad.so (a variant of csrc/grad.hip's Y355_GRAD_CREG)."""
import argparse
import json
import statistics
import time

import numpy as np
import torch

GEOM = {"slim_yolo_v2": (16, "ANCHOR_SIZE"), "tiny_yolo_v3": ([16, 32], "TINY_MULTI_ANCHOR_SIZE"), "yolo_v3": ([8, 16, 32], "MULTI_ANCHOR_SIZE")}


def torch_loss(pred_conf, pred_cls, pred_txtytwth, label, num_classes, obj=5.0, noobj=1.0):
    """The four losses on pred_conf [B,N,1], pred_cls [B,N,C], pred_txtytwth [B,N,4], label [B,N,8] = iou, obj, cls, tx, ty,
    tw, th, weight, in plain torch operations of the inputs' dtype (masks as multiplications, sums over anchors, batch means):
    the 'mse' objectness form.  Differentiable by torch's autograd."""
    s = torch.sigmoid(pred_conf[..., 0])
    iou, t_obj, t_cls, t_box, wt = label[..., 0], label[..., 1], label[..., 2].long(), label[..., 3:7], label[..., 7]
    mask = (wt > 0).to(s.dtype)
    pos = ((t_obj == 1).to(s.dtype) * (s - iou) ** 2).sum(1).mean()
    neg = ((t_obj == 0).to(s.dtype) * s ** 2).sum(1).mean()
    conf_loss = obj * pos + noobj * neg
    ce = torch.nn.functional.cross_entropy(pred_cls.reshape(-1, num_classes), t_cls.clamp(0, num_classes - 1).reshape(-1), reduction="none")
    cls_loss = (ce.view_as(mask) * mask).sum(1).mean()
    xy = torch.nn.functional.binary_cross_entropy_with_logits(pred_txtytwth[..., :2], t_box[..., :2], reduction="none").sum(2)
    wh = ((pred_txtytwth[..., 2:] - t_box[..., 2:]) ** 2).sum(2)
    box_loss = (xy * wt * mask).sum(1).mean() + (wh * wt * mask).sum(1).mean()
    return conf_loss, cls_loss, box_loss, conf_loss + cls_loss + box_loss


def torch_loss_branch(maps, target, strides, anchors, num_classes, input_size, wh_mul):
    """the loss branch of a model on its prediction maps [B, A(5+C), hs, ws] (level 0 first) and the dense target [B,N,11]"""
    C = num_classes
    A = len(anchors) // len(strides)
    conf, cls, box, grid, stride, awh = [], [], [], [], [], []
    for lv, (p, s) in enumerate(zip(maps, strides)):
        B, ch, hs, ws = p.shape
        q = p.permute(0, 2, 3, 1).reshape(B, hs * ws, ch)
        conf.append(q[:, :, :A].reshape(B, -1, 1))
        cls.append(q[:, :, A:(1 + C) * A].reshape(B, -1, C))
        box.append(q[:, :, (1 + C) * A:].reshape(B, -1, 4))
        yy, xx = torch.meshgrid(torch.arange(hs, device=p.device), torch.arange(ws, device=p.device), indexing="ij")
        grid.append(torch.stack([xx, yy], -1).reshape(-1, 1, 2).expand(-1, A, 2).reshape(-1, 2).to(p.dtype))
        stride.append(torch.full((hs * ws * A, 1), float(s), device=p.device, dtype=p.dtype))
        awh.append(torch.tensor(anchors[lv * A:(lv + 1) * A], device=p.device, dtype=p.dtype).repeat(hs * ws, 1))
    conf, cls, box = torch.cat(conf, 1), torch.cat(cls, 1), torch.cat(box, 1)
    grid, stride, awh = torch.cat(grid), torch.cat(stride), torch.cat(awh)
    with torch.no_grad():
        cxy = (torch.sigmoid(box[..., :2]) + grid) * stride
        bwh = torch.exp(box[..., 2:]) * awh * wh_mul
        scale = torch.tensor([input_size[1], input_size[0], input_size[1], input_size[0]], device=box.device, dtype=box.dtype)
        a = torch.cat([cxy - bwh / 2, cxy + bwh / 2], -1) / scale
        b = target[..., 7:11]
        tl, br = torch.max(a[..., :2], b[..., :2]), torch.min(a[..., 2:], b[..., 2:])
        en = (tl < br).to(a.dtype).prod(-1)
        area_i = (br - tl).prod(-1) * en
        iou = area_i / ((a[..., 2:] - a[..., :2]).prod(-1) + (b[..., 2:] - b[..., :2]).prod(-1) - area_i)
        label = torch.cat([iou.unsqueeze(-1), target[..., :7]], -1)
    return torch_loss(conf, cls, box, label, C)


def bench_labels(batch, mean_labels, classes):
    """loss_bench's label lists"""
    from yolo355 import synth
    u = (synth.uniform_pm1(11, (batch,)).astype(np.float64) + 1.0) / 2.0
    counts = np.floor(u * 2.0 * mean_labels + 0.5).astype(int)
    labels = []
    for b, n in enumerate(counts):
        v = (synth.uniform_pm1(100 + b, (max(int(n), 1), 5)).astype(np.float64) + 1.0) / 2.0
        rows = []
        for cx, cy, sw, sh, c in v[:n]:
            w, h = 0.05 + 0.55 * sw, 0.05 + 0.55 * sh
            rows.append([max(cx - w / 2, 0.0), max(cy - h / 2, 0.0), min(cx + w / 2, 1.0), min(cy + h / 2, 1.0), int(c * classes) % classes])
        labels.append(rows)
    return labels, counts


def run(arch, a):
    from yolo355 import synth
    from yolo355.grad import YoloLossGrad
    strides, an = GEOM[arch]
    anchors = getattr(synth, an)
    size = [a.size, a.size]
    labels, counts = bench_labels(a.batch, a.labels, a.classes)
    h = YoloLossGrad(size, strides, anchors, a.classes, max_batch=a.batch, max_labels_per_image=max(1, int(counts.max())))
    dev = [torch.from_numpy(synth.uniform_pm1(500 + l, (a.batch, h.num_anchors * (5 + a.classes), hs, ws)) * np.float32(2.0)).to(h.device)
           for l, (hs, ws) in enumerate(h.grids)]
    h.set_labels(labels)
    target = h.targets().clone()
    t_fb, t_val, t_torch = [], [], []
    out = grads = t_out = None
    leaves = [d.clone().requires_grad_(True) for d in dev]
    for rep in range(a.reps + 2):                                           # two warm-up rounds
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, _, grads = h.forward_backward(dev)
        t1 = time.perf_counter()
        h.forward_backward(dev, with_grad=False)
        t2 = time.perf_counter()
        for p in leaves:
            p.grad = None
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        t_out = torch_loss_branch(leaves, target, h.strides, [tuple(v) for v in h.anchors.tolist()], a.classes, size,
                                  1.0 if h.multi else float(h.strides[0]))
        t_out[3].backward()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if rep >= 2:
            t_fb.append(t1 - t0)
            t_val.append(t2 - t1)
            t_torch.append(t4 - t3)
    top = max(float(g.abs().max()) for g in grads)
    diff = max(float((g - p.grad).abs().max()) for g, p in zip(grads, leaves))
    nbytes = sum(d.numel() * 4 for d in dev)
    res = dict(arch=arch, batch=a.batch, size=a.size, classes=a.classes, anchors_per_image=h.num_anchors_total, labels=int(counts.sum()),
               reps=a.reps, map_bytes_each_way=nbytes, gpu_forward_backward_ms=1e3 * statistics.median(t_fb),
               gpu_value_only_ms=1e3 * statistics.median(t_val), torch_forward_backward_ms=1e3 * statistics.median(t_torch),
               gpu_losses=[float(v) for v in out], torch_losses=[float(v.detach()) for v in t_out],
               max_grad_diff_over_max_grad=diff / top, lib=a.lib or "default")
    h.close()
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", nargs="+", default=sorted(GEOM), choices=sorted(GEOM))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--labels", type=float, default=2.4, help="mean labels per image (VOC07+12 trainval: about 2.4)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--lib", default=None, help="another build of libyolo355_grad.so")
    ap.add_argument("--out", default=None, help="write the results as a JSON list")
    a = ap.parse_args(argv)
    if a.lib:
        from yolo355 import grad
        grad.LIB_PATH = a.lib
    res = [run(arch, a) for arch in a.arch]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
