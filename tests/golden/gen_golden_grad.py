#!/usr/bin/env python3
"""Golden vectors of the gradient of the training losses, from the REFERENCE itself -> tests/golden/grad.npz.

Runs only where the reference is checked out (import recipe of gen_golden.py), on the CPU; nothing of its source travels.
Inputs come from tests/loss_cases.py (seeded), so only the reference's outputs are stored.  For every 64-pixel entry of
loss_cases.LOSS_CASES and for loss_cases.nan_case() ("nan"): the reference's own tools.loss on requires_grad fp32 tensors cut
from the prediction maps, targets from its creators, the IoU under no_grad as its models take it, then backward()

  grad/<case>/total/<level>   from total_loss                    fp32 [B, A(5+C), hs, ws]: the gradient, permuted back to the
  grad/<case>/mix/<level>     from conf_loss + 2 * cls_loss      NCHW layout of the prediction map
  grad/<case>/total/gap       float64 [3]: per channel group (conf, cls, box) the largest |reference - tests/grad_ref.py| over
  grad/<case>/mix/gap         finite elements, not below one fp32 ulp of the group's largest |gradient|

The 416-pixel case is far larger than a fixture may be: it is checked against grad_ref alone.

    python tests/golden/gen_golden_grad.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402
import gen_golden_loss as GL  # noqa: E402

import torch  # noqa: E402
import grad_ref as GR  # noqa: E402
import loss_cases as LC  # noqa: E402

RUNS = {"total": (0.0, 0.0, 0.0, 1.0), "mix": (1.0, 2.0, 0.0, 0.0)}


def ref_grads(tools, dec, pred_maps, target, C, upstream):
    """backward() of the reference's loss branch on given prediction maps: the gradient arriving at each map"""
    A = dec.anchor_number
    leaves = [torch.from_numpy(p).clone().requires_grad_(True) for p in pred_maps]
    conf, cls, box = [], [], []
    for p in leaves:
        B, abC, H, W = p.size()
        q = p.permute(0, 2, 3, 1).contiguous().view(B, H * W, abC)
        conf.append(q[:, :, :A].contiguous().view(B, H * W * A, 1))
        cls.append(q[:, :, A:(1 + C) * A].contiguous().view(B, H * W * A, C))
        box.append(q[:, :, (1 + C) * A:].contiguous())
    conf, cls, box = torch.cat(conf, 1), torch.cat(cls, 1), torch.cat(box, 1)
    B, HW = box.shape[0], box.shape[1]
    box = box.view(B, HW, A, 4)
    target = torch.tensor(target).float()
    with torch.no_grad():
        x1y1x2y2 = (dec.decode_boxes(box) / dec.scale_torch).view(-1, 4)
        iou = tools.iou_score(x1y1x2y2, target[:, :, 7:].view(-1, 4)).view(B, -1, 1)
    label = torch.cat([iou, target[:, :, :7]], dim=2)
    out = tools.loss(pred_conf=conf, pred_cls=cls, pred_txtytwth=box.view(B, -1, 4), label=label, num_classes=C)
    sum(float(u) * o for u, o in zip(upstream, out) if u).backward()
    return [p.grad.numpy().copy() for p in leaves]


def gap_of(ref_maps, mine, A, C):
    gap, top = GR.group_gap(ref_maps, mine, A, C), GR.group_max(ref_maps, A, C)
    return np.array([max(gap[g], float(np.spacing(np.float32(top[g])))) for g in GR.GROUPS], np.float64)


def main():
    ref = G.import_reference()
    tools = sys.modules["tools"]
    import importlib
    mods = {"one": ref.SlimYOLOv2, "multi": importlib.import_module("models.tiny_yolo_v3").YOLOv3tiny}
    out = {}
    cases = [(tag, g, C, LC.loss_labels(tag), LC.loss_pred_maps(tag)) for tag, g, C, B in LC.LOSS_CASES if g != "m3_416"]
    cases.append(("nan", "t64", 2) + LC.nan_case())
    for tag, g, C, labels, maps in cases:
        size, strides, anchors = LC.GEOM[g]
        target = GL.ref_targets(tools, g, labels)
        A = LC.num_anchors(g)
        for run, up in RUNS.items():
            got = ref_grads(tools, GL.decoder(mods, g), maps, target, C, up)
            mine = GR.map_grads(maps, target, strides, anchors, C, size, LC.wh_mul(g), up)
            for a, b in zip(got, mine):
                assert np.array_equal(np.isnan(a), np.isnan(b)), (tag, run, "NaN pattern of the restatement")
            for l, a in enumerate(got):
                assert a.dtype == np.float32
                out["grad/%s/%s/%d" % (tag, run, l)] = a
            out["grad/%s/%s/gap" % (tag, run)] = gap_of(got, mine, A, C)
            top = GR.group_max(got, A, C)
            print(tag, run, "nan", int(sum(np.isnan(a).sum() for a in got)), "gap / max",
                  ["%.2g" % (v / top[k] if top[k] else 0.0) for k, v in zip(GR.GROUPS, out["grad/%s/%s/gap" % (tag, run)])])
    path = os.path.join(HERE, "grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
