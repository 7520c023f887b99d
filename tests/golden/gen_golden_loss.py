#!/usr/bin/env python3
"""Golden vectors of the training targets and losses, from the REFERENCE itself -> tests/golden/loss.npz.

Runs only where the reference is checked out (import recipe of gen_golden.py); nothing of its source travels.  Inputs come
from tests/loss_cases.py (seeded), so only the reference's outputs are stored:

  tgt/<case>            tools.gt_creator / tools.multi_gt_creator on the label lists of loss_cases.target_labels: float64 [3, N, 11]
  loss/<case>/out       the four losses (fp32) of the reference's loss branch on loss_cases.loss_pred_maps / loss_labels: the
                        family's decode_boxes / scale, tools.iou_score, tools.loss -- the statements of
                        models/slim_yolo_v2.py:360-382 and models/tiny_yolo_v3.py:249-273 on given prediction maps
  loss/<case>/gap       |reference fp32 result - tests/loss_ref.py (fp32 terms, float64 sums)| per loss, not below one fp32
                        ulp of the reference's number (a float32 cannot be met closer than that)
  loss/nan/out          the case of loss_cases.nan_case(): [nan, finite, finite, nan]
  qbf/<it>/...          SlimYOLOv2_quantize_bnfuse(trainable=True)(x, target, quantization=True) on two batches, weights
                        quantized before the first: losses, gap, the int8 prediction map with its exponent, the 11 tracker scales

    python tests/golden/gen_golden_loss.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402

import torch  # noqa: E402
from yolo355 import synth  # noqa: E402
import loss_cases as LC  # noqa: E402
import loss_ref as R  # noqa: E402


def ref_targets(tools, tag, labels):
    size, strides, anchors = LC.GEOM[tag]
    if LC.is_multi(tag):
        return tools.multi_gt_creator(size, strides, labels, anchors)
    return tools.gt_creator(size, strides, labels, anchors)


def decoder(ref_mods, tag):
    """an object with the family's grid state on which the reference's decode_boxes runs"""
    size, strides, anchors = LC.GEOM[tag]
    ns = types.SimpleNamespace(device="cpu", stride=strides)
    if LC.is_multi(tag):
        cls = ref_mods["multi"]
        ns.anchor_size = torch.tensor(anchors).view(len(strides), len(anchors) // len(strides), 2)
        ns.anchor_number = ns.anchor_size.size(1)
        ns.grid_cell, ns.stride_tensor, ns.all_anchors_wh = cls.create_grid(ns, size)
    else:
        cls = ref_mods["one"]
        ns.anchor_size = torch.tensor(anchors)
        ns.anchor_number = len(anchors)
        ns.grid_cell, ns.all_anchor_wh = cls.create_grid(ns, size)
    ns.decode_xywh = lambda t: cls.decode_xywh(ns, t)
    ns.scale_torch = torch.tensor([[[size[1], size[0], size[1], size[0]]]]).float()
    ns.decode_boxes = lambda t: cls.decode_boxes(ns, t)
    return ns


def ref_loss(tools, dec, pred_maps, target, C):
    """the reference's loss branch on given prediction maps (the statements after the last convolution)"""
    A = dec.anchor_number
    conf, cls, box = [], [], []
    for p in pred_maps:
        p = torch.from_numpy(p)
        B, abC, H, W = p.size()
        p = p.permute(0, 2, 3, 1).contiguous().view(B, H * W, abC)
        conf.append(p[:, :, :A].contiguous().view(B, H * W * A, 1))
        cls.append(p[:, :, A:(1 + C) * A].contiguous().view(B, H * W * A, C))
        box.append(p[:, :, (1 + C) * A:].contiguous())
    conf, cls, box = torch.cat(conf, 1), torch.cat(cls, 1), torch.cat(box, 1)
    B, HW = box.shape[0], box.shape[1]
    box = box.view(B, HW, A, 4)
    with torch.no_grad():
        x1y1x2y2 = (dec.decode_boxes(box) / dec.scale_torch).view(-1, 4)
        box = box.view(B, -1, 4)
        target = torch.tensor(target).float()
        iou = tools.iou_score(x1y1x2y2, target[:, :, 7:].view(-1, 4)).view(B, -1, 1)
        label = torch.cat([iou, target[:, :, :7]], dim=2)
        out = tools.loss(pred_conf=conf, pred_cls=cls, pred_txtytwth=box, label=label, num_classes=C)
    return np.array([float(v) for v in out], np.float32)


def gap_of(ref_out, mine):
    with np.errstate(invalid="ignore"):
        g = np.abs(ref_out.astype(np.float64) - mine)
        return np.maximum(g, np.spacing(np.abs(ref_out)).astype(np.float64))


def main():
    ref = G.import_reference()
    tools = sys.modules["tools"]
    import importlib
    mods = {"one": ref.SlimYOLOv2, "multi": importlib.import_module("models.tiny_yolo_v3").YOLOv3tiny}
    out = {}
    for tag in LC.TARGET_CASES:
        t = ref_targets(tools, tag, LC.target_labels(tag))
        out["tgt/" + tag] = t
        mine = R.make_targets(LC.GEOM[tag][0], LC.GEOM[tag][1], LC.target_labels(tag), LC.GEOM[tag][2], LC.is_multi(tag))
        print("tgt", tag, t.shape, "positives", int((t[..., 0] == 1).sum()), "ignored", int((t[..., 0] == -1).sum()),
              "restatement max|diff| %.3g" % np.abs(t - mine).max())
    for tag, g, C, B in LC.LOSS_CASES:
        size, strides, anchors = LC.GEOM[g]
        labels, maps = LC.loss_labels(tag), LC.loss_pred_maps(tag)
        target = ref_targets(tools, g, labels)
        o = ref_loss(tools, decoder(mods, g), maps, target, C)
        mine, _ = R.loss(maps, target, strides, anchors, C, size, LC.wh_mul(g))
        out["loss/%s/out" % tag] = o
        out["loss/%s/gap" % tag] = gap_of(o, mine)
        print("loss", tag, o, "rel gap", np.abs(o - mine) / np.abs(o))
    labels, maps = LC.nan_case()
    size, strides, anchors = LC.GEOM["t64"]
    target = ref_targets(tools, "t64", labels)
    o = ref_loss(tools, decoder(mods, "t64"), maps, target, 2)
    mine, _ = R.loss(maps, target, strides, anchors, 2, size, 16.0)
    assert np.isnan(o[[0, 3]]).all() and np.isfinite(o[[1, 2]]).all() and np.isnan(mine[[0, 3]]).all(), (o, mine)
    out["loss/nan/out"] = o
    out["loss/nan/gap"] = np.nan_to_num(gap_of(o, mine), nan=0.0)
    print("loss nan", o, mine)

    # the q_bf model's own loss branch
    cfg = LC.QBF
    size, C = cfg["size"], cfg["classes"]
    anchors = ref.config.ANCHOR_SIZE_MASK
    assert anchors == synth.ANCHOR_SIZE_MASK
    model = ref.Q("cpu", input_size=size, num_classes=C, trainable=True, conf_thresh=0.01, nms_thresh=0.5, anchor_size=anchors)
    G.load_weights(model, synth.make_weights(**cfg["weights"], num_classes=C))
    model.train()
    q = ref.rbq
    q.quantized_layers.clear()
    q.init_quantize_net(model, 8)
    q.quantize_layers(8)
    grabbed = {}
    orig = ref.Tracker.quantize_activation

    def tap(self_t, activation, *a, **k):
        r = orig(self_t, activation, *a, **k)
        if self_t is model.a_tracker_pred:
            grabbed["pred"] = r.detach().numpy().copy()
        return r
    ref.Tracker.quantize_activation = tap
    try:
        for it, seed in enumerate(cfg["image_seeds"]):
            x = synth.make_images(seed, cfg["batch"], size[0], size[1], "blocks")
            target = tools.gt_creator(size, 16, LC.qbf_labels(it), anchors)
            res = model(torch.from_numpy(x), target=torch.tensor(target).float(), quantization=True)
            o = np.array([float(v) for v in res], np.float32)
            sa = int(torch.floor(torch.log2(model.a_tracker_pred.scale)).item())
            pq = np.round(grabbed["pred"].astype(np.float64) * 2.0 ** sa)
            assert np.abs(pq).max() <= 127 and np.array_equal(pq * 2.0 ** -sa, grabbed["pred"].astype(np.float64))
            mine, _ = R.loss([grabbed["pred"]], target, 16, anchors, C, size, 16.0)
            out["qbf/%d/out" % it] = o
            out["qbf/%d/gap" % it] = gap_of(o, mine)
            out["qbf/%d/pred_q" % it] = pq.astype(np.int8)
            out["qbf/%d/sa_pred" % it] = np.array([sa], np.int32)
            out["qbf/%d/scales" % it] = np.array([float(getattr(model, n).scale.item()) for n in
                                                  ["a_tracker_in", "a_tracker1", "a_tracker2", "a_tracker3_1", "a_tracker3_2", "a_tracker4_1",
                                                   "a_tracker4_2", "a_tracker5", "a_tracker6", "a_tracker7", "a_tracker_pred"]], np.float32)
            print("qbf", it, o, "rel gap", np.abs(o - mine) / np.abs(o), "sa_pred", sa, "max|q|", int(np.abs(pq).max()))
    finally:
        ref.Tracker.quantize_activation = orig
    path = os.path.join(HERE, "loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
