"""Host restatement of the reference's training targets and losses (tools.py:132-435 and the loss branch of the models,
e.g. models/slim_yolo_v2.py:360-382), written from their arithmetic: targets in float64 in the reference's operation order,
loss terms in float32, sums in float64.  What tests/test_loss_ref.py pins to the goldens and tests/test_loss.py compares
the GPU with."""
import numpy as np

F = np.float32


def level_grids(input_size, strides, multi):
    """[(hs, ws)] per level: round(h / s) for the one-level creator (tools.py:222-223), h // s for the multi-level one (:268)"""
    h, w = input_size
    if multi:
        return [(h // s, w // s) for s in strides]
    return [(int(round(h / strides[0])), int(round(w / strides[0])))]


def anchor_iou(anchors, bw, bh):
    """tools.compute_iou with both boxes centred at the origin; anchors float64 [n,2]"""
    aw, ah = anchors[:, 0], anchors[:, 1]
    i_w = np.minimum(0.0 + bw / 2, 0.0 + aw / 2) - np.maximum(0.0 - bw / 2, 0.0 - aw / 2)
    i_h = np.minimum(0.0 + bh / 2, 0.0 + ah / 2) - np.maximum(0.0 - bh / 2, 0.0 - ah / 2)
    s_i = i_h * i_w
    u = bw * bh + aw * ah - s_i + 1e-20
    return s_i / u


def label_writes(label, input_size, strides, anchors, multi, ignore_thresh=0.5):
    """The writes of one label, in the reference's order: [(level, gy, gx, a, fields or None)]; fields = the 11 values of a
    positive write, None = an ignore write (fields 0 and 6 become -1).  Empty for a box narrower than one pixel."""
    h, w = input_size
    xmin, ymin, xmax, ymax = (float(v) for v in label[:4])
    cls = int(label[4])
    c_x = (xmax + xmin) / 2 * w
    c_y = (ymax + ymin) / 2 * h
    box_w = (xmax - xmin) * w
    box_h = (ymax - ymin) * h
    if box_w < 1. or box_h < 1.:
        return []
    anchors = np.asarray(anchors, np.float64).reshape(-1, 2)
    A = len(anchors) // len(strides)
    if multi:
        bw, bh = box_w, box_h
    else:
        bw, bh = box_w / strides[0], box_h / strides[0]
    iou = anchor_iou(anchors, bw, bh)
    mask = iou > ignore_thresh
    best = int(np.argmax(iou))
    out = []
    for index in range(len(anchors)):
        if not (index == best or mask[index]):
            continue
        lv = index // A
        a = index - lv * A
        s = strides[lv]
        c_x_s, c_y_s = c_x / s, c_y / s
        gx, gy = int(c_x_s), int(c_y_s)
        if index == best:
            tw = np.log(bw / anchors[index, 0])
            th = np.log(bh / anchors[index, 1])
            weight = 2.0 - (box_w / w) * (box_h / h)
            out.append((lv, gy, gx, a, [1.0, cls, c_x_s - gx, c_y_s - gy, tw, th, weight, xmin, ymin, xmax, ymax]))
        else:
            out.append((lv, gy, gx, a, None))
    return out


def make_targets(input_size, strides, label_lists, anchors, multi, ignore_thresh=0.5, trace=None):
    """float64 [B, N, 11]: gt_creator (multi=False: one stride, anchors in grid units) or multi_gt_creator (anchors in pixels).
    Labels are applied in list order; a cell outside the grid is dropped.  trace (a list) receives (b, slot, kind) per write
    that landed, kind 1 = positive, 0 = ignore."""
    strides = [strides] if np.isscalar(strides) else list(strides)
    grids = level_grids(input_size, strides, multi)
    A = len(np.asarray(anchors).reshape(-1, 2)) // len(strides)
    base = np.cumsum([0] + [hs * ws * A for hs, ws in grids])
    t = np.zeros((len(label_lists), int(base[-1]), 11), np.float64)
    for b, labels in enumerate(label_lists):
        for label in labels:
            for lv, gy, gx, a, fields in label_writes(label, input_size, strides, anchors, multi, ignore_thresh):
                hs, ws = grids[lv]
                if not (0 <= gy < hs and 0 <= gx < ws):
                    continue
                slot = int(base[lv]) + (gy * ws + gx) * A + a
                if fields is None:
                    t[b, slot, 0] = -1.0
                    t[b, slot, 6] = -1.0
                else:
                    t[b, slot] = fields
                if trace is not None:
                    trace.append((b, slot, 0 if fields is None else 1))
    return t


def split_pred(pred_maps, A, C):
    """NCHW maps [B, A(5+C), hs, ws] per level -> conf [B,N], cls [B,N,C], txtytwth [B,N,4] in the head's anchor order"""
    conf, cls, box = [], [], []
    for p in pred_maps:
        B, ch, hs, ws = p.shape
        q = np.ascontiguousarray(np.transpose(p, (0, 2, 3, 1))).reshape(B, hs * ws, ch)
        conf.append(q[:, :, :A].reshape(B, hs * ws * A))
        cls.append(q[:, :, A:(1 + C) * A].reshape(B, hs * ws * A, C))
        box.append(q[:, :, (1 + C) * A:].reshape(B, hs * ws * A, 4))
    return np.concatenate(conf, 1), np.concatenate(cls, 1), np.concatenate(box, 1)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + np.exp(-x, dtype=F))).astype(F)


def decode(box, grids, strides, anchors, wh_mul, input_size):
    """fp32 x1y1x2y2 / [w,h,w,h] of every anchor, no clamp (decode_boxes of the family)"""
    anchors = np.asarray(anchors, F).reshape(len(strides), -1, 2)
    A = anchors.shape[1]
    gx, gy, st, aw, ah = [], [], [], [], []
    for (hs, ws), s, an in zip(grids, strides, anchors):
        yy, xx = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
        gx.append(np.repeat(xx.reshape(-1), A)); gy.append(np.repeat(yy.reshape(-1), A))
        st.append(np.full(hs * ws * A, s)); aw.append(np.tile(an[:, 0], hs * ws)); ah.append(np.tile(an[:, 1], hs * ws))
    gx, gy, st = (np.concatenate(v).astype(F) for v in (gx, gy, st))
    aw, ah = np.concatenate(aw).astype(F), np.concatenate(ah).astype(F)
    with np.errstate(all="ignore"):
        cx = (_sigmoid(box[..., 0]) + gx) * st
        cy = (_sigmoid(box[..., 1]) + gy) * st
        bw = (np.exp(box[..., 2], dtype=F) * aw) * F(wh_mul)
        bh = (np.exp(box[..., 3], dtype=F) * ah) * F(wh_mul)
        h, w = F(input_size[0]), F(input_size[1])
        return np.stack([(cx - bw / F(2)) / w, (cy - bh / F(2)) / h, (cx + bw / F(2)) / w, (cy + bh / F(2)) / h], -1).astype(F)


def _nanmax(a, b):
    return np.where(np.isnan(a) | np.isnan(b), F(np.nan), np.maximum(a, b))


def _nanmin(a, b):
    return np.where(np.isnan(a) | np.isnan(b), F(np.nan), np.minimum(a, b))


def iou_score(a, b):
    """tools.iou_score (:377-389) in fp32 on [..., 4] arrays"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        tlx, tly = _nanmax(a[..., 0], b[..., 0]), _nanmax(a[..., 1], b[..., 1])
        brx, bry = _nanmin(a[..., 2], b[..., 2]), _nanmin(a[..., 3], b[..., 3])
        area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        en = (tlx < brx).astype(F) * (tly < bry).astype(F)
        area_i = ((brx - tlx) * (bry - tly)) * en
        return (area_i / (area_a + area_b - area_i)).astype(F)


def loss_parts(pred_maps, target, strides, anchors, C, input_size, wh_mul):
    """float64 [B, 5] = pos, neg, cls, txty, twth of every image: fp32 terms (the reference's), float64 sums"""
    strides = [strides] if np.isscalar(strides) else list(strides)
    A = len(np.asarray(anchors).reshape(-1, 2)) // len(strides)
    grids = [p.shape[2:] for p in pred_maps]
    conf, cls, box = split_pred([np.asarray(p, F) for p in pred_maps], A, C)
    t = np.asarray(target).astype(F)
    with np.errstate(all="ignore"):
        iou = iou_score(decode(box, grids, strides, anchors, wh_mul, input_size), t[..., 7:11])
        pc = _sigmoid(conf)
        d = pc - iou
        pos = (t[..., 0] == 1).astype(F) * (d * d)
        neg = (t[..., 0] == 0).astype(F) * (pc * pc)
        mask = (t[..., 6] > 0).astype(F)
        m = cls.max(-1)
        lse = np.log(np.exp(cls - m[..., None], dtype=F).sum(-1, dtype=F), dtype=F)
        k = np.clip(t[..., 1].astype(np.int64), 0, C - 1)
        xc = np.take_along_axis(cls, k[..., None], -1)[..., 0]
        ce = (lse - (xc - m)) * mask
        x, tt = box[..., :2], t[..., 2:4]
        bce = (F(1) - tt) * x + (np.maximum(-x, F(0)) + np.log1p(np.exp(-np.abs(x), dtype=F), dtype=F))
        txty = (bce[..., 0] + bce[..., 1]) * t[..., 6] * mask
        e = box[..., 2:] - t[..., 4:6]
        e = e * e
        twth = (e[..., 0] + e[..., 1]) * t[..., 6] * mask
    return np.stack([v.astype(np.float64).sum(1) for v in (pos, neg, ce, txty, twth)], 1)


def combine(parts, obj=5.0, noobj=1.0):
    """(conf_loss, cls_loss, txtytwth_loss, total_loss) float64 of the [B,5] parts: batch means in image order"""
    B = parts.shape[0]
    mean = [sum(float(parts[b, k]) for b in range(B)) / B for k in range(5)]
    conf = obj * mean[0] + noobj * mean[1]
    box = mean[3] + mean[4]
    return np.array([conf, mean[2], box, conf + mean[2] + box], np.float64)


def loss(pred_maps, target, strides, anchors, C, input_size, wh_mul):
    parts = loss_parts(pred_maps, target, strides, anchors, C, input_size, wh_mul)
    return combine(parts), parts
