"""Host restatement of the gradient of the training losses with respect to the predictions, in float64, on top of
tests/loss_ref.py: the formulas of include/yolo355_grad.h per anchor, for the flat tensors tools.loss takes and for the NCHW
prediction maps.  The IoU that serves as the objectness label is loss_ref's fp32 number, a constant of the gradient (the
models take it under no_grad).  What tests/test_grad_ref.py pins to the goldens and to torch's float64 autograd, and what
tests/test_grad.py compares the GPU with."""
import numpy as np

import loss_ref as R

UNIT = (0.0, 0.0, 0.0, 1.0)          # upstream of total_loss.backward()
GROUPS = ("conf", "cls", "box")


def flat_grads(conf, cls, box, label, C, upstream=None, obj=5.0, noobj=1.0):
    """conf [B,N], cls [B,N,C], box [B,N,4], label [B,N,8] = iou, obj, cls, tx, ty, tw, th, weight -> float64
    (g_conf [B,N], g_cls [B,N,C], g_box [B,N,4]).  upstream: gradients arriving at conf_loss, cls_loss, txtytwth_loss,
    total_loss (None: 0, 0, 0, 1).  Masks are multiplications: 0 * nan stays nan."""
    conf, cls, box, label = (np.asarray(v, np.float64) for v in (conf, cls, box, label))
    u = np.asarray(UNIT if upstream is None else upstream, np.float64)
    B = conf.shape[0]
    k_conf, k_cls, k_box = (u[0] + u[3]) / B, (u[1] + u[3]) / B, (u[2] + u[3]) / B
    iou, t_obj, t_cls, t_box, wt = label[..., 0], label[..., 1], label[..., 2], label[..., 3:7], label[..., 7]
    with np.errstate(all="ignore"):
        s = 1.0 / (1.0 + np.exp(-conf))
        pos, neg, mask = (t_obj == 1.0).astype(np.float64), (t_obj == 0.0).astype(np.float64), (wt > 0.0).astype(np.float64)
        g_conf = ((obj * pos) * (2.0 * (s - iou)) + (noobj * neg) * (2.0 * s)) * (s * (1.0 - s)) * k_conf
        e = np.exp(cls - cls.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        kc = np.clip(t_cls.astype(np.int64), 0, C - 1)
        onehot = (np.arange(C) == kc[..., None]).astype(np.float64)
        g_cls = ((p - onehot) * mask[..., None]) * k_cls
        sxy = 1.0 / (1.0 + np.exp(-box[..., :2]))
        g_xy = (((sxy - t_box[..., :2]) * wt[..., None]) * mask[..., None]) * k_box
        g_wh = (((2.0 * (box[..., 2:] - t_box[..., 2:])) * wt[..., None]) * mask[..., None]) * k_box
    return g_conf, g_cls, np.concatenate([g_xy, g_wh], -1)


def label_of(pred_maps, target, strides, anchors, C, input_size, wh_mul):
    """(conf, cls, box, label [B,N,8]) of the map form: the flat tensors the models hand tools.loss, the IoU in fp32"""
    strides = [strides] if np.isscalar(strides) else list(strides)
    A = len(np.asarray(anchors).reshape(-1, 2)) // len(strides)
    grids = [p.shape[2:] for p in pred_maps]
    conf, cls, box = R.split_pred([np.asarray(p, np.float32) for p in pred_maps], A, C)
    t = np.asarray(target).astype(np.float32)
    iou = R.iou_score(R.decode(box, grids, strides, anchors, wh_mul, input_size), t[..., 7:11])
    return conf, cls, box, np.concatenate([iou[..., None], t[..., :7]], -1).astype(np.float32)


def to_maps(g_conf, g_cls, g_box, grids, A, C):
    """the inverse of loss_ref.split_pred: per level an NCHW map [B, A(5+C), hs, ws]"""
    out, n0 = [], 0
    B = g_conf.shape[0]
    for hs, ws in grids:
        n = hs * ws * A
        q = np.concatenate([g_conf[:, n0:n0 + n].reshape(B, hs * ws, A), g_cls[:, n0:n0 + n].reshape(B, hs * ws, A * C),
                            g_box[:, n0:n0 + n].reshape(B, hs * ws, A * 4)], -1)
        out.append(np.ascontiguousarray(np.transpose(q.reshape(B, hs, ws, A * (5 + C)), (0, 3, 1, 2))))
        n0 += n
    return out


def map_grads(pred_maps, target, strides, anchors, C, input_size, wh_mul, upstream=None):
    """float64 gradient maps, one per level, of the shapes of pred_maps"""
    conf, cls, box, label = label_of(pred_maps, target, strides, anchors, C, input_size, wh_mul)
    A = conf.shape[1] // sum(int(p.shape[2]) * int(p.shape[3]) for p in pred_maps)
    return to_maps(*flat_grads(conf, cls, box, label, C, upstream), [p.shape[2:] for p in pred_maps], A, C)


def group_slices(A, C):
    """channel slices of the three groups of a map: conf, cls, box"""
    return dict(conf=slice(0, A), cls=slice(A, A * (1 + C)), box=slice(A * (1 + C), A * (5 + C)))


def group_max(maps, A, C):
    """per group the largest finite |gradient| over all levels"""
    out = {}
    for g, sl in group_slices(A, C).items():
        v = np.concatenate([np.abs(np.asarray(m, np.float64)[:, sl]).reshape(-1) for m in maps])
        v = v[np.isfinite(v)]
        out[g] = float(v.max()) if v.size else 0.0
    return out


def group_gap(got, want, A, C):
    """per group the largest |got - want| over the elements finite in both"""
    out = {}
    for g, sl in group_slices(A, C).items():
        d = np.concatenate([np.abs(np.asarray(a, np.float64)[:, sl] - np.asarray(b, np.float64)[:, sl]).reshape(-1) for a, b in zip(got, want)])
        d = d[np.isfinite(d)]
        out[g] = float(d.max()) if d.size else 0.0
    return out


def assert_maps(got, want, gap, A, C, what):
    """got against golden maps: the same NaN pattern; finite elements within twice the recorded gap of the group and never
    more than 1e-5 of the group's largest |gradient| (loss_cases.golden_bound's rule, per channel group).  gap: dict or [3]."""
    gap = dict(zip(GROUPS, gap)) if not isinstance(gap, dict) else gap
    top = group_max(want, A, C)
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (what, "NaN pattern")
    err = group_gap(got, want, A, C)
    for g in GROUPS:
        bound = min(2.0 * float(gap[g]), 1e-5 * top[g])
        print(what, g, "err %.3g bound %.3g (gap %.3g, max %.3g)" % (err[g], bound, float(gap[g]), top[g]))
        assert err[g] <= bound, (what, g, err[g], bound)
