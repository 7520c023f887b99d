"""Inputs for the detection head above 4096 candidates per image (csrc/nms_large.hip; tests/test_head_large.py).

Nothing here needs a GPU.  The H inputs of head_cases (fp32 maps through engine.head_f32, against the fp32 oracle under
head_cases.h_guards) carried past the old capacity, and dense inputs that are compared on the GPU's own decode
(head_f32(..., return_candidates=True)), where no guard is needed: the oracle's NMS reads the very floats the kernels read.
"""
import numpy as np

import head_cases as HC

_DEC = {}


def h4_variant(n_on, C=20, seed=0):
    """head_cases.h4_compaction with the number of classes as a parameter (C = 20: the same arrays): 416 x 416, three levels,
    three anchors, N = 10647, objectness -20 except on n_on anchors per image, one-hot classes, small boxes.
    A copy of that generator's body, the order of its RNG calls included (head_cases.py is a fixed yardstick and hardcodes 20
    classes): the two must stay in step -- test_h4_variant_is_h4_compaction compares the arrays."""
    rng = np.random.RandomState(seed)
    A, size, strides = 3, [416, 416], (8, 16, 32)
    case = HC.h_random(seed, size, A, C, strides, wh=1.0, hot=50.0)
    case["anchors"] = [[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]]
    n = [hs * ws * A for hs, ws in HC._h_levels(size, strides)]
    for b in range(2):
        on = np.sort(rng.permutation(sum(n))[:n_on])
        base = 0
        for l, p in enumerate(case["preds"]):
            hs, ws = p.shape[2:]
            sel = on[(on >= base) & (on < base + n[l])] - base
            obj = np.full((hs * ws, A), -20.0, np.float32)
            obj[sel // A, sel % A] = rng.uniform(0.0, 3.0, size=len(sel))
            p[b, :A] = obj.T.reshape(A, hs, ws)
            p[b, (1 + C) * A:].reshape(A, 4, hs, ws)[:, 2:] -= 1.5
            base += n[l]
    case["n_on"] = n_on
    return case


def guarded(n_on, C=20):
    """(case, oracle decode) of h4_variant(n_on, C), computed once and shared by the tests; treat both as read-only"""
    key = (n_on, C)
    if key not in _DEC:
        case = HC.h4_compaction(n_on) if C == 20 else h4_variant(n_on, C)
        _DEC[key] = (case, HC.h_decode(case))
    return _DEC[key]


def dense_three_levels():
    """224 x 320, strides 8 / 16 / 32, three anchors: N = 4410, one class, objectness 3 .. 9: every anchor is a candidate,
    boxes of a few cells each with tw, th in +-1: thousands of suppressions in the one class"""
    case = HC.h_random(7, [224, 320], 3, 1, wh=1.0, obj_bias=6.0)
    case["thr"] = 0.5
    return case


def dense_10647():
    """416 x 416, three anchors per level: all 10647 anchors are candidates of two classes (random logits), the boxes up to
    the whole image (anchors up to 373 x 326 px, tw, th in +-1)"""
    case = HC.h_random(8, [416, 416], 3, 2, wh=1.0, obj_bias=6.0)
    case["anchors"] = [[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]]
    case["thr"] = 0.5
    return case


def one_image(case, b):
    """image b of an H case as a batch of one"""
    out = dict(case)
    out["preds"] = [p[b:b + 1].copy() for p in case["preds"]]
    return out


def mixed_batch():
    """B = 3 on the h4 geometry: no candidate, a few hundred, 6000"""
    big, few = guarded(6000)[0], h4_variant(300)
    preds = []
    for pb, pf in zip(big["preds"], few["preds"]):
        empty = pf[0:1].copy()
        empty[:, :3] = -20.0
        preds.append(np.concatenate([empty, pf[1:2], pb[0:1]]))
    out = dict(big)
    out["preds"] = preds
    return out
