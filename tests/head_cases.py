"""Adversarial inputs for the detection head / NMS (csrc/head_nms.hip) and the CPU-side checks that go with them.

Nothing here needs a GPU.  Two harnesses use these generators (tests/test_head_adversarial.py):

  E  Engine.head_nms on crafted int8 prediction maps; the oracle's NMS runs on the GPU's own decoded candidates
     (Engine.candidates), so the comparison is np.array_equal and a threshold may sit exactly on a pair's IoU;
  H  engine.head_f32 on fp32 maps against oracle.fp32_oracle; there is no tap, so every input must satisfy h_guards():
     no decision of the oracle may depend on the last ulp of the decode.

A generator returns a dict.  E: pq int8 [B, A*(5+C), Hs, Ws], sa, size [H, W], anchors (grid units), C, conf, thr.
H: preds (list of fp32 [B, A*(5+C), hs, ws]), strides, anchors (pixels, [nlev*A][2]), C, size, conf.
Channel layout of a map (models/slim_yolo_v2.py:330-341): [A objectness | A*C class logits | A*4 tx ty tw th].

The route resolve_emit_kernel takes depends on the number of suppressing pairs of an image: at most REG_EDGES in the
register rounds (packed per wave after three rounds), up to LDS_EDGES with the tail in LDS, above that the sorted walk.
"""
import numpy as np

from oracle import fp32_oracle as F
from oracle import yolo_oracle as O

NMS_CAP = 4096
REG_EDGES = 7168
LDS_EDGES = 28672
AREA_MIN = 1e-10


# ------------------------------------------------------------------------------------------------- map helpers
def _blank(B, A, C, hs, ws, dtype, off):
    """a map with every anchor switched off (objectness `off`) and everything else 0"""
    m = np.zeros((B, A * (5 + C), hs, ws), dtype)
    m[:, :A] = off
    return m


def ch_cls(A, C, a, c=0):
    return A + a * C + c


def ch_box(A, C, a, k=0):
    return (1 + C) * A + a * 4 + k


def _one_hot(m, b, A, C, a, y, x, cls, hot):
    for c in range(C):
        m[b, ch_cls(A, C, a, c), y, x] = np.where(np.asarray(cls) == c, hot, -hot)


def rand_i8(rng, shape):
    return rng.randint(-127, 128, size=shape).astype(np.int8)


def dequant(pq, sa):
    return pq.astype(np.float32) * np.float32(2.0 ** -sa)


def best_class(prob):
    """(score, class) of every anchor as the reference's postprocess takes them (slim_yolo_v2.py:180-183)"""
    cls = np.argmax(prob, axis=-1)
    return np.take_along_axis(prob, cls[..., None], -1)[..., 0], cls


def e_decode(case):
    """oracle decode of an E case: (box [B,N,4], score [B,N], cls [B,N])"""
    box, prob = O.head_decode(dequant(case["pq"], case["sa"]), case["size"], case["anchors"], case["C"])
    sc, cl = best_class(prob)
    return box, sc, cl


def h_decode(case):
    """oracle decode of an H case: (box [B,N,4], score [B,N], cls [B,N], gap [B,N]); gap: the best class's softmax
    probability minus the runner-up's (inf for one class)"""
    box, prob = F.tiny_head_decode(case["preds"], case["size"], case["anchors"], case["C"], level_strides=tuple(case["strides"]))
    sc, cl = best_class(prob)
    if case["C"] > 1:
        top = np.sort(prob.astype(np.float64) / np.maximum(prob.sum(-1, keepdims=True, dtype=np.float64), 1e-300), axis=-1)
        gap = top[..., -1] - top[..., -2]
    else:
        gap = np.full(sc.shape, np.inf)
    return box, sc, cl, gap


def oracle_nms(box, score, cls, conf, thr, C):
    """the oracle's postprocess on decoded candidates (one image): (boxes, scores, classes, anchor indices)"""
    prob = np.zeros((box.shape[0], C), np.float32)
    prob[np.arange(box.shape[0]), cls] = score
    return O.postprocess(box, prob, conf, thr, C)


# ------------------------------------------------------------------------------------------------- pair statistics
def _ovr_rows(bx, area, i0, i1):
    """the reference's overlap (slim_yolo_v2.py:159-171) of boxes i0..i1 against all, in the dtype of bx"""
    t = bx.dtype.type
    a = bx[i0:i1, None, :]
    xx1, yy1 = np.maximum(a[..., 0], bx[None, :, 0]), np.maximum(a[..., 1], bx[None, :, 1])
    xx2, yy2 = np.minimum(a[..., 2], bx[None, :, 2]), np.minimum(a[..., 3], bx[None, :, 3])
    inter = np.maximum(t(1e-28), xx2 - xx1) * np.maximum(t(1e-28), yy2 - yy1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area[i0:i1, None] + area[None, :] - inter), inter


def pair_ious(box, score, cls, conf, dtype=np.float32, chunk=512):
    """every same-class pair of candidates (score >= conf) of one image: (i, j, ovr) with anchor indices i < j and the
    reference's formula evaluated in `dtype` (float32: bit for bit what the oracle and the kernel compute; the pair is
    symmetric in fp32: the sum of the two areas commutes).  Only pairs with ovr > 0 or NaN are returned."""
    idx = np.where(score >= np.float32(conf))[0]
    out_i, out_j, out_v = [], [], []
    for c in np.unique(cls[idx]):
        ii = idx[cls[idx] == c]
        bx = box[ii].astype(dtype)
        area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
        for i0 in range(0, len(ii), chunk):
            ovr, _ = _ovr_rows(bx, area, i0, min(i0 + chunk, len(ii)))
            r, q = np.where(~(ovr <= 0))
            keep = r + i0 < q
            out_i.append(ii[r[keep] + i0])
            out_j.append(ii[q[keep]])
            out_v.append(ovr[r[keep], q[keep]])
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, dtype)
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_v)


def suppressing(pairs, thr):
    """the pairs for which the reference's predicate holds: not (ovr <= thr) -- NaN suppresses"""
    i, j, v = pairs
    m = ~(v <= np.float32(thr))
    return i[m], j[m]


def chain_depth(edges, score):
    """nodes on the longest path of the suppressing pairs oriented by the NMS order (score desc, anchor index asc)"""
    i, j = edges
    if len(i) == 0:
        return 1
    rank = np.empty(len(score), np.int64)
    rank[np.argsort(-score, kind="stable")] = np.arange(len(score))
    src = np.where(rank[i] < rank[j], i, j)
    dst = np.where(rank[i] < rank[j], j, i)
    o = np.argsort(rank[dst], kind="stable")
    depth = np.ones(len(score), np.int64)
    for s, d in zip(src[o].tolist(), dst[o].tolist()):       # by rank of the later endpoint: its sources are final
        if depth[s] + 1 > depth[d]:
            depth[d] = depth[s] + 1
    return int(depth.max())


def areas(box):
    return (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])


def route(npairs):
    return "registers" if npairs <= REG_EDGES else ("lds_tail" if npairs <= LDS_EDGES else "fallback")


# ------------------------------------------------------------------------------------------------- E cases
E1_SHAPES = [(1, 1), (1.5, 1), (1, 1.5), (2, 2), (3, 1.5), (1.5, 3), (3, 3), (4, 2),
             (2, 4), (4, 4), (6, 3), (3, 6), (6, 6), (8, 4), (4, 8), (8, 8)]
# anchor scale of the three bands: random tw, th in +-4 spread the sizes over e^8, the scale sets how many of the boxes are
# large enough to overlap (counts per band in test_generators_reach_their_paths)
E1_SCALE = {("low", 2): 0.21, ("mid", 2): 0.37, ("high", 2): 0.8, ("low", 5): 0.3, ("mid", 5): 0.6, ("high", 5): 1.8}
E1_BAND = {"low": (1500, 6000), "mid": (9000, 22000), "high": (32000, None)}


def e1_full_capacity(band, C):
    """256 x 256, 16 x 16 cells, 16 anchors: N = 4096 = the candidate capacity, every anchor a candidate"""
    rng = np.random.RandomState(100 + C)
    A = 16
    pq = rand_i8(rng, (2, A * (5 + C), 16, 16))
    anchors = [[w * E1_SCALE[band, C], h * E1_SCALE[band, C]] for w, h in E1_SHAPES]
    return dict(pq=pq, sa=5, size=[256, 256], anchors=anchors, C=C, conf=1e-4, thr=0.5, band=E1_BAND[band])


def e2_dense():
    """208 x 208, the five mask anchors, random maps: 845 candidates per image with IoUs all over (0, 1)"""
    rng = np.random.RandomState(21)
    anchors = [[0.6, 0.9], [1.2, 1.0], [1.5, 2.5], [2.5, 1.6], [3.0, 3.0]]
    pq = rand_i8(rng, (2, 5 * 7, 13, 13))
    pq[:, ch_box(5, 2, 0, 2):: 4] //= 4            # tw, th in +-1: comparable sizes, many partial overlaps
    pq[:, ch_box(5, 2, 0, 3):: 4] //= 4
    return dict(pq=pq, sa=5, size=[208, 208], anchors=anchors, C=2, conf=0.01, thr=0.5)


def boundary_threshold(box, score, cls, conf, C, target, tries=200):
    """(v, ref_at_v, ref_below_v): v = the fp32 IoU nearest to `target` of a same-class pair whose higher-ranked box the
    oracle keeps at nms_thresh v, so that the pair is decided by `ovr <= v`: kept at v, suppressed at nextafter(v, 0)."""
    i, j, v = pair_ious(box, score, cls, conf)
    ok = np.isfinite(v) & (v > 0) & (v < 1)
    i, j, v = i[ok], j[ok], v[ok]
    for k in np.argsort(np.abs(v - np.float32(target)), kind="stable")[:tries]:
        thr = np.float32(v[k])
        below = np.nextafter(thr, np.float32(0))
        hi, lo = (i[k], j[k]) if (score[i[k]], -i[k]) > (score[j[k]], -j[k]) else (j[k], i[k])
        at = oracle_nms(box, score, cls, conf, thr, C)
        if hi not in at[3] or lo not in at[3]:
            continue
        under = oracle_nms(box, score, cls, conf, below, C)
        if lo in under[3]:
            continue
        return thr, at, under
    raise AssertionError("no deciding pair near %g" % target)


def e3_chain(clump):
    """32 x 2048, 2 x 128 cells, three anchors.  Anchors 0 and 1 (40 x 16 px, centres at a quarter and three quarters of
    the cell) all carry the same objectness byte and class 0: the NMS order is the anchor index, consecutive boxes are 8 px
    apart (IoU 32 / 48), boxes two apart 16 px (IoU 24 / 56 <= 0.5): every box suppresses its successor only, a row is one
    chain of 256.  Image 1 has a few boxes switched off and another row offset.  clump: anchor 2 (the whole image)
    switched on in 150 cells with class 1 and random objectness: 150 * 149 / 2 suppressing pairs beside the chain."""
    A, C, sa = 3, (2 if clump else 1), 5
    hs, ws = 2, 128
    rng = np.random.RandomState(31 + clump)
    pq = _blank(2, A, C, hs, ws, np.int8, -127)
    for b in range(2):
        for a, tx in ((0, -35), (1, 35)):                       # sigmoid(-+35 / 32) = 0.251 / 0.749
            pq[b, a] = 64
            pq[b, ch_box(A, C, a, 0)] = tx
            pq[b, ch_box(A, C, a, 1)] = 0 if b == 0 else 6
            if C > 1:
                pq[b, ch_cls(A, C, a, 0)] = 127
                pq[b, ch_cls(A, C, a, 1)] = -127
    pq[1, 0, 0, 110] = -127                          # image 1: row 0 breaks after 220 boxes
    pq[1, 1, 0, 110] = -127
    pq[1, 1, 1, 3] = -127
    if clump:
        for b in range(2):
            cell = rng.permutation(hs * ws)[:150]
            y, x = cell // ws, cell % ws
            pq[b, 2, y, x] = rng.randint(20, 127, size=150)
            pq[b, ch_cls(A, C, 2, 0), y, x] = -127
            pq[b, ch_cls(A, C, 2, 1), y, x] = 127
            pq[b, ch_box(A, C, 2, 2), y, x] = 32                 # e^1 x (2048 x 64 px): past every border from any cell
            pq[b, ch_box(A, C, 2, 3), y, x] = 32
    anchors = [[2.5, 1.0], [2.5, 1.0], [128.0, 4.0]]
    return dict(pq=pq, sa=sa, size=[32, 2048], anchors=anchors, C=C, conf=0.5, thr=0.5)


def _degenerate_layout(rng, hs, ws):
    """cells of the degenerate mix, per image: zero-area boxes, stacks of near-AREA_MIN boxes (three per cell, concentric),
    ordinary boxes -- some of them on the cells of the first two kinds"""
    cells = rng.permutation(hs * ws)
    zero, stack = cells[:70], cells[70:110]
    ordinary = np.concatenate([cells[100:200], cells[:20]])
    return zero, stack, ordinary


def e4_degenerate():
    """256 x 256, 16 x 16 cells, six unit anchors (16 px), sa_pred = 2.  Anchor 0: tw = th = -127 / 4: the box's corners
    coincide in fp32 (zero area).  Anchors 1-3: tw = th = k / 4 with k in -44 .. -30: sides 1e-6 .. 3.5e-5, areas 1e-12 .. 1e-9
    around AREA_MIN, three concentric per cell (neighbouring k: area ratio 0.6).  Anchors 4, 5: ordinary boxes.  All of
    class 0 (one-hot +-127 / 4: the softmax is exactly 1), a few ordinary boxes of class 1."""
    A, C, sa, hs, ws = 6, 2, 2, 16, 16
    rng = np.random.RandomState(41)
    pq = _blank(2, A, C, hs, ws, np.int8, -127)
    for b in range(2):
        zero, stack, ordinary = _degenerate_layout(rng, hs, ws)
        y, x = zero // ws, zero % ws
        pq[b, 0, y, x] = rng.randint(8, 127, size=len(zero))
        pq[b, ch_box(A, C, 0, 2), y, x] = -127
        pq[b, ch_box(A, C, 0, 3), y, x] = -127
        pq[b, ch_box(A, C, 0, 0), y, x] = rng.randint(-8, 9, size=len(zero))
        _one_hot(pq, b, A, C, 0, y, x, np.zeros(len(zero), int), 127)
        y, x = stack // ws, stack % ws
        for a in (1, 2, 3):
            k = rng.randint(-44, -29, size=len(stack))
            pq[b, a, y, x] = rng.randint(8, 127, size=len(stack))
            pq[b, ch_box(A, C, a, 2), y, x] = k
            pq[b, ch_box(A, C, a, 3), y, x] = k
            _one_hot(pq, b, A, C, a, y, x, np.zeros(len(stack), int), 127)
        y, x = ordinary // ws, ordinary % ws
        for a in (4, 5):
            n = len(ordinary)
            pq[b, a, y, x] = rng.randint(8, 127, size=n)
            for k in range(4):
                pq[b, ch_box(A, C, a, k), y, x] = rng.randint(-6, 7, size=n)
            _one_hot(pq, b, A, C, a, y, x, (rng.rand(n) < 0.2).astype(int), 127)
    return dict(pq=pq, sa=sa, size=[256, 256], anchors=[[1.0, 1.0]] * 4 + [[2.0, 2.0], [3.0, 2.0]], C=C, conf=0.5, thr=0.5)


def e5_single(passing):
    """16 x 16 input, one anchor: N = 1"""
    pq = np.zeros((2, 6, 1, 1), np.int8)
    pq[:, 0] = 100 if passing else -100
    pq[1, 2] = 17
    return dict(pq=pq, sa=5, size=[16, 16], anchors=[[0.5, 0.5]], C=1, conf=0.5, thr=0.5)


def e5_wide(C):
    """32 x 512: a 2 x 32 grid of cells and of bins"""
    rng = np.random.RandomState(52 + C)
    pq = rand_i8(rng, (2, 5 * (5 + C), 2, 32))
    return dict(pq=pq, sa=5, size=[32, 512], anchors=[[0.6, 0.9], [1.2, 1.0], [1.5, 2.5], [2.5, 1.6], [3.0, 3.0]], C=C, conf=0.01,
                thr=0.5)


def e5_empty_and_dense():
    """image 0 without a candidate, image 1 dense"""
    case = e2_dense()
    case["pq"] = case["pq"].copy()
    case["pq"][0, :5] = -127
    case["conf"] = 0.05                              # sigmoid(-127 / 32) = 0.0185
    return case


# ------------------------------------------------------------------------------------------------- H cases and guards
H_ANCHORS3 = [[10, 14], [23, 27], [37, 58], [81, 82], [135, 169], [34, 20], [60, 40], [100, 30], [30, 100], [120, 120],
              [16, 16], [50, 50], [90, 60], [60, 90], [110, 110]]


def _h_levels(size, strides):
    return [(size[0] // s, size[1] // s) for s in strides]


def h_random(seed, size, A, C, strides=(8, 16, 32), wh=4.0, obj_bias=0.0, hot=None):
    """random fp32 maps on every level: tx, ty in +-2, tw, th uniform in +-wh (areas from the whole image down to below
    2^-16 of it, aspect ratios up to e^(2 wh)), objectness in +-3 + obj_bias; hot: one-hot class logits of +-hot (the softmax
    is then exactly 1 on both sides), otherwise random logits in +-3"""
    rng = np.random.RandomState(seed)
    preds = []
    for hs, ws in _h_levels(size, strides):
        p = np.zeros((2, A * (5 + C), hs, ws), np.float32)
        p[:, :A] = rng.uniform(-3, 3, size=(2, A, hs, ws)) + obj_bias
        if hot is None:
            p[:, A:(1 + C) * A] = rng.uniform(-3, 3, size=(2, A * C, hs, ws))
        else:
            cls = rng.randint(0, C, size=(2, A, hs, ws))
            oh = np.where(np.arange(C)[None, None, :, None, None] == cls[:, :, None], hot, -hot)
            p[:, A:(1 + C) * A] = oh.reshape(2, A * C, hs, ws)
        box = rng.uniform(-1, 1, size=(2, A, 4, hs, ws))
        box[:, :, :2] *= 2.0
        box[:, :, 2:] *= wh
        p[:, (1 + C) * A:] = box.reshape(2, A * 4, hs, ws)
        preds.append(p.astype(np.float32))
    anchors = [H_ANCHORS3[(l * 5 + a) % 15] for l in range(len(strides)) for a in range(A)]
    return dict(preds=preds, strides=list(strides), anchors=anchors, C=C, size=list(size), conf=0.05, A=A, seed=seed)


def h_guards(case, thr, dec):
    """Conditions on an H input under which last-ulp differences of the decode cannot flip a decision of the oracle, evaluated
    in float64 on the oracle's decode `dec` (h_decode).  Returns dict(ok, iou, order, conf, union, cls): the smallest margins
    found (ok: all hold).
      iou    min |IoU - thr| over same-class candidate pairs (two boxes of area exactly 0: exempt)                  > 1e-4
      order  min score difference over same-class pairs with IoU > thr - 1e-4, and over pairs of two zero-area
             boxes (0 / 0 in the reference's formula: they suppress each other, the order decides which one stays)     > 1e-5
      conf   min |score - conf_thresh| over all anchors                                                               > 1e-5
      union  min union over same-class candidate pairs that are not both of area exactly 0                         >= 1e-9
      cls    min gap between the two largest class probabilities of a candidate (one-hot logits: 1)                 > 1e-5
    """
    box, score, cls, gap = dec
    conf = case["conf"]
    m = dict(iou=np.inf, order=np.inf, conf=np.inf, union=np.inf, cls=np.inf)
    for b in range(box.shape[0]):
        m["conf"] = min(m["conf"], float(np.abs(score[b].astype(np.float64) - conf).min()))
        idx = np.where(score[b] >= np.float32(conf))[0]
        if len(idx):
            m["cls"] = min(m["cls"], float(gap[b][idx].min()))
        for c in np.unique(cls[b][idx]):
            ii = idx[cls[b][idx] == c]
            bx = box[b][ii].astype(np.float64)
            sc = score[b][ii].astype(np.float64)
            ar = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
            for i0 in range(0, len(ii), 512):
                i1 = min(i0 + 512, len(ii))
                ovr, inter = _ovr_rows(bx, ar, i0, i1)
                union = ar[i0:i1, None] + ar[None, :] - inter
                upper = np.arange(i0, i1)[:, None] < np.arange(len(ii))[None, :]
                both0 = (ar[i0:i1, None] == 0) & (ar[None, :] == 0)
                live = upper & ~both0
                if live.any():
                    m["union"] = min(m["union"], float(union[live].min()))
                    m["iou"] = min(m["iou"], float(np.abs(ovr - thr)[live].min()))
                near = (live & (ovr > thr - 1e-4)) | (upper & both0)
                if near.any():
                    m["order"] = min(m["order"], float(np.abs(sc[i0:i1, None] - sc[None, :])[near].min()))
    m["ok"] = m["iou"] > 1e-4 and m["order"] > 1e-5 and m["conf"] > 1e-5 and m["union"] >= 1e-9 and m["cls"] > 1e-5
    return m


def h_reference(case, thr, dec):
    box, score, cls = dec[:3]
    return [oracle_nms(box[b], score[b], cls[b], case["conf"], thr, case["C"]) for b in range(box.shape[0])]


def find_seed(make, thrs, accept=None, seeds=range(200)):
    """the first seed for which make(seed) satisfies h_guards at every threshold of thrs (and accept(case, dec), the case's
    coverage condition) -- how the seeds below were chosen"""
    for seed in seeds:
        case = make(seed)
        dec = h_decode(case)
        if all(h_guards(case, t, dec)["ok"] for t in thrs) and (accept is None or accept(case, dec)):
            return seed
    raise AssertionError("no seed satisfies the guards")


# seeds: find_seed() over the thresholds the case runs at, e.g. find_seed(lambda s: h3_non_square(s), (0.5,));
# test_generators_reach_their_paths asserts the guards and the coverage conditions on every one of them
H1_THR = (0.3, 0.5, 0.75)
H1_SEED = {1: 43, 2: 22, 40: 1}
H1_BIAS = {1: -5.0, 2: -4.5, 40: -2.5}      # about 300 of the 1680 anchors pass conf_thresh 0.05
H2_SEED = {3: 1, 32: 0, 33: 1}
H2_ANCHORS = {3: None, 32: [[70, 80], [90, 70]] * 3, 33: [[70, 80], [90, 70]] * 3}
H2_MIN_PAIRS = {3: 100, 32: 200, 33: 200}
H3_SEED = 10
H4_SEED = 0
H5_SEED = 0


def h1_three_levels(C, seed=None):
    """128 x 128, strides 8 / 16 / 32, five anchors: N = 1680"""
    return h_random(H1_SEED[C] if seed is None else seed, [128, 128], 5, C, wh=4.0, obj_bias=H1_BIAS[C])


def h2_class_limits(C, seed=None):
    """two anchors, three levels, level 0 of 16 x 16 cells: C = 3 and 32 sort by class (32 classes x 16 x 16 bins do not fit
    4096: the bin grid shrinks), C = 33 stays on the area octaves.  C = 3 has 220 boxes per class: they are small, so that
    the 75 k same-class pairs stay clear of the threshold.  C = 32 and 33 have 20 per class: boxes of more than half the
    image (H2_ANCHORS, tw and th in +-0.5), so that a few hundred of the 6.7 k same-class pairs suppress."""
    case = h_random(H2_SEED[C] if seed is None else seed, [128, 128], 2, C, wh=1.5 if H2_ANCHORS[C] is None else 0.5, obj_bias=0.0,
                    hot=50.0)
    if H2_ANCHORS[C] is not None:
        case["anchors"] = H2_ANCHORS[C]
    return case


def h3_non_square(seed=None):
    """320 x 64: level 0 is 40 x 8 cells, the bin grid 16 x 8"""
    return h_random(H3_SEED if seed is None else seed, [320, 64], 3, 2, wh=2.0, obj_bias=-1.0)


def h5_degenerate(seed=None):
    """The degenerate mix of e4_degenerate on the area octaves: 128 x 128, three levels, three anchors, 48 one-hot classes
    (above the class-group limit).  Every zero-area and near-AREA_MIN box clamps into octave group 15, whose smallest area
    is then 0.  Within the guards: stacked near-AREA_MIN boxes of one class have a union below 1e-9 and stay with E4.
      class 0       60 zero-area boxes (tw = th = -40: the corners coincide in fp32) scattered over level 0, objectness
                    logits evenly spaced (scores at least 1e-3 apart), and a few ordinary boxes;
      classes 1-44  one box each of area 1e-12 .. 6e-11 (odd classes) or 1.7e-10 .. 1e-9 (even ones), alone of its kind in
                    its class, inside an ordinary box of that class (same cell, 30 px and more): union = the ordinary
                    area, IoU about 1e-10 / area;
      all classes   20 small boxes of areas 1e-6 .. 1e-5 (octave group 15 as well), 150 ordinary boxes on levels 1 and 2."""
    seed = H5_SEED if seed is None else seed
    rng = np.random.RandomState(500 + seed)
    A, C, size, strides = 3, 48, [128, 128], (8, 16, 32)
    anchors = [[16, 16], [16, 16], [30, 36], [34, 20], [60, 40], [30, 100], [50, 50], [90, 60], [110, 110]]
    levels = _h_levels(size, strides)
    preds = [_blank(2, A, C, hs, ws, np.float32, -20.0) for hs, ws in levels]

    def put(b, l, a, y, x, obj, cls, txy, twh):
        p = preds[l]
        p[b, a, y, x] = obj
        _one_hot(p, b, A, C, a, y, x, cls, 50.0)
        for k in range(2):
            p[b, ch_box(A, C, a, k), y, x] = txy[k]
            p[b, ch_box(A, C, a, 2 + k), y, x] = twh[k]

    for b in range(2):
        cells = rng.permutation(16 * 16)
        zero, tiny, small = cells[:60], cells[60:104], cells[104:124]
        n = len(zero)
        put(b, 0, 0, zero // 16, zero % 16, rng.permutation(np.linspace(-1.0, 3.0, n)), np.zeros(n, int),
            rng.uniform(-2, 2, size=(2, n)), np.full((2, n), -40.0))
        n = len(tiny)
        k = np.arange(n)
        area = np.where(k % 2 == 0, 10.0 ** rng.uniform(-12.0, -10.22, size=n), 10.0 ** rng.uniform(-9.77, -9.0, size=n))
        asp = rng.uniform(0.7, 1.4, size=n)
        side = np.stack([np.sqrt(area) * asp, np.sqrt(area) / asp]) * 128.0          # pixels
        put(b, 0, 1, tiny // 16, tiny % 16, rng.uniform(0.0, 3.0, size=n), 1 + k, rng.uniform(-1, 1, size=(2, n)), np.log(side / 16.0))
        put(b, 0, 2, tiny // 16, tiny % 16, rng.uniform(0.0, 3.0, size=n), 1 + k, rng.uniform(-1, 1, size=(2, n)),
            rng.uniform(0.0, 1.0, size=(2, n)))
        n = len(small)
        put(b, 0, 1, small // 16, small % 16, rng.uniform(0.0, 3.0, size=n), rng.randint(0, C, size=n), rng.uniform(-2, 2, size=(2, n)),
            rng.uniform(np.log(0.13 / 16), np.log(0.4 / 16), size=(2, n)))
        for l, count in ((1, 120), (2, 30)):
            hs, ws = levels[l]
            slot = rng.permutation(hs * ws * A)[:count]
            for a in range(A):
                cell = slot[slot % A == a] // A
                n = len(cell)
                cls = np.where(rng.rand(n) < 0.1, 0, rng.randint(0, C, size=n))
                put(b, l, a, cell // ws, cell % ws, rng.uniform(-1.0, 3.0, size=n), cls, rng.uniform(-2, 2, size=(2, n)),
                    rng.uniform(-1.0, 0.5, size=(2, n)))
    return dict(preds=preds, strides=list(strides), anchors=anchors, C=C, size=size, conf=0.05, A=A, seed=seed)


def h4_compaction(n_on, seed=None):
    """416 x 416, three levels, three anchors: N = 10647 > 4096, the head thresholds and compacts first.  Objectness -20
    everywhere except on n_on anchors (spread over the three levels); 20 one-hot classes, small boxes."""
    seed = H4_SEED if seed is None else seed
    rng = np.random.RandomState(seed)
    A, C, size, strides = 3, 20, [416, 416], (8, 16, 32)
    case = h_random(seed, size, A, C, strides, wh=1.0, hot=50.0)
    case["anchors"] = [[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]]
    n = [hs * ws * A for hs, ws in _h_levels(size, strides)]
    for b in range(2):
        on = np.sort(rng.permutation(sum(n))[:n_on])
        base = 0
        for l, p in enumerate(case["preds"]):
            hs, ws = p.shape[2:]
            sel = on[(on >= base) & (on < base + n[l])] - base          # anchor index within the level = cell * A + a
            obj = np.full((hs * ws, A), -20.0, np.float32)
            obj[sel // A, sel % A] = rng.uniform(0.0, 3.0, size=len(sel))
            p[b, :A] = obj.T.reshape(A, hs, ws)
            p[b, (1 + C) * A:].reshape(A, 4, hs, ws)[:, 2:] -= 1.5      # tw, th in -2.5 .. -0.5
            base += n[l]
    case["n_on"] = n_on
    return case
