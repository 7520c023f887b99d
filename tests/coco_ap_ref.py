"""Literal restatement of the COCO bbox AP contract (points 2 to 10: what pycocotools' COCOeval computes in
evaluate / accumulate / summarize for iouType 'bbox' after loadRes), loops as written there: np.argsort(kind='mergesort'),
np.searchsorted, np.spacing(1).  tests/test_coco_ap_ref.py pins it with hand-worked known answers (and with pycocotools itself
wherever that package exists); it is the oracle of tests/test_coco_ap.py and the host yardstick of
yolo355/tools/apeval_bench.py --coco.  Checker only: nothing of the product imports it.

Data shapes:
    ground_truth   list per image of float64 rows (cls, x, y, w, h, area, iscrowd)
    detections     the engines' padded outputs: boxes f32 [N][max_det][4] x1 y1 x2 y2, scores f32 [N][max_det], cls i32 [N][max_det],
                   count i32 [N]
    image_ids      [N] distinct integers (None: 0 .. N - 1); images are evaluated in ascending id
"""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
P = 1.0 / (1.0 + 2.0 ** -52)                             # tp / (fp + tp + spacing(1)) at tp = 1, fp = 0


def bb_iou(d, g, crowd):
    """maskApi.c bbIou for one pair of x y w h boxes"""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return np.float64(0.0)
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return np.float64(0.0)
    i = w * h
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u


def load_res(boxes, scores, cls, count, i):
    """the data_dict entries of image i in list order: (position, class, [x, y, w, h], area, score) on float64"""
    out = []
    for p in range(int(count[i])):
        x1, y1, x2, y2 = (np.float64(v) for v in np.asarray(boxes, np.float32)[i, p])
        bbox = [x1, y1, x2 - x1, y2 - y1]
        out.append((p, int(cls[i, p]), bbox, bbox[2] * bbox[3], np.float64(np.float32(scores[i, p]))))
    return out


def evaluate_img(gt, dt, area_rng, iou_thrs, max_det):
    """COCOeval.evaluateImg for one (image, category, area range).  gt: rows (x, y, w, h, area, iscrowd) in annotation order; dt:
    load_res entries of the category in list order.  -> dict or None"""
    if len(gt) == 0 and len(dt) == 0:
        return None
    g_ignore = [bool(g[5]) or g[4] < area_rng[0] or g[4] > area_rng[1] for g in gt]
    gtind = np.argsort(np.array(g_ignore, dtype=np.int64), kind='mergesort') if len(gt) else np.zeros(0, np.int64)
    dtind = np.argsort(np.array([-d[4] for d in dt], dtype=np.float64), kind='mergesort') if len(dt) else np.zeros(0, np.int64)
    dt = [dt[i] for i in dtind[0:max_det]]
    gts = [gt[i] for i in gtind]
    iscrowd = [int(g[5]) for g in gts]
    T, G, D = len(iou_thrs), len(gts), len(dt)
    ious = np.zeros((D, G))
    for di, d in enumerate(dt):
        for gi, g in enumerate(gts):
            ious[di, gi] = bb_iou(d[2], g[0:4], iscrowd[gi])
    gtm = np.zeros((T, G), np.int64) - 1                  # the matched detection (index in dt), -1 = none
    dtm = np.zeros((T, D), np.int64) - 1                  # the matched ground truth (index in gts), -1 = none
    gt_ig = np.array([g_ignore[i] for i in gtind], dtype=bool)
    dt_ig = np.zeros((T, D), bool)
    if G and D:
        for tind, t in enumerate(iou_thrs):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] > -1 and not iscrowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = m
                gtm[tind, m] = dind
    a = np.array([d[3] < area_rng[0] or d[3] > area_rng[1] for d in dt], dtype=bool).reshape((1, D))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == -1, np.repeat(a, T, 0)))
    return dict(pos=[d[0] for d in dt], scores=np.array([d[4] for d in dt], np.float64), dtm=dtm, dt_ig=dt_ig, gtm=gtm, gt_ig=gt_ig,
                gtind=gtind)


def summarize(precision, recall, iou_thrs, max_dets):
    def one(ap, iou_thr, a, m):
        if ap:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == iou_thrs)[0]]
            s = s[:, :, :, a, m]
        else:
            s = recall
            s = s[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    M = len(max_dets) - 1
    return np.array([one(1, None, 0, M), one(1, .5, 0, M), one(1, .75, 0, M), one(1, None, 1, M), one(1, None, 2, M), one(1, None, 3, M),
                     one(0, None, 0, 0), one(0, None, 0, 1), one(0, None, 0, 2), one(0, None, 1, M), one(0, None, 2, M),
                     one(0, None, 3, M)], np.float64)


def evaluate(num_classes, ground_truth, boxes, scores, cls, count, image_ids=None, iou_thrs=None, rec_thrs=None, max_dets=None,
             area_rng=None):
    """-> dict(precision [T,R,K,A,M], recall [T,K,A,M], stats [12] or None (other than the default parameter shape), npig [K,A],
    matches {(image index, k, a): dict(pos, dtm, dt_ig, gt_marked)} with ground-truth indices in annotation order)"""
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, np.float64)
    rec_thrs = REC_THRS if rec_thrs is None else np.asarray(rec_thrs, np.float64)
    max_dets = MAX_DETS if max_dets is None else list(max_dets)
    area_rng = AREA_RNG if area_rng is None else area_rng
    N = len(ground_truth)
    ids = np.arange(N) if image_ids is None else np.asarray(image_ids)
    assert len(np.unique(ids)) == N
    order = np.argsort(ids, kind='mergesort')             # np.unique(imgIds): ascending id
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), num_classes, len(area_rng), len(max_dets)
    gts = [np.asarray(g, np.float64).reshape(-1, 7) for g in ground_truth]
    dts = [load_res(boxes, scores, cls, count, i) for i in range(N)]
    ev, matches = {}, {}
    for k in range(K):
        for i in range(N):
            gt = [tuple(r[1:7]) for r in gts[i] if r[0] == k]
            dt = [d for d in dts[i] if d[1] == k]
            for a in range(A):
                e = evaluate_img(gt, dt, area_rng[a], iou_thrs, max_dets[-1])
                ev[k, a, i] = e
                if e is not None:
                    inv = e["gtind"]                      # sorted position -> annotation order
                    dtm = np.where(e["dtm"] >= 0, inv[np.maximum(e["dtm"], 0)], -1) if len(inv) else e["dtm"]
                    marked = np.zeros(e["gtm"].shape, np.uint8)
                    marked[:, inv] = e["gtm"] > -1
                    matches[i, k, a] = dict(pos=np.array(e["pos"], np.int64), dtm=dtm, dt_ig=e["dt_ig"].astype(np.uint8), gt_marked=marked)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    npig_all = np.zeros((K, A), np.int64)
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                E = [ev[k, a, i] for i in order]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["scores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind='mergesort')
                dtm = np.concatenate([e["dtm"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ig"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gt_ig"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                npig_all[k, a] = npig
                if npig == 0:
                    continue
                tps = np.logical_and(dtm > -1, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm > -1), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    if nd:
                        recall[t, k, a, m] = rc[-1]
                    else:
                        recall[t, k, a, m] = 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, rec_thrs, side='left')
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    stats = summarize(precision, recall, iou_thrs, max_dets) if (T, R, A, M) == (10, 101, 4, 3) else None
    return dict(precision=precision, recall=recall, stats=stats, npig=npig_all, matches=matches)


def pad(dets):
    """[(boxes [n,4] x1 y1 x2 y2, scores [n], cls [n]) per image] -> the padded arrays"""
    N = len(dets)
    md = max([1] + [len(s) for _, s, _ in dets])
    boxes, scores, cls = np.zeros((N, md, 4), np.float32), np.zeros((N, md), np.float32), np.zeros((N, md), np.int32)
    count = np.zeros(N, np.int32)
    for i, (b, s, c) in enumerate(dets):
        n = len(s)
        count[i] = n
        if n:
            boxes[i, :n], scores[i, :n], cls[i, :n] = np.asarray(b, np.float32).reshape(n, 4), s, c
    return boxes, scores, cls, count


# box sizes of the synthetic sets: all three area ranges, and areas exactly on both borders (32 * 32 = 16 * 64 = 1024, 96 * 96 = 9216)
SIZES = [(12, 10), (20, 30), (32, 32), (16, 64), (40, 50), (64, 80), (96, 96), (72, 128), (120, 100), (200, 150)]


def synth_set(seed, num_images, num_classes, dets_per_image, max_boxes, crowd=0.15, score_decimals=2, used_classes=None,
              empty=True):
    """A seeded COCO-style set in 640 x 480 images: integer boxes with sizes from SIZES (the annotation's area is w * h, or a
    smaller 'segmentation' area for every third box), crowd share `crowd`; detections are jittered copies of boxes (duplicates,
    sometimes of the wrong class; several inside crowd boxes) or random boxes; scores rounded to score_decimals.  With `empty`,
    image 1 has no box, image 2 no detection, image 3 neither.  Image ids: a shuffled, non-contiguous set.
    -> (ground_truth, boxes, scores, cls, count, image_ids)"""
    rng = np.random.default_rng(seed)
    uc = num_classes if used_classes is None else used_classes
    gts, dets = [], []
    for i in range(num_images):
        nb = int(rng.integers(0, max_boxes + 1))
        nd = int(rng.poisson(dets_per_image))
        if empty and i in (1, 3):
            nb = 0
        if empty and i in (2, 3):
            nd = 0
        if empty and i == 2:
            nb = max(nb, 2)
        rows = []
        for j in range(nb):
            w, h = SIZES[int(rng.integers(0, len(SIZES)))]
            x, y = int(rng.integers(0, 640 - w)), int(rng.integers(0, 480 - h))
            area = float(w * h) if j % 3 else float(int(w * h * rng.uniform(0.4, 1.0)))
            rows.append([int(rng.integers(0, uc)), x, y, w, h, area, rng.random() < crowd])
        g = np.asarray(rows, np.float64).reshape(-1, 7)
        gts.append(g)
        b, s, c = np.zeros((nd, 4), np.float32), np.zeros(nd, np.float32), np.zeros(nd, np.int32)
        for k in range(nd):
            u = rng.random()
            if nb and u < 0.65:
                j = int(rng.integers(0, nb))
                x, y, w, h = g[j, 1:5]
                if g[j, 6] and rng.random() < 0.7:          # a detection inside a crowd region
                    fw, fh = rng.uniform(0.2, 0.6, 2)
                    x1, y1 = x + rng.uniform(0, w * (1 - fw)), y + rng.uniform(0, h * (1 - fh))
                    b[k] = (x1, y1, x1 + w * fw, y1 + h * fh)
                elif rng.random() < 0.3:                   # exact copy: IoU 1, and equal IoUs between duplicates
                    b[k] = (x, y, x + w, y + h)
                else:
                    b[k] = np.array([x, y, x + w, y + h]) + rng.normal(0, 0.04 * min(w, h), 4)
                c[k] = g[j, 0] if rng.random() < 0.9 else rng.integers(0, uc)
                s[k] = 0.25 + 0.75 * rng.random()
            else:
                w, h = SIZES[int(rng.integers(0, len(SIZES)))]
                x, y = rng.uniform(0, 640 - w), rng.uniform(0, 480 - h)
                b[k] = (x, y, x + w, y + h)
                c[k] = rng.integers(0, uc)
                s[k] = 0.75 * rng.random()
        if score_decimals is not None:
            s = np.round(s, score_decimals).astype(np.float32)
        dets.append((b, s, c))
    ids = rng.permutation(np.arange(7, 7 + 3 * num_images, 3))[:num_images].astype(np.int64)
    return (gts,) + pad(dets) + (ids,)
