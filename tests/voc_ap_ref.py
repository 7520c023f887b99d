"""NumPy restatement of the VOC AP contract (what write_voc_results_file + voc_eval + voc_ap of the
reference's utils/vocapi_evaluator_mask.py:140-336 compute), with the rank order the project defines: a STABLE sort of the
results-file order by score descending.  tests/test_voc_ap_ref.py pins it to the reference's own output bit for bit
(tests/golden/voc_ap.npz); it is the oracle for everything larger than that fixture, and the host yardstick of
yolo355/tools/apeval_bench.py.  Checker only: nothing of the product imports it.

Data shapes used throughout the VOC AP tests:
    ground_truth   list per image of rows (cls, xmin, ymin, xmax, ymax, difficult)
    detections     the engines' padded outputs: boxes f32 [N][max_det][4], scores f32 [N][max_det], cls i32 [N][max_det], count i32 [N]
"""
import numpy as np


def quantize_scores(s):
    """'{:.3f}' -> float() of the results file"""
    return np.rint(np.asarray(s, np.float32).astype(np.float64) * 1000.0) / 1000.0


def quantize_coords(b):
    """'{:.1f}'.format(coord + 1) -> float(): the + 1 is a float32 addition"""
    return np.rint((np.asarray(b, np.float32) + np.float32(1)).astype(np.float64) * 10.0) / 10.0


def voc_ap(rec, prec, use_07_metric=True):
    if use_07_metric:
        ap = 0.0
        for k in range(11):
            t = k * 0.1                                   # np.arange(0., 1.1, 0.1)[k]
            m = rec >= t
            p = np.max(prec[m]) if m.any() else 0.0
            ap = ap + p / 11.0
        return float(ap)
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]        # the envelope from the right
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def flatten(boxes, scores, cls, count):
    """padded outputs -> (image, position, class, score f32, box f32 [n,4]) of the meaningful entries, in file order"""
    count = np.asarray(count)
    img = np.repeat(np.arange(len(count)), count)
    pos = np.concatenate([np.arange(c) for c in count]) if len(count) else np.zeros(0, np.int64)
    return (img, pos, np.asarray(cls)[img, pos].astype(np.int64), np.asarray(scores, np.float32)[img, pos],
            np.asarray(boxes, np.float32)[img, pos])


def evaluate(num_classes, ground_truth, boxes, scores, cls, count, ovthresh=0.5, use_07_metric=True, quantize=True):
    """-> dict(ap [C], npos [C], ndet [C], mean, rec / prec / flag: per class arrays in rank order (flag 1 TP, 2 FP, 0 neither))"""
    img, pos, dcls, dsc, dbox = flatten(boxes, scores, cls, count)
    sq = quantize_scores(dsc) if quantize else dsc.astype(np.float64)
    bq = quantize_coords(dbox) if quantize else dbox.astype(np.float64)
    gt = [np.asarray(g, np.float64).reshape(-1, 6) for g in ground_truth]
    out = dict(ap=np.zeros(num_classes), npos=np.zeros(num_classes, np.int64), ndet=np.zeros(num_classes, np.int64), rec=[], prec=[], flag=[])
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(num_classes):
            recs = {}
            npos = 0
            for i, g in enumerate(gt):
                r = g[g[:, 0] == c]
                recs[i] = (np.ascontiguousarray(r[:, 1:5]), r[:, 5] != 0, np.zeros(len(r), bool))
                npos += int((r[:, 5] == 0).sum())
            sel = np.where(dcls == c)[0]                  # file order: image ascending, position ascending
            out["npos"][c], out["ndet"][c] = npos, len(sel)
            if len(sel) == 0:
                out["ap"][c] = -1.0
                for k in ("rec", "prec"):
                    out[k].append(np.zeros(0))
                out["flag"].append(np.zeros(0, np.uint8))
                continue
            order = sel[np.argsort(-sq[sel], kind="stable")]
            nd = len(order)
            tp, fp = np.zeros(nd), np.zeros(nd)
            for d, e in enumerate(order):
                bbgt, difficult, det = recs[int(img[e])]
                bb = bq[e]
                ovmax, jmax = -np.inf, -1
                if bbgt.size > 0:
                    iw = np.maximum(np.minimum(bbgt[:, 2], bb[2]) - np.maximum(bbgt[:, 0], bb[0]), 0.0)
                    ih = np.maximum(np.minimum(bbgt[:, 3], bb[3]) - np.maximum(bbgt[:, 1], bb[1]), 0.0)
                    inters = iw * ih
                    uni = (bb[2] - bb[0]) * (bb[3] - bb[1]) + (bbgt[:, 2] - bbgt[:, 0]) * (bbgt[:, 3] - bbgt[:, 1]) - inters
                    ov = inters / uni
                    ovmax, jmax = np.max(ov), int(np.argmax(ov))
                if ovmax > ovthresh:
                    if not difficult[jmax]:
                        if not det[jmax]:
                            tp[d] = 1.0
                            det[jmax] = True
                        else:
                            fp[d] = 1.0
                else:
                    fp[d] = 1.0
            out["flag"].append((tp + 2 * fp).astype(np.uint8))
            fpc, tpc = np.cumsum(fp), np.cumsum(tp)
            rec = tpc / float(npos)
            prec = tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)
            out["rec"].append(rec)
            out["prec"].append(prec)
            out["ap"][c] = voc_ap(rec, prec, use_07_metric)
    out["mean"] = float(np.mean(out["ap"]))
    return out


def all_boxes_to_padded(all_boxes):
    """all_boxes[cls][image] (N x 5 arrays or []) -> padded outputs; per image the classes in ascending order, which keeps every
    class's own file order"""
    C, N = len(all_boxes), len(all_boxes[0])
    per = [[(j, np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5)) for j in range(C)] for i in range(N)]
    count = np.array([sum(len(a) for _, a in p) for p in per], np.int32)
    md = max(1, int(count.max()) if N else 1)
    boxes, scores, cls = np.zeros((N, md, 4), np.float32), np.zeros((N, md), np.float32), np.zeros((N, md), np.int32)
    for i, p in enumerate(per):
        k = 0
        for j, a in p:
            boxes[i, k:k + len(a)], scores[i, k:k + len(a)], cls[i, k:k + len(a)] = a[:, :4], a[:, 4], j
            k += len(a)
    return boxes, scores, cls, count


def synth_set(seed, num_images, num_classes, dets_per_image, boxes_per_image, max_det=None, score_decimals=None, difficult=0.2,
              used_classes=None):
    """A seeded evaluation set: integer ground-truth boxes in a 500 x 375 image, detections that are jittered copies of boxes
    (sometimes several of one box: duplicates; sometimes of the wrong class) or random boxes.  score_decimals rounds the scores
    (ties).  used_classes: only the first that many classes occur.  -> (ground_truth, boxes, scores, cls, count)"""
    rng = np.random.default_rng(seed)
    uc = num_classes if used_classes is None else used_classes
    nd = rng.poisson(dets_per_image, num_images)
    md = int(max_det if max_det is not None else max(1, nd.max()))
    nd = np.minimum(nd, md)
    boxes = np.zeros((num_images, md, 4), np.float32)
    scores = np.zeros((num_images, md), np.float32)
    cls = np.zeros((num_images, md), np.int32)
    gts = []
    for i in range(num_images):
        nb = int(rng.poisson(boxes_per_image))
        x1, y1 = rng.integers(0, 400, nb), rng.integers(0, 300, nb)
        w, h = rng.integers(8, 100, nb), rng.integers(8, 75, nb)
        g = np.stack([rng.integers(0, uc, nb), x1, y1, x1 + w, y1 + h, rng.random(nb) < difficult], 1).astype(np.float64).reshape(-1, 6)
        gts.append(g)
        for k in range(nd[i]):
            if nb and rng.random() < 0.6:
                j = int(rng.integers(0, nb))
                boxes[i, k] = g[j, 1:5] + rng.normal(0, 2.5, 4)
                cls[i, k] = g[j, 0] if rng.random() < 0.9 else rng.integers(0, uc)
                scores[i, k] = 0.25 + 0.75 * rng.random()
            else:
                a, b = rng.uniform(0, 400), rng.uniform(0, 300)
                boxes[i, k] = (a, b, a + rng.uniform(5, 100), b + rng.uniform(5, 75))
                cls[i, k] = rng.integers(0, uc)
                scores[i, k] = 0.75 * rng.random()
    if score_decimals is not None:
        scores = np.round(scores, score_decimals).astype(np.float32)
    return gts, boxes, scores, cls, nd.astype(np.int32)
