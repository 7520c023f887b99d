"""Host restatement of the reference's anchor fit (generate_ab_kmeans.py:27-156): float64, every elementwise operation in the
order written there, every sum SEQUENTIAL in box order (np.cumsum adds one element after the other; np.sum adds pairwise and is
not used).  The yardstick of the GPU fit wherever the reference's own vectors (tests/golden/anchors.npz) do not reach."""
import numpy as np


def seq_sum(x):
    x = np.asarray(x, np.float64)
    return float(np.cumsum(x)[-1]) if len(x) else 0.0


def iou(w1, h1, w2, h2):
    """iou() :27-47, both boxes centred at 0; w1 / h1 arrays, w2 / h2 scalars"""
    S_1, S_2 = w1 * h1, w2 * h2
    I_w = np.minimum(0.0 + w1 / 2, 0.0 + w2 / 2) - np.maximum(0.0 - w1 / 2, 0.0 - w2 / 2)
    I_h = np.minimum(0.0 + h1 / 2, 0.0 + h2 / 2) - np.maximum(0.0 - h1 / 2, 0.0 - h2 / 2)
    I = I_w * I_h
    with np.errstate(divide="ignore", invalid="ignore"):
        v = I / (S_1 + S_2 - I)
    return np.where((I_w < 0) | (I_h < 0), 0.0, v)


def assign(boxes, cents):
    """-> (group int32 [n], min_distance [n], IoU with the chosen centroid [n]): group 0 and distance 1 to start with, a
    centroid wins only with distance < min_distance"""
    n = len(boxes)
    g, md, bi = np.zeros(n, np.int32), np.ones(n, np.float64), np.zeros(n, np.float64)
    for c, (cw, ch) in enumerate(np.asarray(cents, np.float64).reshape(-1, 2)):
        v = iou(boxes[:, 0], boxes[:, 1], cw, ch)
        d = 1.0 - v
        m = d < md
        md[m], g[m], bi[m] = d[m], c, v[m]
    return g, md, bi


def do_kmeans(k, boxes, cents):
    """do_kmeans :87-115 -> (new centroids [k, 2], groups, loss, counts)"""
    g, md, _ = assign(boxes, cents)
    new, counts = np.zeros((k, 2), np.float64), np.zeros(k, np.int32)
    for c in range(k):
        sel = boxes[g == c]
        counts[c] = len(sel)
        new[c] = [seq_sum(sel[:, 0]) / max(len(sel), 1), seq_sum(sel[:, 1]) / max(len(sel), 1)]
    return new, g, seq_sum(md), counts


def init_centroids(boxes, k, first, u):
    """init_centroids :50-84 with the draws given -> [k, 2], found centroids first, unfilled slots (0, 0)"""
    cents = [boxes[first]]
    for j in range(k - 1):
        _, D, _ = assign(boxes, cents)
        prefix = np.cumsum(D)
        thresh = prefix[-1] * u[j]
        above = np.nonzero(prefix > thresh)[0]
        if len(above):
            cents.append(boxes[above[0]])
    out = np.zeros((k, 2), np.float64)
    out[:len(cents)] = np.array(cents)
    return out


def fit(boxes, k, first=None, u=None, init_index=None, iters=1000, convergence=1e-6):
    """anchor_box_kmeans :118-156 -> dict(init, anchors, groups, counts, loss, losses (every step), iterations)"""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 2)
    init = boxes[np.asarray(init_index)].copy() if init_index is not None else init_centroids(boxes, k, int(first), u)
    cents, g, old_loss, counts = do_kmeans(k, boxes, init)
    losses, iterations = [old_loss], 1
    while True:
        cents, g, loss, counts = do_kmeans(k, boxes, cents)
        iterations += 1
        losses.append(loss)
        if abs(old_loss - loss) < convergence or iterations > iters:
            break
        old_loss = loss
    return dict(init=init, anchors=cents, groups=g, counts=counts, loss=loss, losses=np.array(losses), iterations=iterations)


def score(boxes, anchors):
    """-> (mean over the boxes of the IoU with the chosen anchor, counts [k], chosen anchor [n])"""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 2)
    anchors = np.asarray(anchors, np.float64).reshape(-1, 2)
    g, _, bi = assign(boxes, anchors)
    return seq_sum(bi) / len(boxes), np.bincount(g, minlength=len(anchors)).astype(np.int32), g

