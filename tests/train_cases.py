"""Inputs of the training tests (tests/test_train_ref.py, tests/test_train.py) and of their golden generator
(tests/golden/gen_golden_train.py): the smallest shapes at which the kernels of csrc/train.hip can still go wrong, weights from
yolo355.synth (seeded), images in synth.make_images' noise pattern, labels from loss_cases.random_labels."""
import functools

import numpy as np

import loss_cases as LC
from yolo355 import synth

ANCHORS = synth.ANCHOR_SIZE_MASK
STRIDE = 16
# tag -> (input size [h, w], batch, classes): odd maps and widths that are no multiple of a tile with an odd batch and 35
# prediction channels; 125 prediction channels; first layers that cross tile boundaries in both directions
CASES = {
    "t48x80_b3_c2": ([48, 80], 3, 2),
    "t64_b2_c20": ([64, 64], 2, 20),
    "t96x160_b1": ([96, 160], 1, 2),
    # The deployed regime of the weight gradient, just above its threshold (more than 524 288 input pixels: every layer's run is
    # then longer than 32 pixels, so each wave accumulates over several steps, runs start and end inside images and the number
    # of runs is at or near its cap; tests/test_train.py asserts it from y355_train_wgrad_plan).  26 x 28 maps at stride 16
    # with a last run of 8 pixels; 15 x 17 maps, eight image boundaries, an odd pixel count and 125 prediction channels.
    "t416x448_b3_c2": ([416, 448], 3, 2),
    "t240x272_b9_c20": ([240, 272], 9, 20),
    # 1 x 1 and 1 x 2 maps at stride 16: every tap but the centre (and one neighbour) is padding, the last pool maps 2 x 2 to 1 x 1
    "t16_b5_c2": ([16, 16], 5, 2),
    "t16x32_b3_c20": ([16, 32], 3, 20),
}
TAGS = list(CASES)                              # new cases go at the end: the seeds follow the index
DEEP = ["t416x448_b3_c2", "t240x272_b9_c20"]
GOLDEN_TAGS = list(TAGS)                        # the cases tests/golden/train.npz holds
LAYERS = ["conv1", "conv2", "conv3_1", "conv3_2", "conv4_1", "conv4_2", "conv5", "conv6", "conv7", "pred"]
POOL = [True, True, False, True, False, True, False, False, False, False]
FULL_LIMIT, SAMPLE_LIMIT = 20000, 4096          # the fixture stays below the largest one there is (fp32.npz)
ADDED_LIMIT = 512                               # ... so the cases after the first three keep this many elements of a gradient


def _seed(tag):
    return 100 + 10 * TAGS.index(tag)


@functools.lru_cache(maxsize=None)
def weights(tag):
    """[(w fp32 [cout,cin,3,3], b fp32 [cout])] of layers 1..10; gain 2 keeps activations and gradients O(1) down the stack"""
    C = CASES[tag][2]
    return [(w, b) for _, w, b in synth.make_weights(_seed(tag), num_classes=C, weight_gain=2.0, bias_gain=1.0)]


@functools.lru_cache(maxsize=None)
def images(tag):
    (h, w), B, _ = CASES[tag]
    return synth.make_images(_seed(tag) + 1, B, h, w, "noise")


def labels(tag):
    _, B, C = CASES[tag]
    return [LC.random_labels(_seed(tag) + 2 + b, 3 - b % 2, C) for b in range(B)]


def keys(k):
    """state_dict keys of layer k = 1..10"""
    n = LAYERS[k - 1]
    return (n + ".weight", n + ".bias") if n == "pred" else (n + ".convs.0.weight", n + ".convs.0.bias")


def state_dict(ws):
    import torch
    sd = {}
    for k, (w, b) in enumerate(ws, 1):
        kw, kb = keys(k)
        sd[kw], sd[kb] = torch.from_numpy(np.array(w)), torch.from_numpy(np.array(b))
    return sd


def sample_index(n, tag):
    """the elements of a flattened gradient of n elements the fixture keeps: all up to FULL_LIMIT, else a fixed stride that
    leaves at most SAMPLE_LIMIT; in the cases after the first three ADDED_LIMIT takes the place of both, with a stride that
    shares no factor with the nine taps (on a 1 x 1 map the centre tap alone is not padding)"""
    added = TAGS.index(tag) >= 3
    full, limit = (ADDED_LIMIT, ADDED_LIMIT) if added else (FULL_LIMIT, SAMPLE_LIMIT)
    if n <= full:
        return np.arange(n)
    step = -(-n // limit)
    while added and step % 3 == 0:
        step += 1
    return np.arange(0, n, step)


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))
