"""Inputs of the BatchNorm training tests (tests/test_bntrain_ref.py, tests/test_bntrain.py) and of their golden generator
(tests/golden/gen_golden_bntrain.py): parameters from yolo355.synth.make_fp32_model("slim_yolo_v2", ...) (seeded; gamma, beta
and the running statistics away from BatchNorm2d's defaults), images in synth.make_images' noise pattern, labels from
loss_cases.random_labels."""
import functools

import numpy as np

import loss_cases as LC
import train_cases as TC
from yolo355 import synth

ANCHORS = TC.ANCHORS
STRIDE = TC.STRIDE
LAYERS = TC.LAYERS
POOL = TC.POOL
DIV = [1, 2, 4, 4, 8, 8, 16, 16, 16, 16]         # layer k's pre-pool grid is the input's divided by DIV[k - 1]
COUT = [16, 32, 64, 64, 128, 128, 256, 256, 256]
# tag -> (input size [h, w], batch, classes)
CASES = {
    # the small shapes of tests/train_cases.py
    "b48x80_b3_c2": ([48, 80], 3, 2),
    "b64_b2_c20": ([64, 64], 2, 20),
    "b96x160_b1": ([96, 160], 1, 2),
    # the smallest legal statistics: N = 2 at layers 7..9 (two images of a 1 x 1 map, one image of a 1 x 2 map)
    "b16_b2_c2": ([16, 16], 2, 2),
    "b16x32_b1_c20": ([16, 32], 1, 20),
    # N odd at every layer from 3 on (9 x 60 x 68 ... 9 x 15 x 17); every reduction spans many runs, the last ones shorter
    "b240x272_b9_c20": ([240, 272], 9, 20),
    # one all-zero filter per layer (Z constant, var = 0, xhat = 0) and one negative gamma per layer (the order inside a
    # pooling window reverses)
    "b64_b2_c2_planted": ([64, 64], 2, 2),
}
TAGS = list(CASES)                               # new cases go at the end: the seeds follow the index
DEEP = "b240x272_b9_c20"
PLANTED = "b64_b2_c2_planted"
SMALLEST = ["b16_b2_c2", "b16x32_b1_c20"]
GOLDEN_TAGS = list(TAGS)


def _seed(tag):
    return 300 + 10 * TAGS.index(tag)


def planted_channels(k):
    """(the channel of layer k = 1..9 whose filter is all zero, the one whose gamma is negative)"""
    return (3 * k) % COUT[k - 1], (5 * k + 1) % COUT[k - 1]


@functools.lru_cache(maxsize=None)
def params(tag):
    """synth.make_fp32_model's list of dicts {name, w, b, bn (gamma, beta, running_mean, running_var) or None}, layers 1..10"""
    C = CASES[tag][2]
    layers = synth.make_fp32_model("slim_yolo_v2", _seed(tag), C, 5)
    if tag == PLANTED:
        for k in range(1, 10):
            L = layers[k - 1]
            zero, neg = planted_channels(k)
            assert zero != neg
            w, g = L["w"].copy(), L["bn"][0].copy()
            w[zero] = 0.0
            g[neg] = -g[neg]
            L["w"], L["bn"] = w, (g,) + tuple(L["bn"][1:])
    return layers


def state_dict(tag_or_layers):
    """the reference's state_dict of a case (torch tensors; num_batches_tracked left out, as synth.state_dict_fp32 does)"""
    import torch
    layers = params(tag_or_layers) if isinstance(tag_or_layers, str) else tag_or_layers
    return {k: torch.from_numpy(np.array(v)) for k, v in synth.state_dict_fp32(layers).items()}


@functools.lru_cache(maxsize=None)
def images(tag):
    (h, w), B, _ = CASES[tag]
    return synth.make_images(_seed(tag) + 1, B, h, w, "noise")


def labels(tag):
    _, B, C = CASES[tag]
    return [LC.random_labels(_seed(tag) + 2 + b, 3 - b % 2, C) for b in range(B)]


def sample_index(n, tag):
    """train_cases.sample_index: the first case keeps what its first three keep (every element of a gradient up to 20 000,
    else at most 4 096), the others what its added ones keep (at most 512): the fixture stays below fp32.npz"""
    return TC.sample_index(n, TC.TAGS[0 if TAGS.index(tag) == 0 else 3])


rel_l2 = TC.rel_l2
keys = TC.keys


def bn_keys(k):
    return tuple("%s.convs.1.%s" % (LAYERS[k - 1], f) for f in ("weight", "bias", "running_mean", "running_var"))
