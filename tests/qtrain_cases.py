"""Inputs of the quantisation-aware training tests (tests/test_qtrain_ref.py, tests/test_qtrain.py): train_cases' weights,
images and labels, each case under two sets of activation exponents --

  "cal"     the exponents after one first-call calibration of the integer oracle (oracle/yolo_oracle.py) on the case's batch;
  "cal+1"   every exponent one higher, so that every tracker clips somewhere.

check(tag, eset) asserts from the oracle the conditions under which the fp32 forward of csrc/qtrain.hip is exact: the integer
accumulator and the pre-requantisation value t stay below 2^24, and torch's exponent rule agrees with the exact one on the
case's weights."""
import functools

import numpy as np

import train_cases as TC
from oracle import yolo_oracle as O

ANCHORS = TC.ANCHORS
CASES = TC.CASES
# odd maps and 35 prediction channels; 125 prediction channels at a size the int8 engine is run at; 1 x 1 and 1 x 2 maps
TAGS = ["t48x80_b3_c2", "t64_b2_c20", "t16_b5_c2", "t16x32_b3_c20"]
ENGINE_TAG = "t64_b2_c20"                         # the case the int8 Engine is compared on
CLIP_TAGS = ["t64_b2_c20", "t16_b5_c2"]           # over these two every tracker clips under "cal+1"
DEEP_TAG = TC.DEEP[1]                             # run-to-run bits only
SETS = ["cal", "cal+1"]
PAIRS = [(t, s) for t in TAGS for s in SETS]
PAIR_IDS = ["%s-%s" % p for p in PAIRS]
NUM_TRACKERS = 11

weights, images, labels = TC.weights, TC.images, TC.labels


@functools.lru_cache(maxsize=None)
def qlayers(tag):
    """[{q_w, e_w, q_b, e_b}] of the case's weights: the oracle's power-of-two recipe (torch's exponent rule)"""
    return O.quantize_layers([(TC.LAYERS[k], w, b) for k, (w, b) in enumerate(weights(tag))])


@functools.lru_cache(maxsize=None)
def calibrated(tag):
    """the eleven exponents of a first-call calibration of the oracle on the case's batch"""
    tr = [O.RangeTracker() for _ in range(NUM_TRACKERS)]
    r = O.forward_backbone_int(images(tag), qlayers(tag), tr, quant_freeze=True, keep=False)
    return tuple(int(v) for v in r["sa"])


def exponents(tag, eset):
    return [e + (1 if eset == "cal+1" else 0) for e in calibrated(tag)]


def frozen_trackers(sa):
    """oracle trackers that hold the exponents sa and do not move"""
    tr = [O.RangeTracker() for _ in range(NUM_TRACKERS)]
    for t, e in zip(tr, sa):
        t.first_a = 1
        t.scale = t.scale + float(2.0 ** e)
    return tr


@functools.lru_cache(maxsize=None)
def oracle(tag, eset):
    """forward_backbone_int(saturate=True) of the case at the set's exponents, with the maxima the trackers saw:
    max_abs[0] = max|x|, max_abs[k] = max|t'| 2^-F' of layer k (exact in fp32 while max|t'| < 2^24)"""
    sa = exponents(tag, eset)
    r = O.forward_backbone_int(images(tag), qlayers(tag), frozen_trackers(sa), quant_freeze=True, saturate=True, keep=True)
    assert list(r["sa"]) == sa
    mx = [np.float32(np.abs(images(tag)).max())] + [np.float32(g * 2.0 ** -O.RETUNE[k]) for k, g in enumerate(r["guard"])]
    r["max_abs"] = np.array(mx, np.float32)
    r["t_max"] = [g * 2.0 ** -O.RETUNE[k] * 2.0 ** _Fx(qlayers(tag)[k], sa[k], k) for k, g in enumerate(r["guard"])]
    return r


def _Fx(L, sa_in, k):
    return max(sa_in + L["e_w"], L["e_b"]) + (3 if O.LEAKY[k] else 0)


def exact_exponent(m):
    """floor(log2(fl32(127 / m))) taken as the exponent field of the fp32 quotient; 0 for m = 0, 127 where it overflows"""
    m = np.float32(m)
    if not m > 0:
        return 0
    with np.errstate(over="ignore", divide="ignore"):
        s = np.float32(127.0) / m
    f = int((np.array(s, np.float32).view(np.uint32) >> 23) & 0xff)
    return 127 if f == 0xff else f - 127


def check(tag, eset):
    """the conditions of exactness, from the oracle; returns (log2 acc_max, log2 t_max) over the layers"""
    r = oracle(tag, eset)
    acc, tm = max(r["acc_max"]), max(r["t_max"])
    assert acc < 2 ** 24 and tm < 2 ** 24, (tag, eset, acc, tm)
    for k, ((w, b), L) in enumerate(zip(weights(tag), qlayers(tag))):
        assert exact_exponent(np.abs(w).max()) == L["e_w"] and exact_exponent(np.abs(b).max()) == L["e_b"], (tag, k)
    return float(np.log2(max(acc, 1))), float(np.log2(max(tm, 1)))
